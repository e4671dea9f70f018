""" Export of segmented stacks: image, mask, overlay, outlines and analysis table as local files.

Reference: ``ResultExportWorker.export_data`` (src/inference/result_export.py:67-216).  Masks, outlines and the statistics
come from the device pipeline of ``analysis.py``; the overlay (result_export.py:183-190) is one HIP launch pair
(mseg_overlay_rgb).  The OMERO download is not part of this build: ``export_local`` takes the image stack and the ROI
records of ``InferWorker.polygon_rois`` and computes the CSV the reference downloads from the Analysis upload.
"""
from pathlib import Path

import numpy as np
import torch

from .. import _lib
from ..utils import tiffio as tiff
from ..utils.qt_shim import QObject, pyqtSignal, pyqtSlot
from .analysis import _device, _stream, _ws, analyze_device, rois_to_device, _host_mask


def check_overlay_input(img):
    """ValueError unless img is a uint8 / uint16 [T, H, W] or [T, H, W, C >= 3] array (what mseg_overlay_rgb takes)"""
    if img.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"overlay: uint8 or uint16 images only (got {img.dtype})")
    if not (img.ndim == 3 or (img.ndim == 4 and img.shape[-1] >= 3)):
        raise ValueError(f"overlay: expected [T, H, W] or [T, H, W, C >= 3], got shape {img.shape}")


def _overlay_device(img, outlines_dev):
    """img numpy uint8 / uint16 [T, H, W] or [T, H, W, C >= 3], outlines uint8 device tensor -> uint8 device tensor"""
    lib = _lib.load()
    img = np.asarray(img)
    check_overlay_input(img)
    pix = 0 if img.dtype == np.uint8 else 1
    Cin, Cout = (1, 3) if img.ndim == 3 else (img.shape[-1], img.shape[-1])
    T, H, W = img.shape[:3]
    if tuple(outlines_dev.shape) != (T, H, W):
        raise ValueError("overlay: outlines must be [T, H, W] like the image")
    dev = outlines_dev.device
    src = torch.from_numpy(np.ascontiguousarray(img).view(np.int16) if pix == 1 else np.ascontiguousarray(img))
    src = src.to(dev)
    out = torch.empty((T, H, W, Cout), dtype=torch.uint8, device=dev)
    ws = _ws(lib.mseg_overlay_workspace_bytes(), dev)
    _lib.check(lib.mseg_overlay_rgb(src.data_ptr(), pix, T, H, W, Cin, outlines_dev.data_ptr(), out.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream(dev)), "overlay_rgb")
    return out


def overlay(img, outlines, device=None):
    """ result_export.py:183-190: uint8(clip(255 * f32(img) / max(img), 0, 255)), a [T, H, W] image as three channels,
    outline pixels (255, 255, 0).  A 2-channel image raises ValueError (the reference raises IndexError). """
    dev = _device(device)
    o = torch.from_numpy(np.ascontiguousarray(np.asarray(outlines).astype(np.uint8))).to(dev)
    return _overlay_device(img, o).cpu().numpy()


def export_local(img, rois, result_path, name, text_output=print, device=None):
    """ The Export button for local data: writes ``<stem>.tif``, ``<stem>_mask.tif``, ``<stem>_overlay.tif``,
    ``<stem>_outlines.tif`` and ``<stem>_analysis.csv`` into ``result_path`` (names of result_export.py:201-210).
    img: uint8 / uint16, [T, H, W] or [T, H, W, C] with C >= 3 (every channel is written; the overlay changes channels
    0..2 of outline pixels); rois: ``InferWorker.polygon_rois`` records in iteration order.  Other dtypes or C == 2
    raise ValueError before any file is written.
    An all-empty result skips with the reference's message and writes nothing.  Returns the list of written paths. """
    img = np.asarray(img)
    check_overlay_input(img)
    T, H, W = img.shape[:3]
    stem = Path(name).stem
    lab, k, cast, outl = rois_to_device(rois, T, H, W, device)
    if int(k.max()) == 0:
        text_output(f'  Skip {stem} (no segmentation results found)')
        return []
    df = analyze_device(lab, k)
    mask = _host_mask(lab, cast)
    ov = _overlay_device(img, outl).cpu().numpy()
    result_path = Path(result_path)
    result_path.mkdir(parents=True, exist_ok=True)
    files = [result_path / f"{stem}{s}" for s in (".tif", "_mask.tif", "_overlay.tif", "_outlines.tif", "_analysis.csv")]
    tiff.imwrite(str(files[0]), img)
    tiff.imwrite(str(files[1]), mask)
    tiff.imwrite(str(files[2]), ov)
    tiff.imwrite(str(files[3]), outl.bool().cpu().numpy())
    df.to_csv(files[4], index=False)
    return files


class ResultExportWorker(QObject):
    """ Worker class for the result export (reference result_export.py:10-224: same constructor, signals and slots).  The
    OMERO route is not part of this build: ``export_data`` raises like ``InferWorker.start_inference``; use
    ``export_local``. """
    finished = pyqtSignal()  # Signal when import is finished
    progress = pyqtSignal(int)  # Signal for updating the progress bar
    text_output = pyqtSignal(str)  # Signal for possible exceptions, e.g., user interaction to stop export
    stop_export = False

    def __init__(self, img_id_list, inference_path, omero_username, omero_password, omero_host, omero_port, group_id):
        super().__init__()
        self.img_id_list = img_id_list
        self.omero_username = omero_username
        self.omero_password = omero_password
        self.omero_host = omero_host
        self.omero_port = omero_port
        self.group_id = group_id
        self.conn = None
        self.inference_path = inference_path  # path for local results

    def export_data(self):
        """The reference pulls images and ROIs from an OMERO server here (result_export.py:67-213): not part of this
        build."""
        raise RuntimeError("ResultExportWorker.export_data needs the OMERO stack (omero-py), which is outside the "
                           "MI355X hot path; use microbeseg_amd.inference.result_export.export_local()")

    @pyqtSlot()
    def stop_export_process(self):
        """ Set internal export stop state to True """
        self.stop_export = True
