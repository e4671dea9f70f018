""" Analysis of segmented stacks on the device: polygon ROIs -> filled masks + outlines -> per-frame statistics.

Reference: ``AnalysisWorker.analyze_data`` (src/inference/analysis.py:69-203) and ``make_coordinates`` (:214-234).  The
per-polygon CPU loop (skimage.draw.polygon / polygon_perimeter, label, regionprops) runs as HIP kernels
(csrc/analysis.hip, mseg_stack_relabel in csrc/postproc.hip); the OMERO I/O around it is not part of this build, so
``analyze_local`` is the local-file route.  DESIGN.md §6g states the recovered pixel rule and the reference quirks kept.
"""
import ctypes as C
import warnings
from pathlib import Path

import numpy as np
import pandas as pd
import torch

from .. import _lib
from ..utils.qt_shim import QObject, pyqtSignal, pyqtSlot

COLUMNS = ['frame', 'counts', 'mean_area', 'total_area', 'mean_minor_axis_length', 'mean_major_axis_length']
CAST_AT = 66535   # the reference's stack becomes int32 when cell_id reaches this value (analysis.py:136-137)


def make_coordinates(polystr, size_x, size_y):
    """ Convert polygon string to coordinates (reference analysis.py:214-234: Python ``round``, clamped to the image,
    tokens without a comma skipped)

    :return: Lists of coordinates r, c
    """
    r, c = [], []
    for textCoord in polystr.split(' '):
        coord = textCoord.split(',')
        if len(coord) == 1:
            continue
        r.append(np.minimum(np.maximum(int(round(float(coord[1]))), 0), size_y - 1))
        c.append(np.minimum(np.maximum(int(round(float(coord[0]))), 0), size_x - 1))
    return r, c


def _device(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("No MI355X visible: the analysis runs on the device (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def _csr(rois, height, width):
    """ROI records (``theT``, ``points``) -> (rc int32 [nv, 2], voff int64 [n + 1], frame int32 [n])"""
    rs, cs, lens, frames = [], [], [], []
    for roi in rois:
        r, c = make_coordinates(roi['points'], size_x=width, size_y=height)
        rs.extend(int(v) for v in r)
        cs.extend(int(v) for v in c)
        lens.append(len(r))
        frames.append(int(roi['theT']))
    rc = np.stack([np.asarray(rs, np.int32), np.asarray(cs, np.int32)], 1) if rs else np.zeros((0, 2), np.int32)
    voff = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=voff[1:])
    return np.ascontiguousarray(rc), voff, np.asarray(frames, np.int32)


def rois_to_device(rois, n_frames, height, width, device=None):
    """-> (mask int32 [T, H, W] relabelled per frame, k int32 [T], cast, outlines uint8 [T, H, W]) as device tensors;
    ``cast`` tells whether the reference's stack became int32 (at least 66 534 polygons)."""
    lib = _lib.load()
    dev = _device(device)
    T, H, W = int(n_frames), int(height), int(width)
    rc, voff, frame = _csr(rois, H, W)
    n = len(frame)
    st = _stream(dev)
    rc_d = torch.from_numpy(rc).to(dev) if rc.size else torch.zeros((1, 2), dtype=torch.int32, device=dev)
    voff_d = torch.from_numpy(voff).to(dev)
    fr_d = torch.from_numpy(frame).to(dev) if n else torch.zeros(1, dtype=torch.int32, device=dev)
    filled = torch.empty((T, H, W), dtype=torch.int32, device=dev)
    outl = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    ws = _ws(lib.mseg_roi_fill_workspace_bytes(n), dev)
    _lib.check(lib.mseg_roi_fill(rc_d.data_ptr(), voff_d.data_ptr(), fr_d.data_ptr(), n, T, H, W, filled.data_ptr(),
                                 ws.data_ptr(), ws.numel(), st), "roi_fill")
    _lib.check(lib.mseg_roi_outline(rc_d.data_ptr(), voff_d.data_ptr(), fr_d.data_ptr(), n, int(voff[-1]), T, H, W,
                                    outl.data_ptr(), st), "roi_outline")
    lab, k = relabel_stack(filled)
    return lab, k, n + 1 >= CAST_AT, outl


def relabel_stack(values):
    """skimage.measure.label(frame, background=0) for every frame of a uint16 / int32 [T, H, W] device tensor in one call
    -> (int32 labels, int32 components per frame).  Stacks of 2^31 pixels and more go in groups of frames."""
    lib = _lib.load()
    dev = values.device
    T, H, W = values.shape
    pix = {torch.int32: _lib_pix("I32"), torch.int16: _lib_pix("U16")}[values.dtype]   # uint16 data viewed as int16
    out = torch.empty((T, H, W), dtype=torch.int32, device=dev)
    k = torch.empty(T, dtype=torch.int32, device=dev)
    step = max(1, min(T, (2 ** 31 - 1) // (H * W)))
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        ws = _ws(lib.mseg_stack_relabel_workspace_bytes(t1 - t0, H, W), dev)
        _lib.check(lib.mseg_stack_relabel(values[t0:t1].data_ptr(), pix, t1 - t0, H, W, out[t0:t1].data_ptr(),
                                          k[t0:t1].data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "stack_relabel")
    return out, k


def _lib_pix(name):
    return {"U8": 0, "U16": 1, "I32": 2}[name]


def rois_to_masks(rois, n_frames, height, width, device=None):
    """ Polygon ROI records (``InferWorker.polygon_rois``: ``theT``, ``points``; in iteration order) -> (mask, outlines),
    the arrays of analysis.py:112-144 / result_export.py:112-144: the filled and per-frame relabelled stack (uint16, or
    int32 when the reference's cast happened and a frame holds more than 65535 cells) and the outlines (bool).

    Polygons with fewer than 3 distinct vertices (1-pixel instances of the tracer) make the reference raise in
    polygon_perimeter; here they are filled as skimage.draw.polygon fills them and outlined through their vertices. """
    lab, k, cast, outl = rois_to_device(rois, n_frames, height, width, device)
    return _host_mask(lab, cast), outl.bool().cpu().numpy()


def _host_mask(lab, cast):
    m = lab.cpu().numpy()
    if m.max(initial=0) > 65535:
        if not cast:
            raise ValueError("a frame holds more than 65535 cells in a uint16 stack: the reference's ids would wrap")
        return m
    return m.astype(np.uint16)


def _region_stats(lab, k):
    """device labels int32 [T, H, W] + components per frame -> per frame (counts, total_area, areas, major, minor)"""
    lib = _lib.load()
    dev = lab.device
    T, H, W = lab.shape
    kh = k.cpu().numpy().astype(np.int64)
    off = np.zeros(T + 1, np.int64)
    np.cumsum(kh, out=off[1:])
    n_lab = int(off[-1])
    off_d = torch.from_numpy(off).to(dev)
    area = torch.empty(max(n_lab, 1), dtype=torch.int64, device=dev)
    major = torch.empty(max(n_lab, 1), dtype=torch.float64, device=dev)
    minor = torch.empty(max(n_lab, 1), dtype=torch.float64, device=dev)
    total = torch.empty(T, dtype=torch.int64, device=dev)
    ws = _ws(lib.mseg_region_stats_workspace_bytes(n_lab), dev)
    _lib.check(lib.mseg_region_stats(lab.data_ptr(), T, H, W, off_d.data_ptr(), n_lab, area.data_ptr(), major.data_ptr(),
                                     minor.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
               "region_stats")
    area, major, minor = area.cpu().numpy(), major.cpu().numpy(), minor.cpu().numpy()
    total = total.cpu().numpy().view(np.uint64)
    return kh, off, total, area, major, minor


def _results(kh, off, total, area, major, minor):
    results = {c: [] for c in COLUMNS}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # np.mean([]) of an empty frame -> NaN, as in the reference
        for t in range(len(kh)):
            a, b = off[t], off[t + 1]
            present = area[a:b] > 0                            # regionprops lists the labels present in the frame
            results['frame'].append(t)
            results['counts'].append(int(kh[t]))
            results['total_area'].append(int(total[t]))
            results['mean_area'].append(np.mean(area[a:b][present]))
            results['mean_minor_axis_length'].append(np.mean(minor[a:b][present]))
            results['mean_major_axis_length'].append(np.mean(major[a:b][present]))
    return pd.DataFrame(results)


def analyze_masks(mask, device=None):
    """ Per-frame statistics of a [T, H, W] label stack, the table of analysis.py:151-170 (columns frame, counts,
    mean_area, total_area, mean_minor_axis_length, mean_major_axis_length).  Sums and moments on the device, the means of
    the per-cell arrays with np.mean on the host (the reference's pairwise summation).

    ``counts`` is np.max(mask[frame]) and ``total_area`` is np.sum(mask[frame]): the reference sums the LABEL VALUES of
    a frame, not its pixels, and this reproduces that.  A frame without cells has NaN means (np.mean([])), which
    ``to_csv`` writes as empty fields. """
    dev = _device(device)
    m = np.asarray(mask)
    if m.ndim == 2:
        m = m[None]
    if m.min(initial=0) < 0 or m.max(initial=0) > 2 ** 31 - 1:
        raise ValueError("label values must lie in 0 .. 2^31 - 1")
    lab = torch.from_numpy(np.ascontiguousarray(m.astype(np.int32))).to(dev)
    k = lab.reshape(lab.shape[0], -1).amax(1).to(torch.int32)
    return _results(*_region_stats(lab, k))


def analyze_device(lab, k):
    """analyze_masks for the device tensors of rois_to_device (no host copy of the stack)"""
    return _results(*_region_stats(lab, k))


def write_analysis(results_df, csv_path):
    results_df.to_csv(csv_path, index=False)


def analyze_local(rois, n_frames, height, width, csv_path, text_output=print, device=None):
    """ The Analysis button for local data: ROIs -> masks -> statistics -> ``csv_path``.  An all-empty result skips
    with the reference's message (analysis.py:146-148) and writes no file.  Returns the DataFrame or None. """
    lab, k, cast, _ = rois_to_device(rois, n_frames, height, width, device)
    k_max = int(k.max())
    if k_max == 0:
        text_output(f'  Skip {Path(csv_path).stem} (no segmentation results found)')
        return None
    if k_max > 65535 and not cast:
        raise ValueError("a frame holds more than 65535 cells in a uint16 stack: the reference's ids would wrap")
    df = analyze_device(lab, k)
    write_analysis(df, csv_path)
    return df


class AnalysisWorker(QObject):
    """ Worker class for the result analysis (reference analysis.py:12-212: same constructor, signals and slots).  The
    OMERO route is not part of this build: ``analyze_data`` raises like ``InferWorker.start_inference``; use
    ``analyze_local`` with the ROI records of ``InferWorker.polygon_rois``. """
    finished = pyqtSignal()  # Signal when import is finished
    progress = pyqtSignal(int)  # Signal for updating the progress bar
    text_output = pyqtSignal(str)  # Signal for possible exceptions, e.g., user interaction to stop export
    stop_analysis = False

    def __init__(self, img_id_list, results_path, omero_username, omero_password, omero_host, omero_port, group_id):
        super().__init__()
        self.img_id_list = img_id_list
        self.results_path = results_path
        self.omero_username = omero_username
        self.omero_password = omero_password
        self.omero_host = omero_host
        self.omero_port = omero_port
        self.group_id = group_id
        self.conn = None

    def analyze_data(self):
        """The reference pulls ROIs from an OMERO server here (analysis.py:69-203): not part of this build."""
        raise RuntimeError("AnalysisWorker.analyze_data needs the OMERO stack (omero-py), which is outside the "
                           "MI355X hot path; use microbeseg_amd.inference.analysis.analyze_local()")

    @pyqtSlot()
    def stop_analysis_process(self):
        """ Set internal export stop state to True """
        self.stop_analysis = True
