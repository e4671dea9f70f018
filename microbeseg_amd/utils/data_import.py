""" Import of annotated images into a training set, on the device.

Reference: ``DataImportWorker.import_data`` (src/utils/data_import.py:24-278).  The reference cuts an annotated image into
a grid of crops, rejects nearly empty ones, uploads every kept crop with its polygon ROIs to an OMERO dataset, and training
later receives what ``DataExportWorker.export_data`` (src/utils/data_export.py:44-106) makes of that dataset: the image
rescaled to uint16 with the stored frame range and the polygons rasterised again.  ``import_local`` writes exactly that
result to ``<out>/train|val|test`` without the server in between: statistics, crops, the cell census of the rejection
rule (csrc/prepare.hip), contour tracing and polygon fill (csrc/polygons.hip, csrc/analysis.hip) run on the device.
DESIGN.md §6i states the rules, the reference quirks kept and the divergences.
"""
import contextlib
import json
import random
from pathlib import Path

import numpy as np
import torch

from .. import _lib
from .data_cropping import _stream, _to_device, _host, extract_crops_device, frame_stats_device, stats_from_sums
from .qt_shim import QObject, pyqtSignal, pyqtSlot, QCoreApplication

SUFFIXES = ['.png', '.tiff', '.tif', '.jpeg', '.jpg']


def imread(path):
    """.tif / .tiff through utils/tiffio, .png / .jpg through PIL when it is installed; FileNotFoundError if absent"""
    path = Path(path)
    if not path.is_file():
        raise FileNotFoundError(str(path))
    if path.suffix.lower() in ('.tif', '.tiff'):
        from . import tiffio
        return np.squeeze(tiffio.imread(str(path)))
    try:
        from PIL import Image
    except ImportError as err:
        raise RuntimeError(f"{path.name}: reading {path.suffix} files needs PIL, which is not installed") from err
    return np.squeeze(np.asarray(Image.open(str(path))))


def mask_path(img_id):
    """``img<rest>`` -> ``mask<rest>`` in the same folder (data_import.py:95)"""
    img_id = Path(img_id)
    return img_id.parent / "mask{}".format(img_id.name.split('img')[-1])


def centred_pads(shape, crop_size):
    """data_import.py:134-147: ``None`` if "too much pads" are needed, else ((top, bottom), (left, right)) of the zero
    padding that centres an image smaller than the crop (the odd pixel goes to the top / left)"""
    pads = [0, 0]
    if shape[0] < crop_size:
        pads[0] = crop_size - shape[0]
    if shape[1] < crop_size:
        pads[1] = crop_size - shape[1]
    if pads[0] > shape[0] or pads[1] > shape[1]:
        return None
    return (((pads[0] + 1) // 2, pads[0] // 2), ((pads[1] + 1) // 2, pads[1] // 2))


def import_grid(shape, crop_size):
    """data_import.py:151-164 for a (padded) image of ``shape``: ``None`` if the image is one crop as it is, else
    (num_crops_y, num_crops_x, y0, x0) — the grid and the rows / columns trimmed at the top / left.  The reference slices
    ``[floor(border):floor(-border)]`` with border = remainder / 2: an odd remainder loses one pixel more at the bottom /
    right, and what is left is exactly num_crops * crop_size."""
    h, w = int(shape[0]), int(shape[1])
    if not (h > crop_size or w > crop_size):
        return None
    ny, nx = h // crop_size, w // crop_size
    border_y = max(0, (h - ny * crop_size) / 2)
    border_x = max(0, (w - nx * crop_size) / 2)
    return ny, nx, int(np.floor(border_y)), int(np.floor(border_x))


def split_of(random_number, p_val, p_test):
    """data_import.py:188-194"""
    if random_number < p_test:
        return 'test'
    if random_number < p_test + p_val:
        return 'val'
    return 'train'


def accept_crop(num_cells_crop, area_crop, num_cells, area_cells):
    """data_import.py:177-179, short-circuit included (a region without cells never divides)"""
    return not (num_cells_crop == 0 or area_crop < area_cells / num_cells)


def crop_census_device(mask, np_dtype, y0, x0, ny, nx, crop_size):
    """device mask (H, W) -> (cells int [ny * nx + 1], area int [ny * nx + 1]), last slot = the whole grid region"""
    lib = _lib.load()
    dev = mask.device
    n = ny * nx + 1
    cells = torch.empty(n, dtype=torch.int32, device=dev)
    area = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.mseg_crop_census_workspace_bytes(), dtype=torch.uint8, device=dev)
    H, W = mask.shape
    _lib.check(lib.mseg_crop_census(mask.data_ptr(), 0 if np_dtype == np.uint8 else 1, H, W, int(y0), int(x0), int(ny),
                                    int(nx), int(crop_size), cells.data_ptr(), area.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _stream(dev)), "crop_census")
    return cells.cpu().numpy(), area.cpu().numpy()


def _label_mask(mask, name):
    """masks of other dtypes than uint8 / uint16 whose values fit are cast to uint16; larger (or negative) values raise"""
    if mask.dtype in (np.uint8, np.uint16):
        return mask
    if mask.min(initial=0) < 0 or mask.max(initial=0) > 65535 or not np.array_equal(mask, np.round(mask)):
        raise ValueError(f"{name}: mask values must be integers in 0 .. 65535")
    return mask.astype(np.uint16)


def round_trip_masks(mask_crops):
    """int16-storage mask crops (n, S, S) on the device -> (uint16 masks (n, S, S) as training receives them after the
    import -> export round trip, polygons per crop): the contour polygons of every id in id order (data_import.py:
    240-253), filled again with ids 1.. in that order, the last polygon winning, no relabelling (data_export.py:61-70)."""
    from .hull_polygon import label_polygons
    lib = _lib.load()
    dev = mask_crops.device
    n, S, _ = mask_crops.shape
    rc, lens, frames, first = [], [], [], []
    for k in range(n):
        first.append(len(lens))
        for polygons in label_polygons(mask_crops[k]).values():
            for polygon in polygons:
                rc.append(polygon.T.astype(np.int32))
                lens.append(polygon.shape[1])
                frames.append(k)
    counts = [(first[k + 1] if k + 1 < n else len(lens)) - first[k] for k in range(n)]
    if not lens:
        return np.zeros((n, S, S), np.uint16), counts
    voff = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=voff[1:])
    rc_d = torch.from_numpy(np.ascontiguousarray(np.concatenate(rc, 0))).to(dev)
    voff_d = torch.from_numpy(voff).to(dev)
    fr_d = torch.from_numpy(np.asarray(frames, np.int32)).to(dev)
    filled = torch.empty((n, S, S), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.mseg_roi_fill_workspace_bytes(len(lens))), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.mseg_roi_fill(rc_d.data_ptr(), voff_d.data_ptr(), fr_d.data_ptr(), len(lens), n, S, S,
                                 filled.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "roi_fill")
    # mseg_roi_fill numbers the polygons of the whole stack; the export starts at 1 in every image
    base = torch.tensor(first, dtype=torch.int32, device=dev).view(n, 1, 1)
    filled = torch.where(filled > 0, filled - base, filled)
    return filled.cpu().numpy().astype(np.uint16), counts


class DataImportWorker(QObject):
    """ Worker class for dataset import (reference data_import.py:17-286: same signals and slots).  ``import_data`` is the
    OMERO route and raises like ``AnalysisWorker.analyze_data``; ``import_local`` is the local route. """
    finished = pyqtSignal()  # Signal when import is finished
    text_output = pyqtSignal(str)  # Signal for possible exceptions, e.g., too small crops
    progress = pyqtSignal(int)  # Signal for updating the progress bar
    stop_import = False

    def import_data(self, img_ids, keep_normalization, crop_size, trainset_id, train_path, omero_username,
                    omero_password, omero_host, omero_port, group_id, p_train, p_val, p_test):
        """The reference uploads crops and ROIs to an OMERO server here (data_import.py:24-278): not part of this build."""
        raise RuntimeError("DataImportWorker.import_data needs the OMERO stack (omero-py), which is outside the MI355X "
                           "hot path; use DataImportWorker.import_local() or prepare_script.py import")

    def import_local(self, img_ids, keep_normalization, crop_size, out_path, p_train, p_val, p_test, rng=None,
                     raw_masks=False, text_output=print, device=None):
        """ Import annotated images (``img<name>`` with ``mask<name>`` beside it) into ``out_path/train|val|test`` as
        ``img_extNNN.tif`` / ``mask_extNNN.tif`` — what training receives after the reference's import -> export round
        trip — plus ``split_info.json`` (``num_ext`` continues across runs) and ``import_info.json`` (the key / value
        records of data_import.py:211-225).  ``raw_masks=True`` [extension] writes the mask crops as they are instead of
        their polygons' fill (the round trip erodes thin cells).  ``rng``: a ``random.Random``; one ``random()`` draw per
        image decides its set.  Returns the list of records written. """
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("No MI355X visible: the import runs on the device (there is no CPU path)")
            device = torch.device("cuda", torch.cuda.current_device())
        dev = torch.device(device)
        rng = rng if rng is not None else random.Random()
        out_path = Path(out_path)
        out_path.mkdir(parents=True, exist_ok=True)
        S = int(crop_size)
        say = text_output
        say('\nImporting data')

        split_info = {}
        if (out_path / 'split_info.json').is_file():
            with open(out_path / 'split_info.json', 'r') as infile:
                split_info = json.load(infile)
        if not split_info:
            split_info = {'used': [], 'num_ext': 0}
        if 'num_ext' not in split_info:
            split_info['num_ext'] = 0
        records = []

        from . import tiffio
        on_gpu = torch.cuda.device(dev) if dev.type == 'cuda' else contextlib.nullcontext()
        with on_gpu, torch.no_grad():
            for i, img_id in enumerate(img_ids):
                QCoreApplication.processEvents()
                if self.stop_import:
                    say("Stop data import due to user interaction.")
                    break
                img_id = Path(img_id)
                if img_id.suffix.lower() not in SUFFIXES:
                    continue
                img = imread(img_id)
                mask_id = mask_path(img_id)
                if mask_id.suffix.lower() not in SUFFIXES:
                    continue
                try:
                    mask = imread(mask_id)
                except FileNotFoundError:
                    say("  {}: No mask found (different file formats?)".format(img_id.name))
                    continue
                if np.max(mask) == 0:
                    say("  {}: empty mask --> skip".format(img_id.name))
                    continue
                if len(img.shape) == 3 and img.shape[-1] <= 3:
                    img = np.mean(img, axis=-1).astype(img.dtype)
                    say("  {}: rgb image converted to grayscale".format(img_id.name))
                if len(img.shape) >= 3:
                    say("  {}: 3D image --> skip".format(img_id.name))
                    continue
                if len(mask.shape) == 3 and mask.shape[-1] <= 3:
                    mask = np.mean(mask, axis=-1).astype(mask.dtype)
                    say("  {}: rgb mask converted to grayscale".format(img_id.name))
                if len(mask.shape) >= 3:
                    say("  {}: mask shape not supported --> skip".format(img_id.name))
                    continue
                if img.dtype.kind not in 'ui':
                    raise RuntimeError(f"{img_id.name}: {img.dtype} images are not supported (the reference's export "
                                       "parses the stored frame range as integers)")
                mask = _label_mask(mask, mask_id.name)
                on_device = img.dtype in (np.uint8, np.uint16)

                # frame information before cropping / padding
                if on_device:
                    img_dev = _to_device(img, dev)
                    vmin, vmax, s, q = frame_stats_device(img_dev)
                    mean_frame, std_frame = (np.float64(v) for v in stats_from_sums(vmin, vmax, s, q, img.size))
                    vmin, vmax = img.dtype.type(vmin), img.dtype.type(vmax)
                else:
                    vmin, vmax, mean_frame, std_frame = np.min(img), np.max(img), np.mean(img), np.std(img)
                if keep_normalization and np.issubdtype(img.dtype, np.unsignedinteger):
                    min_frame, max_frame = np.iinfo(img.dtype).min, np.iinfo(img.dtype).max
                else:
                    min_frame, max_frame = vmin, vmax
                if int(max_frame) == int(min_frame):
                    say("  {}: constant image --> skip".format(img_id.name))
                    continue

                pads = centred_pads(img.shape, S)
                if pads is None:
                    say("  {}: too much pads needed --> skip".format(img_id.name))
                    continue
                if pads != ((0, 0), (0, 0)):
                    img = np.pad(img, pads, mode='constant')
                    mask = np.pad(mask, pads, mode='constant')
                    if on_device:
                        img_dev = _to_device(img, dev)
                mask_dev = _to_device(mask, dev)

                grid = import_grid(img.shape, S)
                origins, offsets = [], []
                if grid is not None:
                    ny, nx, y0, x0 = grid
                    cells, area = crop_census_device(mask_dev, mask.dtype, y0, x0, ny, nx, S)
                    num_cells, area_cells = int(cells[-1]), int(area[-1])
                    for h in range(ny):
                        for w in range(nx):
                            if accept_crop(int(cells[h * nx + w]), int(area[h * nx + w]), num_cells, area_cells):
                                origins.append((y0 + h * S, x0 + w * S))
                                offsets.append((w * S + x0, h * S + y0))
                else:
                    origins.append((0, 0))
                    offsets.append((0, 0))

                import_set = split_of(rng.random(), p_val, p_test)
                if not origins:
                    continue

                if on_device:
                    img_crops = _host(extract_crops_device(img_dev, img.dtype, origins, S, 0, int(min_frame),
                                                           int(max_frame), want=("u16",))["u16"])
                else:
                    img_crops = np.stack([np.clip(65535 * (img[a:a + S, b:b + S].astype(np.float32) - int(min_frame))
                                                  / (int(max_frame) - int(min_frame)), 0, 65535).astype(np.uint16)
                                          for a, b in origins])
                mask_crops = extract_crops_device(mask_dev, mask.dtype, origins, S, 0, 0, 1, want=("raw",))["raw"]
                filled, counts = round_trip_masks(mask_crops.to(torch.int16))
                out_masks = _host(mask_crops) if raw_masks else filled

                (out_path / import_set).mkdir(parents=True, exist_ok=True)
                for k, (x_start, y_start) in enumerate(offsets):
                    num = split_info['num_ext']
                    split_info['num_ext'] += 1
                    self.progress.emit(int(100 * (i + 1) / len(img_ids)))
                    if counts[k] == 0:          # the export finds no ROI and skips the image (data_export.py:72-73)
                        say("img_ext{:03d}: no roi found --> skip".format(num))
                        continue
                    tiffio.imwrite(str(out_path / import_set / "img_ext{:03d}.tif".format(num)), img_crops[k])
                    tiffio.imwrite(str(out_path / import_set / "mask_ext{:03d}.tif".format(num)), out_masks[k])
                    records.append({"file": "img_ext{:03d}.tif".format(num),
                                    "crop_size": str(S), "set": import_set, "project": "imported_data",
                                    "dataset": img_id.parent.stem, "image": "ext_{}".format(img_id.name),
                                    "image_id": "imported", "frame": str(0), "channel": str(0),
                                    "pre_labeled": str(False), "x_start": str(x_start), "y_start": str(y_start),
                                    "min_frame": str(min_frame), "max_frame": str(max_frame),
                                    "mean_frame": str(mean_frame), "std_frame": str(std_frame)})

        with open(out_path / 'split_info.json', 'w', encoding='utf-8') as outfile:
            json.dump(split_info, outfile, ensure_ascii=False, indent=2)
        info = []
        if (out_path / 'import_info.json').is_file():
            with open(out_path / 'import_info.json', 'r') as infile:
                info = json.load(infile)
        with open(out_path / 'import_info.json', 'w', encoding='utf-8') as outfile:
            json.dump(info + records, outfile, ensure_ascii=False, indent=2)
        if not self.stop_import:
            self.progress.emit(100)
        self.finished.emit()
        return records

    @pyqtSlot()
    def stop_import_process(self):
        """ Set internal import stop state to True """
        self.stop_import = True
