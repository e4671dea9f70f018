""" The per-cell table of a segmented stack: shape, intensity in the image's channels, and overlap links between frames.

[extension] The reference stops at the per-frame means of its Analysis worker (src/inference/analysis.py:151-170); the
per-cell values behind those means are what people who follow single microbes need.  The integer sums come from the
device (csrc/cells.hip: ``mseg_cell_measure``, ``mseg_cell_links``), every float of the table is derived
from them here on the host in Python integers and fp64, so the table is exact where it can be and identical from run to
run.  ``assemble_tracks`` turns the links into track ids: this is OVERLAP linking — a cell follows the cell of the
previous frame it shares the most pixels with.  There is no motion model, and no gap closing unless ``gap`` is given: a
cell that moves further than its own extent between two frames, or that is missed in one frame, starts a new track.
``gap=G`` joins a cell that was missed in up to G consecutive frames to its track again: after the ordinary links, the cells
without predecessor look for a cell without successor 2 .. G + 1 frames back, under the motion summed over the gap
(``close_gaps``, ``mseg_cell_links_gap``).  ``drift=R`` takes the
usual cause of such jumps out first: the whole field of view moving by a few (tens of) pixels between time points.  The
integer shift of every frame pair is the peak of the device's foreground-overlap surface (csrc/drift.hip:
``mseg_stack_drift``), and the links are taken under it (``mseg_cell_links_shifted``).  ``flow=r`` goes on
from there for stacks whose cells move AGAINST EACH OTHER, as in a growing colony: every tile of every frame gets its own
whole-pixel shift, the peak of the tile's overlap surface within +-r pixels of the pair's drift (``mseg_stack_flow``;
DESIGN.md §6v), and the links are taken under that field (``mseg_cell_links_field``).  No sub-pixel or smoothed field, no
rotation, no per-cell search; gaps are closed by ``gap``, not by the field.  ``hull=True`` adds
the measures of the cell's PIXEL OUTLINE people take from rod-shaped microbes: crack perimeter, convex hull, largest and
smallest caliper (csrc/hull.hip: ``mseg_cell_hull``).  No sub-pixel contour is fitted.  ``midline=True`` adds the
length along a BENT cell, where the largest caliper is only the chord: every cell is thinned alone to a one-pixel skeleton
(Guo & Hall) and the skeleton is counted (csrc/midline.hip: ``mseg_cell_midline``).  Whole pixels: no
pruning, no sub-pixel midline; for straight rods the caliper stays the better length.  ``percentiles=(5, 50, 95)`` adds the
ROBUST intensity columns: percentiles (50 = the median) of every cell's pixel values and of every frame's background per
measured channel, where one hot pixel or a bright neighbour moves mean and max.  The device returns order statistics, the
exact integers of given ranks (csrc/order_stats.hip: ``mseg_cell_order_stats``); the linear interpolation
between two of them is numpy's, in fp64, here.  uint8 / uint16 images only, no other percentile method.  ``neighbors=R`` adds
every cell's NEIGHBOURHOOD within its frame: how many unit pixel edges it shares with other cells, with the frame's border
and with background, how many cells touch it, how many lie within R pixels, the nearest of them and the one it shares the
most edges with (csrc/neighbors.hip: ``mseg_cell_neighbors``); ``cell_contacts`` returns the contact graph
itself, one row per pair of cells within R.  Whole pixels only: distances are centre-to-centre distances of pixels, no
sub-pixel contour is fitted, nothing beyond R is seen, and this is no Voronoi or Delaunay neighbourhood.  ``spots=THR`` adds
every cell's fluorescent FOCI per measured channel: the local maxima of an exact integer band-pass of the image, D = 16^s
B_s(v) - B_2s(v) with binomial smoothings B_k (a difference of Gaussians, s = ``spot_scale``), whose response reaches THR
grey levels, counted under every cell and on the background (csrc/spots.hip: ``mseg_cell_spots``);
``cell_spots`` returns the spots themselves with their position along the cell's axes, which separates polar from mid-cell
foci.  Integers from the device, one division per float here.  Whole pixels and a fixed threshold: no sub-pixel positions,
no Gaussian fitting, no automatic or noise-relative threshold (the list carries the response: re-threshold afterwards), no
float images, no linking of spots over time.  ``profile=N`` adds WHERE ALONG THE CELL the signal sits, for signals that form
no foci: every cell's pixels are projected on its orientation, the projected extent is cut into N bins from pole to pole, and
the device returns every bin's pixel count and channel sums (csrc/profile.hip: ``mseg_cell_profile``); the
table gains the pole-to-pole extent, the pole / mid-cell ratio, the pole asymmetry and the position of the brightest bin,
``cell_profiles`` returns the profiles themselves, one row per cell, channel and bin.  Whole pixels, along the straight
orientation axis (a bent cell is folded onto its chord), no background subtraction, no normalisation across cells.
"""
import ctypes as C
import math
import types

import numpy as np
import pandas as pd
import torch

from .. import _lib

SHAPE_COLUMNS = ['frame', 'label', 'area', 'centroid_y', 'centroid_x', 'bbox_min_row', 'bbox_min_col', 'bbox_max_row',
                 'bbox_max_col', 'major_axis_length', 'minor_axis_length', 'orientation', 'touches_border']
CHANNEL_COLUMNS = ['mean_ch{c}', 'std_ch{c}', 'min_ch{c}', 'max_ch{c}', 'sum_ch{c}', 'bg_mean_ch{c}']
LINK_COLUMNS = ['pred_label', 'overlap', 'track_id', 'parent_track']
DRIFT_COLUMNS = ['drift_y', 'drift_x', 'centroid_y_reg', 'centroid_x_reg']
FLOW_COLUMNS = ['flow_y', 'flow_x']
HULL_COLUMNS = ['perimeter', 'convex_area', 'solidity', 'feret_max', 'feret_min', 'feret_angle', 'feret_y0', 'feret_x0',
                'feret_y1', 'feret_x1']
MIDLINE_COLUMNS = ['skeleton_pixels', 'skeleton_length', 'skeleton_ends', 'skeleton_branches', 'midline_length',
                   'midline_width', 'midline_y0', 'midline_x0', 'midline_y1', 'midline_x1']
PERCENTILE_COLUMNS = ['p{p}_ch{c}', 'bg_p{p}_ch{c}']     # all cell columns (channel by channel), then all background columns
MAX_PERCENTILES = 8   # 2 ranks each: the 16 ranks mseg_cell_order_stats accepts
MAX_DRIFT = 128       # largest search radius mseg_stack_drift accepts
MAX_FLOW = 32         # largest search radius mseg_stack_flow accepts
FLOW_TILES = (64, 128, 256)    # the tile sizes mseg_stack_flow and mseg_cell_links_field accept
GAP_COLUMNS = ['pred_gap']
MAX_GAP = 4           # most consecutive missed frames ``gap`` closes: mseg_cell_links_gap looks up to MAX_GAP + 1 frames back
NEIGHBOR_COLUMNS = ['contact_length', 'border_length', 'contact_fraction', 'n_touching', 'n_neighbors', 'nn_label',
                    'nn_distance', 'nn_gap', 'contact_label', 'contact_max']
CONTACT_COLUMNS = ['frame', 'label_a', 'label_b', 'contact', 'distance']
MIN_TABLE = 64        # smallest pair table mseg_cell_links and mseg_cell_neighbors accept
MAX_NEIGHBOR_RADIUS = 32   # largest radius mseg_cell_neighbors accepts
SPOT_COLUMNS = ['n_spots_ch{c}', 'spot_max_ch{c}', 'spot_sum_ch{c}', 'bg_spots_ch{c}']      # channel by channel
SPOT_TABLE_COLUMNS = ['frame', 'channel', 'label', 'y', 'x', 'value', 'response', 'axis_pos', 'axis_off']
MAX_SPOT_SCALE = 5    # largest scale mseg_cell_spots accepts
MAX_SPOT_THRESHOLD = 65535
PROFILE_COLUMNS = ['pole_mid_ratio_ch{c}', 'pole_asym_ch{c}', 'profile_peak_ch{c}']      # after axis_extent, channel by channel
PROFILE_TABLE_COLUMNS = ['frame', 'channel', 'label', 'bin', 'bin_pos', 'count', 'sum', 'mean']
MIN_PROFILE_BINS, MAX_PROFILE_BINS = 2, 32      # the bins mseg_cell_profile accepts
MAX_PROFILE_CHANNELS = 8    # most channels of one mseg_cell_profile call
PROFILE_UNIT = 16384        # the length of the integer direction (uy, ux) a profile is taken along
SPOT_RECORD = np.dtype([('frame', '<i4'), ('channel', '<i4'), ('y', '<i4'), ('x', '<i4'), ('label', '<i4'), ('value', '<i4'),
                        ('d', '<i8')])      # MsegSpot


def columns(channels=(), link=True, drift=False, hull=False, midline=False, percentiles=(), neighbors=False, spots=False,
            flow=False, gap=False, profile=False):
    """the table's columns, in order, for the measured ``channels``; ``drift``: with the drift columns (needs ``link``);
    ``flow``: with flow_y / flow_x after the drift columns (needs ``drift``); ``gap``: with pred_gap after the link, drift and
    flow columns (needs ``link``);
    ``hull``: with the outline columns; ``midline``: with the midline columns; ``percentiles``: with p{P}_ch{c} for every
    measured channel (per channel the percentiles in the order given), then bg_p{P}_ch{c} likewise; ``neighbors``: with the
    neighbourhood columns; ``spots``: with the four spot columns of every measured channel, channel by channel; ``profile``:
    with axis_extent and the three profile columns of every measured channel, channel by channel; these come last"""
    if drift and not link:
        raise ValueError("the drift columns belong to the link columns: drift needs link")
    if flow and not drift:
        raise ValueError("the flow columns follow the drift columns: flow needs drift")
    if gap and not link:
        raise ValueError("pred_gap belongs to the link columns: gap needs link")
    on = dict(link=link, drift=drift, flow=flow, gap=gap, hull=hull, midline=midline, percentiles=bool(percentiles),
              neighbors=neighbors, spots=spots, profile=profile)
    return [name for key, names, _ in _FAMILIES if on.get(key, True) for name in names(channels, percentiles)]


def channel_stems(percentiles=(), spots=False, profile=False):
    """the stems k of the table's per-channel columns k_ch{c}, for a caller that numbers the channels its own way
    (``InferWorker.cell_table``)"""
    names = CHANNEL_COLUMNS + [name.replace('{p}', str(int(q))) for q in percentiles for name in PERCENTILE_COLUMNS] + \
        (SPOT_COLUMNS if spots else []) + (PROFILE_COLUMNS if profile else [])
    return [name[:-len('_ch{c}')] for name in names]


def _need_channels(have, why, **families):
    """the refusal of the families that read an image (percentiles=, spots=, profiles= ..: on or off, in the order in which
    they refuse) where ``have``, the image or the channels to read, is missing"""
    for what, on in families.items():
        if on and not have:
            raise ValueError(f"{what.replace('_', ' ')} are taken of an image's channels: {why}")


def _device(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("No MI355X visible: the cell table is measured on the device (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _labels_to_device(mask, dev):
    """host array or device tensor -> (contiguous [T, H, W] device tensor: int16 holding uint16 bits, or int32; MSEG_PIX_*)"""
    if isinstance(mask, torch.Tensor):
        lab = mask if mask.dim() == 3 else mask[None]
        if lab.dtype not in (torch.int16, torch.int32):
            if lab.dtype in (torch.uint8, torch.int64, getattr(torch, "uint16", torch.int16)):
                lab = lab.to(torch.int32)
            else:
                raise ValueError(f"label tensors are int16 (uint16 bits), int32, uint8 or int64, got {lab.dtype}")
        lab = lab.to(dev).contiguous()
    else:
        m = np.asarray(mask)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.dtype.kind not in "iu":
            raise ValueError("mask: an integer [T, H, W] or [H, W] label array expected")
        if m.dtype == np.uint16:
            lab = torch.from_numpy(np.ascontiguousarray(m).view(np.int16)).to(dev)
        else:
            if m.min(initial=0) < 0 or m.max(initial=0) > 2 ** 31 - 1:
                raise ValueError("label values must lie in 0 .. 2^31 - 1")
            lab = torch.from_numpy(np.ascontiguousarray(m.astype(np.int32))).to(dev)
    return lab, (_lib.PIX_U16 if lab.dtype == torch.int16 else _lib.PIX_I32)


def _frame_counts(lab):
    """largest id of every frame = the size of its table"""
    T = lab.shape[0]
    k = np.zeros(T, np.int64)
    for t in range(T):                       # per frame: the widened copy of a uint16 frame stays one frame large
        f = lab[t]
        k[t] = int((f.to(torch.int32) & 0xFFFF).max()) if f.dtype == torch.int16 else max(int(f.max()), 0)
    return k


def _image_to_device(img, lab_shape, dev):
    """-> (device tensor that owns the memory, MSEG_PIX_*, n_channels, element strides (frame, channel, row, pixel)) of an
    image given as [T, C, H, W] or [T, H, W] ([H, W] for a single frame), with ANY strides: a view of an [H, W, 3] or
    [3, H, W] source is measured in place.  None for dtypes other than uint8 / uint16."""
    T, H, W = lab_shape
    if isinstance(img, torch.Tensor):
        if img.dtype not in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16)):
            return None
        t = img.to(dev)
        if t.dim() == 2:
            t = t[None]
        if t.dim() == 3:
            t = t[:, None]
        if tuple(t.shape[0:1] + t.shape[2:]) != (T, H, W):
            raise ValueError(f"image {tuple(t.shape)} does not match the label stack {(T, H, W)}")
        pix = _lib.PIX_U8 if t.dtype == torch.uint8 else _lib.PIX_U16
        return t, t.data_ptr(), pix, t.shape[1], tuple(int(s) for s in t.stride())
    a = np.asarray(img)
    if a.dtype not in (np.uint8, np.uint16):
        return None
    if a.ndim == 2:
        a = a[None]
    if a.ndim == 3:
        a = a[:, None]
    if a.ndim != 4 or (a.shape[0],) + a.shape[2:] != (T, H, W):
        raise ValueError(f"image {a.shape} does not match the label stack {(T, H, W)}")
    item = a.dtype.itemsize
    if any(s < 0 or s % item for s in a.strides):
        a = np.ascontiguousarray(a)
    strides = tuple(s // item for s in a.strides)
    span = 1 + sum((n - 1) * s for n, s in zip(a.shape, strides))
    flat = np.lib.stride_tricks.as_strided(a, shape=(span,), strides=(item,))   # the memory the view spans
    host = flat.view(np.int16) if a.dtype == np.uint16 else flat
    t = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    return t, t.data_ptr(), (_lib.PIX_U8 if a.dtype == np.uint8 else _lib.PIX_U16), a.shape[1], strides


def _channel_groups(channels):
    """channel indices -> runs (first, step, count) that one call covers with a single channel stride"""
    groups, i = [], 0
    while i < len(channels):
        if i + 1 == len(channels):
            groups.append((channels[i], 1, 1))
            break
        step, j = channels[i + 1] - channels[i], i + 1
        while j + 1 < len(channels) and channels[j + 1] - channels[j] == step:
            j += 1
        groups.append((channels[i], step, j - i + 1))
        i = j + 1
    return groups


def _offsets_to_device(off, dev):
    """the host table of label offsets [T + 1] as an int64 device tensor"""
    return torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(dev)


def _workspace(nbytes, dev, refused):
    """the device workspace a ``*_workspace_bytes`` call asked for; 0 bytes: the library takes no such arguments"""
    if nbytes == 0:
        raise ValueError(refused)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _channel_run(image, group):
    """the image arguments of a C call (address, MSEG_PIX_*, channels, frame / channel / row / pixel stride) for one run
    (first, step, count) of ``_channel_groups`` in the memory of an ``_image_to_device`` tuple"""
    _, base, ipix, _, (fs, cs0, rs, ps) = image
    first, step, count = group
    return base + first * cs0 * (1 if ipix == _lib.PIX_U8 else 2), ipix, count, fs, step * cs0, rs, ps


class _Stack:
    """What the entry points make of their arguments before the first device call: ``dev``; the labels on it, ``lab`` and
    ``pix`` (``_labels_to_device``), with ``T``, ``H``, ``W``; ``off``, the host table int64 [T + 1] of label offsets
    (``_frame_counts``); with an image, ``image``, the tuple of ``_image_to_device`` (uint8 / uint16 only), and ``channels``,
    the indices to measure as a list (default: all; each must exist); without one, None and []."""

    def __init__(self, mask, img=None, channels=None, device=None):
        self.dev = _device(device)
        with torch.cuda.device(self.dev):
            self.lab, self.pix = _labels_to_device(mask, self.dev)
            self.T, self.H, self.W = (int(v) for v in self.lab.shape)
            self.off = np.zeros(self.T + 1, np.int64)
            np.cumsum(_frame_counts(self.lab), out=self.off[1:])
            self.image, self.channels = None, []
            if img is not None:
                self.image = _image_to_device(img, (self.T, self.H, self.W), self.dev)
                if self.image is None:
                    raise ValueError("only uint8 / uint16 images are measured")
                self.channels = list(range(self.image[3])) if channels is None else [int(c) for c in channels]
                if any(c < 0 or c >= self.image[3] for c in self.channels):
                    raise ValueError(f"channels {self.channels} requested, the image has {self.image[3]}")


def _raw_args(lab, off, off_d=None):
    """what every ``*_raw`` opens with -> (lib, dev, T, H, W, n, off_d): the library, the device and the sizes of the labels,
    the number of label slots, and ``off`` on the device: uploaded here, once per call, unless the caller has it there"""
    T, H, W = (int(v) for v in lab.shape)
    return _lib.load(), lab.device, T, H, W, int(off[-1]), _offsets_to_device(off, lab.device) if off_d is None else off_d


def _with_status(items, dtype, dev, launch):
    """``items`` zeroed elements and the call's status word behind them in ONE device tensor, so that one download brings
    both: ``launch(address of the items, address of the status word)`` -> (the items on the host, the status word)"""
    out = torch.zeros(items + 1, dtype=dtype, device=dev)
    launch(out.data_ptr(), out.data_ptr() + items * out.element_size())
    host = out.cpu().numpy()
    return host[:-1], int(host[-1:].view(np.int32)[0])


def measure_raw(lab, pix, off, image=None, channels=()):
    """The integer sums of ``mseg_cell_measure`` as host arrays.  lab: device labels [T, H, W]; off: int64 [T + 1] host
    table; image: the tuple of ``_image_to_device``.  -> dict: shape uint64 [6, n], bbox int32 [n, 4], ch_sums uint64
    [2, C, n], ch_minmax uint32 [2, C, n], bg_sums uint64 [3, T, C], bg_minmax uint32 [2, T, C]"""
    lib, dev, T, H, W, n, off_d = _raw_args(lab, off)
    shape = torch.zeros((6, max(n, 1)), dtype=torch.int64, device=dev)
    bbox = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)
    out = {"ch_sums": [], "ch_minmax": [], "bg_sums": [], "bg_minmax": []}
    calls = _channel_groups(list(channels)) if image is not None and len(channels) else [None]
    for g in calls:
        img_args = (None, 0, 0, 0, 0, 0, 0) if g is None else _channel_run(image, g)
        Cg = img_args[2]
        chs = torch.zeros((2, max(Cg, 1), max(n, 1)), dtype=torch.int64, device=dev)
        chm = torch.zeros((2, max(Cg, 1), max(n, 1)), dtype=torch.int32, device=dev)
        bgs = torch.zeros((3, T, max(Cg, 1)), dtype=torch.int64, device=dev)
        bgm = torch.zeros((2, T, max(Cg, 1)), dtype=torch.int32, device=dev)
        _lib.check(lib.mseg_cell_measure(lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), n, *img_args,
                                         shape.data_ptr(), bbox.data_ptr(), chs.data_ptr(), chm.data_ptr(),
                                         bgs.data_ptr(), bgm.data_ptr(), _stream(dev)), "cell_measure")
        if Cg:
            out["ch_sums"].append(chs.cpu().numpy().view(np.uint64)[:, :, :n])
            out["ch_minmax"].append(chm.cpu().numpy().view(np.uint32)[:, :, :n])
            out["bg_sums"].append(bgs.cpu().numpy().view(np.uint64))
            out["bg_minmax"].append(bgm.cpu().numpy().view(np.uint32))
    res = {"shape": shape.cpu().numpy().view(np.uint64)[:, :n], "bbox": bbox.cpu().numpy()[:n]}
    empty = {"ch_sums": np.zeros((2, 0, n), np.uint64), "ch_minmax": np.zeros((2, 0, n), np.uint32),
             "bg_sums": np.zeros((3, T, 0), np.uint64), "bg_minmax": np.zeros((2, T, 0), np.uint32)}
    for key, parts in out.items():
        res[key] = np.concatenate(parts, axis=2 if key.startswith("bg") else 1) if parts else empty[key]
    return res


def hull_raw(lab, pix, off, bbox):
    """``mseg_cell_hull`` for the whole stack -> int64 [10, n] on the host: perimeter, hull_n, hull_area2, feret2, ay, ax, by,
    bx, minw_num, minw_den2 per cell slot, zeros for absent ids.  ``bbox``: int32 [n, 4], the boxes of ``measure_raw``; a
    cell with a pixel outside its box makes the device set its status word, which raises here."""
    n = int(off[-1])
    bbox = np.ascontiguousarray(bbox, np.int32).reshape(n, 4)
    row_off = np.zeros(n + 1, np.int64)        # corner rows of a present cell: r1 - r0 + 1; an absent one (r1 == 0) has none
    np.cumsum(np.where(bbox[:, 2] > bbox[:, 0], bbox[:, 2].astype(np.int64) - bbox[:, 0] + 1, 0), out=row_off[1:])
    n_rows = int(row_off[-1])
    if n == 0:
        return np.zeros((10, 0), np.int64)
    lib, dev, T, H, W, n, off_d = _raw_args(lab, off)
    bbox_d, row_d = torch.from_numpy(bbox).to(dev), torch.from_numpy(row_off).to(dev)
    ws = _workspace(lib.mseg_cell_hull_workspace_bytes(n, n_rows), dev,
                    f"mseg_cell_hull: no workspace for {n} cells with {n_rows} rows")
    ints, status = _with_status(10 * n, torch.int64, dev, lambda out, word: _lib.check(lib.mseg_cell_hull(
        lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), n, bbox_d.data_ptr(), row_d.data_ptr(), n_rows, out, word,
        ws.data_ptr(), ws.numel(), _stream(dev)), "cell_hull"))
    if status:
        raise RuntimeError("mseg_cell_hull: a cell has pixels outside the bounding box given for it")
    return ints.reshape(10, n)


def midline_raw(lab, pix, off, bbox, skeleton=False):
    """``mseg_cell_midline`` for the whole stack -> int64 [12, n] on the host: skel_n, n_orth, n_diag, n_end, n_branch, rounds,
    e0_y, e0_x, e0_d2, e1_y, e1_x, e1_d2 per cell slot, zeros for absent ids; with ``skeleton`` also the uint8 [T, H, W] image
    of all skeletons.  ``bbox``: int32 [n, 4], the boxes of ``measure_raw``.  A set status word raises."""
    n = int(off[-1])
    bbox = np.ascontiguousarray(bbox, np.int32).reshape(n, 4)
    b = bbox.astype(np.int64)
    word_off = np.zeros(n + 1, np.int64)       # bit rows of a present cell: the box and a ring of one pixel, rows of 64-bit words
    np.cumsum(np.where(b[:, 2] > b[:, 0], (b[:, 2] - b[:, 0] + 2) * ((b[:, 3] - b[:, 1] + 2 + 63) // 64), 0), out=word_off[1:])
    n_words = int(word_off[-1])
    if n == 0:
        ints = np.zeros((12, 0), np.int64)
        return (ints, np.zeros(tuple(lab.shape), np.uint8)) if skeleton else ints
    lib, dev, T, H, W, n, off_d = _raw_args(lab, off)
    skel = torch.empty((T, H, W), dtype=torch.uint8, device=dev) if skeleton else None
    bbox_d, word_d = torch.from_numpy(bbox).to(dev), torch.from_numpy(word_off).to(dev)
    ws = _workspace(lib.mseg_cell_midline_workspace_bytes(n, n_words), dev,
                    f"mseg_cell_midline: no workspace for {n} cells with {n_words} words")
    ints, status = _with_status(12 * n, torch.int64, dev, lambda out, word: _lib.check(lib.mseg_cell_midline(
        lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), n, bbox_d.data_ptr(), word_d.data_ptr(), n_words, out,
        skel.data_ptr() if skeleton else None, word, ws.data_ptr(), ws.numel(), _stream(dev)), "cell_midline"))
    if status & 1:
        raise RuntimeError("mseg_cell_midline: a cell has pixels outside the bounding box given for it")
    if status:
        raise RuntimeError("mseg_cell_midline: a cell was still being thinned at the round cap")
    ints = ints.reshape(12, n)
    return (ints, skel.cpu().numpy()) if skeleton else ints


def _whole(v, lo, hi, what, floats=True):
    """the one rule under the ``check_*`` functions: ``v`` as an int if it is a whole number in lo .. hi, else ValueError "``what``
    expected, got v".  Never a bool, a str or bytes; else what equals its ``int`` (3.0, a numpy integer; what ``int`` refuses does
    not), without ``floats`` integers only"""
    try:
        if not isinstance(v, (bool, str, bytes)) and (floats or isinstance(v, (int, np.integer))) and int(v) == v and \
                lo <= int(v) <= hi:
            return int(v)
    except (TypeError, ValueError, OverflowError):
        pass
    raise ValueError(f"{what} expected, got {v!r}")


def check_percentiles(p):
    """the rule of ``measure_cells(percentiles=...)``, ``InferWorker.percentiles`` and --percentiles: None or () = off;
    else 1 .. 8 distinct whole numbers in 0 .. 100 -> a tuple of ints in the order given"""
    if p is None:
        return ()
    try:
        vals = list(p)
    except TypeError:
        raise ValueError(f"percentiles: None or a sequence of whole numbers in 0 .. 100 expected, got {p!r}") from None
    out = []
    for v in vals:
        out.append(_whole(v, 0, 100, "percentiles: whole numbers in 0 .. 100"))
    if len(out) > MAX_PERCENTILES or len(set(out)) != len(out):
        raise ValueError(f"percentiles: at most {MAX_PERCENTILES} distinct values expected, got {out}")
    return tuple(out)


def percentile_ranks(count, percentiles):
    """The two order statistics numpy's linear rule reads for each percentile P of a sample of ``count`` values (an int or an
    integer array): h = (count - 1) * (P / 100) in fp64, k = floor(h) -> ranks k and min(k + 1, count - 1), g = h - k.
    -> (ranks int64 [2 * len(percentiles), *count.shape]: rows 2 i and 2 i + 1 belong to percentiles[i]; g fp64
    [len(percentiles), *count.shape]).  A count of 0 gives rank 0 (which nobody reads) and g 0.  Pure numpy."""
    n = np.asarray(count).astype(np.int64)
    ranks = np.zeros((2 * len(percentiles),) + n.shape, np.int64)
    g = np.zeros((len(percentiles),) + n.shape, np.float64)
    top = np.maximum(n - 1, 0)
    for i, q in enumerate(percentiles):
        h = top.astype(np.float64) * (np.float64(q) / np.float64(100))
        k = np.floor(h)
        ranks[2 * i] = np.minimum(k.astype(np.int64), top)
        ranks[2 * i + 1] = np.minimum(ranks[2 * i] + 1, top)
        g[i] = h - k
    return ranks, g


def percentile_value(lo, hi, g):
    """numpy's linear rule on the two order statistics: lo + (hi - lo) * g where g < 0.5, else hi - (hi - lo) * (1 - g); fp64"""
    lo, hi, g = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(g, np.float64)
    d = hi - lo
    return np.where(g < 0.5, lo + d * g, hi - d * (1.0 - g))


def order_stats_raw(lab, pix, off, image, channels, bbox, ranks, bg_ranks):
    """``mseg_cell_order_stats`` for the whole stack, one call per channel group -> (values uint32 [R, C, n], bg_values uint32
    [R, T, C]) on the host: per cell slot (frame) and channel the pixel value of rank ranks[j, s] (bg_ranks[j, t]) in ascending
    order.  ``bbox``: int32 [n, 4], the boxes of ``measure_raw``; ranks int64 [R, n], bg_ranks int64 [R, T].  A rank beyond a
    cell's pixels inside its box (or beyond a frame's background) makes the device set its status word, which raises here."""
    lib, dev, T, H, W, n, off_d = _raw_args(lab, off)
    ranks = np.ascontiguousarray(ranks, np.int64)
    bg_ranks = np.ascontiguousarray(bg_ranks, np.int64)
    R = int(bg_ranks.shape[0])
    _need_channels(image is not None and len(channels), "none given", order_statistics=True)
    if bg_ranks.shape != (R, T) or ranks.shape != (R, n):
        raise ValueError(f"ranks [{R}, {n}] and bg_ranks [{R}, {T}] expected, got {ranks.shape} and {bg_ranks.shape}")
    bbox_d = torch.from_numpy(np.ascontiguousarray(bbox, np.int32).reshape(n, 4)).to(dev) if n else None
    ranks_d = torch.from_numpy(ranks).to(dev) if n else None
    bg_ranks_d = torch.from_numpy(bg_ranks).to(dev)
    vals, bgs = [], []
    for group in _channel_groups(list(channels)):
        Cg = group[2]
        ws = _workspace(lib.mseg_cell_order_stats_workspace_bytes(T, n, Cg, R), dev,
                        f"mseg_cell_order_stats: no workspace for T = {T}, {Cg} channels, {R} ranks")
        host, status = _with_status(R * Cg * n + R * T * Cg, torch.int32, dev, lambda out, word: _lib.check(     # values, bg_values
            lib.mseg_cell_order_stats(lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), n, *_channel_run(image, group),
                                      bbox_d.data_ptr() if n else None, R, ranks_d.data_ptr() if n else None,
                                      bg_ranks_d.data_ptr(), out if n else None, out + 4 * R * Cg * n, word, ws.data_ptr(),
                                      ws.numel(), _stream(dev)), "cell_order_stats"))
        if status:
            raise RuntimeError("mseg_cell_order_stats: a rank lies beyond the pixels of a cell inside the bounding box given "
                               "for it (or beyond a frame's background)")
        host = host.view(np.uint32)
        vals.append(host[:R * Cg * n].reshape(R, Cg, n))
        bgs.append(host[R * Cg * n:].reshape(R, T, Cg))
    return np.concatenate(vals, axis=1), np.concatenate(bgs, axis=2)


def _pow2(v):
    return 1 << max(int(v) - 1, 0).bit_length()


def check_drift(drift):
    """the rule of ``measure_cells(drift=...)``, ``InferWorker.drift`` and --drift: None, or an int in 0 .. MAX_DRIFT"""
    return None if drift is None else _whole(drift, 0, MAX_DRIFT, f"drift: None or a whole number of pixels in 0 .. {MAX_DRIFT}")


def drift_raw(lab, pix, off, max_drift):
    """``mseg_stack_drift`` for the whole stack -> scores uint32 [T - 1, 2R + 1, 2R + 1] on the host: scores[t - 1, dy + R,
    dx + R] = pixels where the foreground of frame t - 1 moved by (dy, dx) lies on the foreground of frame t"""
    lib, dev, T, H, W, _, off_d = _raw_args(lab, off)
    R = int(max_drift)
    side = 2 * R + 1
    scores = torch.zeros((max(T - 1, 1), side, side), dtype=torch.int32, device=dev)
    ws = _workspace(lib.mseg_stack_drift_workspace_bytes(T, H, W), dev,
                    f"mseg_stack_drift: no workspace for a {T} x {H} x {W} stack")
    _lib.check(lib.mseg_stack_drift(lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), R, scores.data_ptr(), ws.data_ptr(),
                                    ws.numel(), _stream(dev)), "stack_drift")
    return scores.cpu().numpy().view(np.uint32)[:T - 1]


def pick_drift(scores):
    """scores uint32 [T - 1, 2R + 1, 2R + 1] -> int32 [T, 2] = (dy, dx) of every frame against its predecessor, row 0 =
    (0, 0).  The largest score wins; ties go to the smallest dy^2 + dx^2, then the smaller dy, then the smaller dx, so a
    shift that only ties the score at (0, 0) never wins; a pair whose best score is 0 gets (0, 0).  Pure numpy."""
    scores = np.asarray(scores)
    if scores.ndim != 3 or scores.shape[1] != scores.shape[2] or scores.shape[1] % 2 == 0:
        raise ValueError(f"scores: [T - 1, 2R + 1, 2R + 1] expected, got {scores.shape}")
    R = scores.shape[1] // 2
    d = np.arange(-R, R + 1, dtype=np.int64)
    dy, dx = (g.ravel() for g in np.meshgrid(d, d, indexing="ij"))
    norm = dy * dy + dx * dx
    shift = np.zeros((scores.shape[0] + 1, 2), np.int32)
    for t, surface in enumerate(scores, start=1):
        flat = surface.ravel().astype(np.int64)
        if flat.max() == 0:
            continue
        best = np.lexsort((dx, dy, norm, -flat))[0]            # the last key is the first criterion
        shift[t] = dy[best], dx[best]
    return shift


def check_flow(flow, tile=64):
    """the rule of ``measure_cells(flow=..., flow_tile=...)``, ``InferWorker.flow`` / ``flow_tile`` and --flow / --flow_tile:
    None, or an int in 0 .. MAX_FLOW, and a tile of FLOW_TILES -> (flow, tile)"""
    what = f"flow_tile: one of {', '.join(str(b) for b in FLOW_TILES)} pixels"
    if _whole(tile, min(FLOW_TILES), max(FLOW_TILES), what) not in FLOW_TILES:
        raise ValueError(f"{what} expected, got {tile!r}")
    return None if flow is None else _whole(flow, 0, MAX_FLOW, f"flow: None or a whole number of pixels in 0 .. {MAX_FLOW}"), \
        int(tile)


def flow_raw(lab, pix, off, base, radius, tile):
    """``mseg_stack_flow`` for the whole stack -> scores uint32 [T - 1, ty, tx, 2r + 1, 2r + 1] on the host: scores[t - 1, j,
    i, ey + r, ex + r] = pixels of tile (j, i) of frame t where the foreground of frame t - 1 moved by base[t] + (ey, ex)
    lies on the foreground of frame t.  ``base``: int32 [T, 2], row 0 unused"""
    lib, dev, T, H, W, _, off_d = _raw_args(lab, off)
    r, B = int(radius), int(tile)
    base = np.ascontiguousarray(base, np.int32)
    if base.shape != (T, 2):
        raise ValueError(f"base: int32 [{T}, 2] expected, got {base.shape}")
    ty, tx, side = -(-H // B), -(-W // B), 2 * r + 1
    base_d = torch.from_numpy(base).to(dev)
    scores = torch.zeros((max(T - 1, 1), ty, tx, side, side), dtype=torch.int32, device=dev)
    ws = _workspace(lib.mseg_stack_flow_workspace_bytes(T, H, W), dev,
                    f"mseg_stack_flow: no workspace for a {T} x {H} x {W} stack")
    _lib.check(lib.mseg_stack_flow(lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), B, r, base_d.data_ptr(),
                                   scores.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "stack_flow")
    return scores.cpu().numpy().view(np.uint32)[:T - 1]


def pick_flow(scores, base):
    """scores uint32 [T - 1, ty, tx, 2r + 1, 2r + 1], base int [T, 2] -> int32 [T, ty, tx, 2]: per tile base[t] + the
    deviation (ey, ex) ``pick_drift`` picks from the tile's surface (the largest score; ties to the smallest ey^2 + ex^2,
    then the smaller ey, then the smaller ex; (0, 0) where the best score is 0, so an empty tile falls back to the pair's
    drift).  Frame 0 holds zeros.  Pure numpy."""
    scores = np.asarray(scores)
    if scores.ndim != 5 or scores.shape[3] != scores.shape[4] or scores.shape[3] % 2 == 0:
        raise ValueError(f"scores: [T - 1, ty, tx, 2r + 1, 2r + 1] expected, got {scores.shape}")
    pairs, ty, tx, side = scores.shape[:4]
    base = np.asarray(base, np.int64)
    if base.shape != (pairs + 1, 2):
        raise ValueError(f"base: [{pairs + 1}, 2] expected, got {base.shape}")
    d = np.arange(-(side // 2), side // 2 + 1, dtype=np.int64)
    ey, ex = (g.ravel() for g in np.meshgrid(d, d, indexing="ij"))
    order = np.lexsort((ex, ey, ey * ey + ex * ex))                # the deviations from the most to the least preferred
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    # one key per (tile, deviation): the score first, then the preference; all-zero tiles end at rank 0 = (0, 0)
    field = np.zeros((pairs + 1, ty, tx, 2), np.int32)
    for t in range(1, pairs + 1):                                  # pair by pair: the keys of one pair at a time
        key = scores[t - 1].reshape(ty, tx, side * side).astype(np.int64) * order.size + (order.size - 1 - rank)
        best = key.argmax(axis=-1)
        field[t] = base[t] + np.stack([ey[best], ex[best]], axis=-1)
    return field


def _motion(lab, shift, field, tile):
    """the motion argument of ``link_raw`` / ``link_gap_raw``, checked against the stack -> int32 [T, 2] (``shift``), int32
    [T, ty, tx, 2] (``field``, which goes with ``tile``), or None: same (y, x)"""
    T, H, W = (int(v) for v in lab.shape)
    if (field is None) != (tile is None) or (field is not None and shift is not None):
        raise ValueError("field and tile go together, and not with shift")
    if field is not None:
        moved = np.ascontiguousarray(field, np.int32)
        if int(tile) not in FLOW_TILES or moved.shape != (T, -(-H // int(tile)), -(-W // int(tile)), 2):
            raise ValueError(f"field: int32 [{T}, ceil({H} / tile), ceil({W} / tile), 2] with a tile of {FLOW_TILES} expected, "
                             f"got {moved.shape} with tile {tile}")
        return moved
    if shift is None:
        return None
    moved = np.ascontiguousarray(shift, np.int32)
    if moved.shape != (T, 2):
        raise ValueError(f"shift: int32 [{T}, 2] expected, got {moved.shape}")
    return moved


def _links_call(lab, pix, off, cap, moved=None, tile=None, back=1, flags=None, off_d=None):
    """one launch of the links entry point the arguments ask for: ``mseg_cell_links``; with ``moved``: ``_shifted``; with ``tile``
    as well: ``_field``; with ``flags`` = (want, open): ``_gap``, ``back`` frames back -> (pred [n], overlap [n], status [T])"""
    lib, dev, T, H, W, n, off_d = _raw_args(lab, off, off_d)
    pred = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    ovl = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    status = torch.zeros(T, dtype=torch.int32, device=dev)
    moved_d = torch.from_numpy(np.ascontiguousarray(moved, np.int32)).to(dev) if moved is not None else None
    name, motion = "cell_links", ((moved_d.data_ptr(),) if moved is not None else ())
    if flags is not None:
        # want, then open, in one upload; the byte after them keeps the tensor (and both addresses) valid for a stack without cells
        flags_d = torch.from_numpy(np.concatenate([*flags, [False]]).astype(np.uint8)).to(dev)
        name, motion = "cell_links_gap", (int(back), int(tile) if tile is not None else 0, *(motion or (None,)),
                                          flags_d.data_ptr(), flags_d.data_ptr() + n)
    ws = _workspace(lib.mseg_cell_links_workspace_bytes(T, n, cap), dev,
                    f"mseg_{name}: no workspace for T = {T}, {n} cells, table {cap}")
    if flags is None and moved is not None:
        name, motion = ("cell_links_field", (int(tile),) + motion) if tile is not None else ("cell_links_shifted", motion)
    _lib.check(getattr(lib, "mseg_" + name)(lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), n, cap, *motion, pred.data_ptr(),
                                            ovl.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), name)
    return pred.cpu().numpy()[:n], ovl.cpu().numpy()[:n], status.cpu().numpy()


def _links(lab, pix, off, table_cap, moved, tile, back=1, flags=None, off_d=None):
    """The body of ``link_raw`` and ``link_gap_raw``: frame t against frame t - ``back`` (``flags`` = (want, open): flagged cells
    only) in one ``_links_call``, and the redo, alone on the frames t - back .. t, of every frame whose table filled up"""
    T, H, W = (int(v) for v in lab.shape)
    if table_cap is None:
        new = old = np.diff(off)
        if flags is not None:
            frame = np.repeat(np.arange(T), new)
            new, old = (np.bincount(frame[f], minlength=T) for f in flags)
        pair = int((new[back:] + old[:T - back]).max()) if T > back else 0
        table_cap = min(max(MIN_TABLE, _pow2(4 * pair)), _pow2(H * W + 1))
    pred, ovl, status = _links_call(lab, pix, off, int(table_cap), moved, tile, back, flags, off_d)
    pred, ovl = pred.copy(), ovl.copy()
    for t in np.nonzero(status)[0]:
        lo, hi = int(off[t - back]), int(off[t + 1])
        sub = off[t - back:t + 2] - lo
        p2, o2, s2 = _links_call(lab[t - back:t + 1], pix, sub, max(MIN_TABLE, _pow2(H * W + 1)),
                                 None if moved is None else moved[t - back:t + 1], tile, back,
                                 None if flags is None else tuple(f[lo:hi] for f in flags))
        if s2.any():
            raise RuntimeError(f"mseg_cell_links{'' if flags is None else '_gap'}: a table of more than H * W entries "
                               "reported full")
        pred[off[t]:off[t + 1]] = p2[sub[back]:]
        ovl[off[t]:off[t + 1]] = o2[sub[back]:]
    return pred, ovl


def link_raw(lab, pix, off, table_cap=None, shift=None, field=None, tile=None):
    """``mseg_cell_links`` for the whole stack -> (pred int32 [n], overlap int32 [n]) on the host.  The pair tables start
    at 4 entries per cell of the two frames; a frame pair whose table filled up (the device status word says so) is redone
    on its own with a table of more than H * W entries, which cannot fill up: the result is always exact.  ``shift``: int32
    [T, 2] = (dy, dx) per frame against its predecessor (row 0 unused): the links are taken under these shifts
    (``mseg_cell_links_shifted``); None: same (y, x), as ever.  ``field`` with ``tile``: int32 [T, ty, tx, 2], one (dy, dx)
    per ``tile`` x ``tile`` pixels of every frame (frame 0 unused): the links are taken under it (``mseg_cell_links_field``)."""
    return _links(lab, pix, np.asarray(off, np.int64), table_cap, _motion(lab, shift, field, tile), tile)


def check_gap(gap):
    """the rule of ``measure_cells(gap=...)``, ``InferWorker.gap`` and --gap: None, or an int in 1 .. MAX_GAP"""
    return None if gap is None else _whole(gap, 1, MAX_GAP, f"gap: None or a whole number of missed frames in 1 .. {MAX_GAP}",
                                           floats=False)


def compose_motion(moved, g):
    """The motion over g frames: out[t] = moved[t] + moved[t - 1] + ... + moved[t - g + 1] for t >= g, zeros below.
    ``moved``: the shifts of ``pick_drift`` [T, 2] or the field of ``pick_flow`` [T, ty, tx, 2] (entry 0 is never part of a
    sum).  A field is summed per tile index: the tile of frame t keeps its index through the gap, which is an approximation
    (the shifts are a few pixels, the tiles at least 64), not a composition through the displaced tile.  -> int32, pure numpy"""
    moved = np.asarray(moved)
    g = int(g)
    if moved.ndim not in (2, 4) or moved.shape[-1] != 2 or g < 1:
        raise ValueError(f"moved: [T, 2] or [T, ty, tx, 2] and g >= 1 expected, got {moved.shape} and {g}")
    total = np.cumsum(moved.astype(np.int64), axis=0)
    out = np.zeros(moved.shape, np.int32)
    out[g:] = total[g:] - total[:max(len(total) - g, 0)]
    return out


def link_gap_raw(lab, pix, off, g, want, open, shift=None, field=None, tile=None, table_cap=None, off_d=None):
    """``mseg_cell_links_gap`` for the whole stack -> (pred int32 [n], overlap int32 [n]) on the host: per cell of frame t
    flagged in ``want`` the cell of frame t - g flagged in ``open`` that shares the most pixels with it (ties to the smaller
    label), 0 for every other cell.  ``want``, ``open``: bool [n] in ``off`` order.  ``shift`` int32 [T, 2], or ``field`` int32
    [T, ty, tx, 2] with ``tile``: the motion of frame t against frame t - g, ALREADY composed (``compose_motion``); neither:
    same (y, x).  The pair tables start at 4 entries per flagged cell of the two frames; a frame whose table filled up (the
    device status word says so) is redone alone, on the g + 1 frames t - g .. t, with a table of more than H * W entries,
    which cannot fill up: the result is always exact.  ``off_d``: ``off`` on the device already (``close_gaps`` uploads it once
    for all its passes), or None."""
    g = int(g)
    off = np.asarray(off, np.int64)
    n = int(off[-1])
    moved = _motion(lab, shift, field, tile)
    if not 1 <= g <= MAX_GAP + 1:
        raise ValueError(f"g: 1 .. {MAX_GAP + 1} frames back expected, got {g}")
    want, open_ = np.asarray(want, bool), np.asarray(open, bool)
    if want.shape != (n,) or open_.shape != (n,):
        raise ValueError(f"want and open: bool [{n}] expected, got {want.shape} and {open_.shape}")
    return _links(lab, pix, off, table_cap, moved, tile, g, (want, open_), off_d)


def close_gaps(lab, pix, off, pred, overlap, min_overlap, G, shift=None, field=None, tile=None):
    """ Gap closing after the ordinary links -> (pred int32 [n], overlap int32 [n], pred_gap int32 [n]).

    ``pred``, ``overlap``: the links of ``link_raw``; a link counts as accepted when ``overlap >= min_overlap``.  An ORPHAN
    is a cell without accepted predecessor, an OPEN END a cell that no cell names as its accepted predecessor.  One pass per
    g = 2 .. G + 1, in that order: the orphans of the frames t >= g look among the open ends of frame t - g, pixel (y, x)
    against (y - Dy, x - Dx) with D the motion summed over the g frames (``compose_motion`` of ``shift``, or of ``field``
    with ``tile``; neither: 0); per orphan the open end sharing the most pixels wins, ties to the smaller label
    (``link_gap_raw``: one ``mseg_cell_links_gap`` call per pass); the link stands when its overlap is >= ``min_overlap``.
    Cells that continued take no part, on either side.  After a pass the linked orphans and their predecessors leave the
    sets; two orphans of one frame that found the same open end both keep it: a division across the gap.  The sets are
    O(cells) host work between the passes.  pred_gap: 0 where pred is 0, 1 for an ordinary link (one that ``min_overlap``
    rejects included, as pred / overlap keep it), g for a closed gap: pred then names a label of frame t - g.  A slot
    without pixels overlaps nothing, so it is flagged without effect."""
    off = np.asarray(off, np.int64)
    T, n = len(off) - 1, int(off[-1])
    pred, overlap = np.array(pred, np.int32), np.array(overlap, np.int32)
    frame = np.repeat(np.arange(T, dtype=np.int64), np.diff(off))
    pred_gap = (pred > 0).astype(np.int32)
    linked = (pred > 0) & (overlap >= int(min_overlap))
    orphan, open_ = ~linked, np.ones(n, bool)
    open_[off[frame[linked] - 1] + pred[linked] - 1] = False
    moved = field if field is not None else shift
    off_d = None                      # the offsets go up once, with the first pass that has something to look for
    for g in range(2, int(G) + 2):
        want = orphan & (frame >= g)
        if g >= T or not want.any() or not open_[:off[T - g]].any():
            continue
        over = compose_motion(moved, g) if moved is not None else None
        if off_d is None:
            off_d = _offsets_to_device(off, lab.device)
        p, o = link_gap_raw(lab, pix, off, g, want, open_, shift=over if field is None else None,
                            field=over if field is not None else None, tile=tile, off_d=off_d)
        hit = want & (p > 0) & (o >= int(min_overlap))
        pred[hit], overlap[hit], pred_gap[hit] = p[hit], o[hit], g
        orphan[hit] = False
        open_[off[frame[hit] - g] + p[hit] - 1] = False
    return pred, overlap, pred_gap


def check_neighbors(r):
    """the rule of ``measure_cells(neighbors=...)``, ``InferWorker.neighbors`` and --neighbors: None, or an int in 1 ..
    MAX_NEIGHBOR_RADIUS"""
    return None if r is None else _whole(r, 1, MAX_NEIGHBOR_RADIUS,
                                         f"neighbors: None or a whole number of pixels in 1 .. {MAX_NEIGHBOR_RADIUS}")


def _neighbors_call(lab, pix, off, radius, cap, pair_cap):
    """one ``mseg_cell_neighbors`` call with room for ``pair_cap`` rows, repeated with the exact count if there are more
    -> (ints int64 [9, n], pairs int32 [m, 5], status int32 [T])"""
    lib, dev, T, H, W, n, off_d = _raw_args(lab, off)
    ws = _workspace(lib.mseg_cell_neighbors_workspace_bytes(T, n, cap), dev,
                    f"mseg_cell_neighbors: no workspace for T = {T}, {n} cells, table {cap}")
    out = torch.zeros((9, max(n, 1)), dtype=torch.int64, device=dev)
    tail = torch.zeros(1 + (T + 1) // 2, dtype=torch.int64, device=dev)      # n_pairs, then the T status words: one download
    while True:
        rows = torch.zeros((max(pair_cap, 1), 5), dtype=torch.int32, device=dev)
        _lib.check(lib.mseg_cell_neighbors(lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), n, int(radius), int(cap),
                                           out.data_ptr(), rows.data_ptr(), int(pair_cap), tail.data_ptr(),
                                           tail.data_ptr() + 8, ws.data_ptr(), ws.numel(), _stream(dev)), "cell_neighbors")
        host = tail.cpu().numpy()
        m, status = int(host[0]), host[1:].view(np.int32)[:T].copy()
        if m <= pair_cap:
            return out.cpu().numpy()[:, :n], rows.cpu().numpy()[:m], status
        pair_cap = m


def neighbors_raw(lab, pix, off, radius, table_cap=None):
    """``mseg_cell_neighbors`` for the whole stack -> (ints int64 [9, n], pairs int32 [m, 5]) on the host: per cell slot
    contact_edges, border_edges, free_edges, n_touch, n_near, nn_label, nn_d2, contact_label, contact_label_edges, zeros for
    absent ids; per pair of cells of one frame within ``radius`` a row frame, a, b, edges, d2 with a < b, sorted by (frame, a,
    b).  The pair tables start at 8 entries per cell of the largest frame; a frame whose table filled up (the device status
    word says so) is redone on its own with the table doubled until it is clean, at most up to more than K (K - 1) / 2
    entries, which cannot fill up: the result is always exact."""
    T = int(lab.shape[0])
    n = int(off[-1])
    radius = check_neighbors(radius)
    if radius is None:
        raise ValueError("neighbors_raw: a radius is needed")
    if n == 0:
        return np.zeros((9, 0), np.int64), np.zeros((0, 5), np.int32)
    k = np.diff(np.asarray(off, np.int64))
    if table_cap is None:
        table_cap = max(MIN_TABLE, _pow2(8 * int(k.max())))
    ints, pairs, status = _neighbors_call(lab, pix, off, radius, int(table_cap), 8 * n)
    ints, parts = ints.copy(), [pairs[~np.isin(pairs[:, 0], np.nonzero(status)[0])]]
    for t in np.nonzero(status)[0]:
        kt = int(k[t])
        top = max(MIN_TABLE, _pow2(kt * (kt - 1) // 2 + 1))
        sub, cap = np.array([0, kt], np.int64), int(table_cap)
        while True:
            cap *= 2
            if cap > top:
                raise RuntimeError("mseg_cell_neighbors: a table of more than K (K - 1) / 2 entries reported full")
            i2, p2, s2 = _neighbors_call(lab[t:t + 1], pix, sub, radius, cap, 8 * kt)
            if not s2.any():
                break
        ints[:, off[t]:off[t + 1]] = i2
        p2 = p2.copy()
        p2[:, 0] = t
        parts.append(p2)
    pairs = np.concatenate(parts)
    return ints, pairs[np.lexsort((pairs[:, 2], pairs[:, 1], pairs[:, 0]))]


def cell_contacts(mask, radius=8, device=None):
    """ The contact graph of a segmented stack: one row per pair of cells of one frame that lie within ``radius`` pixels of
    each other, sorted by (frame, label_a, label_b), label_a < label_b.

    ``contact``: the unit pixel edges the two cells share (0: they do not touch, or only at a corner); ``distance``: the
    smallest distance between the centres of a pixel of the one and a pixel of the other (1 for cells that share an edge,
    sqrt(2) for a corner; distance - 1 is the gap).  From the device (``mseg_cell_neighbors``), through ``neighbors_raw``
    like ``measure_cells(neighbors=radius)``.  Whole pixels, centre-to-centre: no sub-pixel contour, no pairs beyond
    ``radius`` (1 .. 32), no Voronoi or Delaunay neighbourhood.
    :return: pandas.DataFrame with the columns CONTACT_COLUMNS.
    """
    radius = check_neighbors(radius)
    if radius is None:
        raise ValueError("cell_contacts: a radius in 1 .. 32 is needed")
    st = _Stack(mask, device=device)
    with torch.cuda.device(st.dev):
        pairs = neighbors_raw(st.lab, st.pix, st.off, radius)[1]
    return contacts_from_pairs(pairs)


def contacts_from_pairs(pairs):
    """the DataFrame of ``cell_contacts`` from the sorted pair rows of ``neighbors_raw``: distance = sqrt(d2), fp64"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 5)
    return pd.DataFrame({"frame": pairs[:, 0], "label_a": pairs[:, 1], "label_b": pairs[:, 2], "contact": pairs[:, 3],
                         "distance": np.sqrt(pairs[:, 4].astype(np.float64))}, columns=CONTACT_COLUMNS)


def check_spots(thr, scale=2):
    """the rule of ``measure_cells(spots=..., spot_scale=...)``, ``InferWorker.spots`` / ``spot_scale`` and --spots /
    --spot_scale: thr None = off -> None; else a whole number of grey levels in 1 .. 65535 and a whole scale in 1 .. 5 ->
    (thr, scale) as ints"""
    if thr is None:
        return None
    return _whole(thr, 1, MAX_SPOT_THRESHOLD, f"spots: None or a whole number in 1 .. {MAX_SPOT_THRESHOLD}"), \
        _whole(scale, 1, MAX_SPOT_SCALE, f"spot_scale: a whole number in 1 .. {MAX_SPOT_SCALE}")


def spot_bound(T, H, W, C=1):
    """the most spots T frames of H x W can have in C channels: two 8-adjacent pixels are never both spots"""
    return int(T) * int(C) * ((int(H) + 1) // 2) * ((int(W) + 1) // 2)


def spots_raw(lab, pix, off, image, channels, thr, scale, spot_cap=None):
    """``mseg_cell_spots`` for the whole stack, one call per channel group -> (cell_count int32 [C, n], bg_count int32 [T, C],
    records) on the host.  records: a SPOT_RECORD array, one entry per spot (frame, channel = the INDEX into ``channels``, y,
    x, label, value = the pixel's own value, d = D(p) in units of 16^(2 scale) per grey level), sorted by (frame, channel, y,
    x): the same bytes from run to run.  ``spot_cap``: room for so many spots per call (default: 4 per cell and 1024 per
    frame and channel); a list that overflowed (the device's status word says so) is never returned: the call is redone
    with room for the count the device reported, at most the worst case ``spot_bound``: the result is always complete."""
    _need_channels(image is not None and len(channels), "none given", spots=True)
    if check_spots(thr, scale) is None:
        raise ValueError("spots_raw: a threshold is needed")
    thr, scale = check_spots(thr, scale)
    lib, dev, T, H, W, n, off_d = _raw_args(lab, off)
    counts, bgs, recs, first_ci = [], [], [], 0
    for group in _channel_groups(list(channels)):
        Cg = group[2]
        ws = _workspace(lib.mseg_cell_spots_workspace_bytes(T, n, Cg), dev,
                        f"mseg_cell_spots: no workspace for T = {T}, {n} cells, {Cg} channels")
        top = spot_bound(T, H, W, Cg)
        cap = min(top, (4 * n + 1024 * T) * Cg) if spot_cap is None else max(int(spot_cap), 0)
        while True:
            tail = torch.zeros(2, dtype=torch.int64, device=dev)                      # n_spots, then the status word
            ints = torch.zeros(Cg * n + T * Cg, dtype=torch.int32, device=dev)       # cell_count, then bg_count
            lst = torch.zeros((max(cap, 1), 4), dtype=torch.int64, device=dev)       # 32 bytes per record
            _lib.check(lib.mseg_cell_spots(lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), n, *_channel_run(image, group),
                                           scale, thr, ints.data_ptr() if n else None, ints.data_ptr() + 4 * Cg * n,
                                           lst.data_ptr() if cap else None, cap, tail.data_ptr(), tail.data_ptr() + 8,
                                           ws.data_ptr(), ws.numel(), _stream(dev)), "cell_spots")
            end = tail.cpu().numpy()
            found, status = int(end[0]), int(end[1:].view(np.int32)[0])
            if found > top:
                raise RuntimeError(f"mseg_cell_spots: {found} spots reported, the frames can hold {top} at most")
            if found <= cap and not status:
                break
            cap = found
        host = ints.cpu().numpy()
        counts.append(host[:Cg * n].reshape(Cg, n).copy())
        bgs.append(host[Cg * n:Cg * n + T * Cg].reshape(T, Cg).copy())
        r = lst.cpu().numpy().reshape(-1).view(SPOT_RECORD)[:found].copy()
        r['channel'] += first_ci
        recs.append(r)
        first_ci += Cg
    records = np.concatenate(recs)
    return np.concatenate(counts, axis=0), np.concatenate(bgs, axis=1), \
        records[np.lexsort((records['x'], records['y'], records['channel'], records['frame']))]


def spot_axes(dy, dx, major, minor, orientation):
    """(axis_pos, axis_off) of an offset (dy, dx) from a cell's centroid: its projections on the cell's major axis, the
    direction (cos orientation, sin orientation) in (row, column), and on its minor axis, (-sin orientation, cos
    orientation), divided by half the major and half the minor axis length; fp64, arrays or scalars.  NaN where the axis
    length is 0.  The SIGN of axis_pos is arbitrary: a cell has no head.  The orientation is the table's own (``_axes``), with
    its special case: a cell whose row and column variances are EXACTLY equal gets +-pi/4 by scikit-image 0.18.3's rule, which
    for an exactly diagonal cell names the minor axis; axis_pos and axis_off then change places, as they would for anyone
    who projects on the table's ``orientation`` column."""
    dy, dx, o = np.asarray(dy, np.float64), np.asarray(dx, np.float64), np.asarray(orientation, np.float64)
    major, minor = np.asarray(major, np.float64), np.asarray(minor, np.float64)
    # the C library's cos / sin value by value: numpy's array loops may use other kernels for long arrays than for scalars
    co = np.array([math.cos(v) for v in o.ravel().tolist()], np.float64).reshape(o.shape)
    si = np.array([math.sin(v) for v in o.ravel().tolist()], np.float64).reshape(o.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        pos = np.where(major > 0, (dy * co + dx * si) / (0.5 * major), np.nan)
        offs = np.where(minor > 0, (dx * co - dy * si) / (0.5 * minor), np.nan)
    return pos, offs


def spots_from_records(records, scale, off, raw, channels, background=False):
    """the DataFrame of ``cell_spots`` from the sorted records of ``spots_raw`` and the integer sums of ``measure_raw``:
    response = d / 16^(2 scale) (int64 -> fp64 rounds to nearest and the division by a power of two is exact: the correctly
    rounded quotient of the two integers); axis_pos / axis_off from the centroid, the orientation and the axis lengths the
    table derives (``_axes``), NaN for label 0, for a label that is no cell of the frame, and for a zero axis"""
    off = np.asarray(off, np.int64)
    records = np.asarray(records, SPOT_RECORD)
    if not background:
        records = records[records['label'] != 0]
    t, label = records['frame'].astype(np.int64), records['label'].astype(np.int64)
    slot = off[t] + label - 1
    area = np.asarray(raw["shape"][0]).astype(np.int64)
    on_cell = (label >= 1) & (label <= off[t + 1] - off[t])
    on_cell[on_cell] = area[slot[on_cell]] > 0
    used, inverse = np.unique(slot[on_cell], return_inverse=True)
    geo = np.zeros((len(used), 5), np.float64)                   # centroid_y, centroid_x, major, minor, orientation
    for i, k in enumerate(used.tolist()):
        n, sy, sx, syy, sxx, sxy = (int(plane[k]) for plane in raw["shape"])
        geo[i] = (sy / n, sx / n) + _axes(n, sy, sx, syy, sxx, sxy)
    g = geo[inverse]
    pos, offs = np.full(len(records), np.nan), np.full(len(records), np.nan)
    pos[on_cell], offs[on_cell] = spot_axes(records['y'][on_cell] - g[:, 0], records['x'][on_cell] - g[:, 1], g[:, 2], g[:, 3],
                                            g[:, 4])
    names = np.asarray([int(c) for c in channels], np.int64)
    return pd.DataFrame({"frame": t, "channel": names[records['channel']], "label": label,
                         "y": records['y'].astype(np.int64), "x": records['x'].astype(np.int64),
                         "value": records['value'].astype(np.int64),
                         "response": records['d'].astype(np.float64) / float(1 << (8 * int(scale))), "axis_pos": pos,
                         "axis_off": offs}, columns=SPOT_TABLE_COLUMNS)


def cell_spots(mask, img, channels=None, spots=None, spot_scale=2, background=False, device=None):
    """ The fluorescent foci of a segmented stack: one row per spot, sorted by (frame, channel, y, x).

    A spot is a local maximum of the exact integer band-pass D = 16^s B_s(v) - B_2s(v) of a channel plane (a difference of
    Gaussians with sigma = sqrt(s / 2) and sqrt(s), s = ``spot_scale`` in 1 .. 5; csrc/spots.hip ``mseg_cell_spots``, DESIGN.md
    §6t) whose response D / 16^(2 s) reaches ``spots`` grey levels (1 .. 65535); it belongs to the label under it.
    ``value``: the pixel's own value; ``response``: in grey levels.  ``axis_pos`` / ``axis_off``: the spot's offset from its
    cell's centroid, projected on the cell's major / minor axis and divided by half the ``major_axis_length`` / half the
    ``minor_axis_length`` of the cell table: about +-1 at the poles, 0 at mid-cell.  NaN for label 0 and for a zero axis.  The
    SIGN of axis_pos is arbitrary, because a cell has no head: only |axis_pos| separates polar from mid-cell foci.
    ``channels``: indices into the channel axis of ``img`` (default: all); ``background=False`` drops the spots on label 0.
    Whole pixels: no sub-pixel positions, no Gaussian fit; a fixed threshold in grey levels, no automatic or noise-relative
    one (the list carries ``response``: re-threshold afterwards); uint8 / uint16 images only; spots are not linked over time.
    :return: pandas.DataFrame with the columns SPOT_TABLE_COLUMNS.
    """
    checked = check_spots(spots, spot_scale)
    if checked is None:
        raise ValueError("cell_spots: a threshold in 1 .. 65535 grey levels is needed")
    _need_channels(img is not None, "no image given", spots=True)
    st = _Stack(mask, img, channels, device)
    _need_channels(st.channels, "none is measured", spots=True)
    with torch.cuda.device(st.dev):
        raw = measure_raw(st.lab, st.pix, st.off)
        records = spots_raw(st.lab, st.pix, st.off, st.image, st.channels, *checked)[2]
    return spots_from_records(records, checked[1], st.off, raw, st.channels, background)


def _spot_sums(records, off, n_channels):
    """{(channel index, cell slot): (largest D, sum of D)} over the records on a cell of their frame.  The sums are exact:
    the two 32-bit halves of D are added apart in int64 and joined in Python integers"""
    off = np.asarray(off, np.int64)
    records = np.asarray(records, SPOT_RECORD)
    t, label, ci = records['frame'].astype(np.int64), records['label'].astype(np.int64), records['channel'].astype(np.int64)
    ok = (label >= 1) & (label <= off[t + 1] - off[t]) & (ci >= 0) & (ci < n_channels)
    n = int(off[-1])
    keys, inverse = np.unique(ci[ok] * n + off[t[ok]] + label[ok] - 1, return_inverse=True)
    d = records['d'][ok]
    top = np.full(len(keys), np.iinfo(np.int64).min, np.int64)
    lo, hi = np.zeros(len(keys), np.int64), np.zeros(len(keys), np.int64)
    np.maximum.at(top, inverse, d)
    np.add.at(lo, inverse, d & 0xFFFFFFFF)
    np.add.at(hi, inverse, d >> 32)                            # arithmetic shift: d == (d >> 32 << 32) + (d & 0xFFFFFFFF)
    return {(k // n, k % n): (m, (h << 32) + l) for k, m, l, h in zip(keys.tolist(), top.tolist(), lo.tolist(), hi.tolist())}


def check_profile(bins):
    """the rule of ``measure_cells(profile=...)``, ``InferWorker.profile`` and --profile: None = off -> None; else a whole
    number of bins in 2 .. 32 -> an int"""
    return None if bins is None else _whole(bins, MIN_PROFILE_BINS, MAX_PROFILE_BINS, "profile: None or a whole number of bins in "
                                            f"{MIN_PROFILE_BINS} .. {MAX_PROFILE_BINS}")


def profile_direction(orientation):
    """The integer direction (uy, ux) in (row, column) a profile is taken along, for the table's ``orientation`` o (``_axes``,
    the value ``spot_axes`` also projects on): uy = floor(16384 cos o + 0.5), ux = floor(16384 sin o + 0.5) -> int32 [n, 2].
    Bin 0 of a profile is the end with the SMALLER projection uy y + ux x, the sense in which the spots' axis_pos grows;
    the other sense would do as well, because a cell has no head.  The C library's cos / sin value by value, as in
    ``spot_axes``; the device only ever sees the integers.  Pure host code."""
    o = np.asarray(orientation, np.float64).reshape(-1)
    out = np.zeros((len(o), 2), np.int32)
    for i, v in enumerate(o.tolist()):
        out[i] = math.floor(PROFILE_UNIT * math.cos(v) + 0.5), math.floor(PROFILE_UNIT * math.sin(v) + 0.5)
    return out


def _orientations(raw):
    """the table's orientation (``_axes``) of every cell slot of ``measure_raw``'s sums -> (fp64 [n], present bool [n]); 0 for an
    absent id"""
    sh = [[int(v) for v in plane] for plane in raw["shape"]]
    o = np.zeros(len(sh[0]), np.float64)
    for s, n in enumerate(sh[0]):
        if n:
            o[s] = _axes(n, sh[1][s], sh[2][s], sh[3][s], sh[4][s], sh[5][s])[2]
    return o, np.asarray(sh[0], np.int64) > 0


def _cell_directions(raw):
    """``profile_direction`` of every cell slot's own orientation, (0, 0) for an absent id -> int32 [n, 2]"""
    o, present = _orientations(raw)
    dirs = profile_direction(o)
    dirs[~present] = 0
    return dirs


def profile_raw(lab, pix, off, image, channels, bbox, dirs, bins, area=None):
    """``mseg_cell_profile`` for the whole stack -> (count uint32 [N, n], sums uint64 [C, N, n], extent int64 [2, n]) on the
    host: per cell slot the pixels and the channel sums of each of the N = ``bins`` bins along ``dirs`` (int32 [n, 2] = uy, ux;
    ``profile_direction``), and the extreme projections qmin, qmax.  One call per channel run of ``_channel_groups`` and at
    most MAX_PROFILE_CHANNELS channels per call, one download per call.  ``bbox``: int32 [n, 4], the boxes of
    ``measure_raw``.  The call has no status word: a cell whose bins do not add up to its area has pixels outside the box
    given for it, which raises here.  ``area``: the areas ``measure_raw`` reported (raw["shape"][0]); None: they are measured
    here."""
    n = int(off[-1])
    N = check_profile(bins)
    if N is None:
        raise ValueError("profile_raw: a number of bins is needed")
    _need_channels(image is not None and len(channels), "none given", profiles=True)
    dirs = np.ascontiguousarray(dirs, np.int32)
    if dirs.shape != (n, 2):
        raise ValueError(f"dirs: int32 [{n}, 2] expected, got {dirs.shape}")
    runs = [(first + k * step, step, min(MAX_PROFILE_CHANNELS, cnt - k))
            for first, step, cnt in _channel_groups(list(channels)) for k in range(0, cnt, MAX_PROFILE_CHANNELS)]
    if n == 0:
        return np.zeros((N, 0), np.uint32), np.zeros((len(channels), N, 0), np.uint64), np.zeros((2, 0), np.int64)
    if area is None:
        area = measure_raw(lab, pix, off)["shape"][0]
    lib, dev, T, H, W, n, off_d = _raw_args(lab, off)
    bbox_d = torch.from_numpy(np.ascontiguousarray(bbox, np.int32).reshape(n, 4)).to(dev)
    dirs_d = torch.from_numpy(dirs).to(dev)
    count, extent, sums = None, None, []
    for run in runs:
        Cg = run[2]
        out = torch.empty(Cg * N * n + 2 * n + (N * n + 1) // 2, dtype=torch.int64, device=dev)   # sums, extent, count: one download
        s_ptr = out.data_ptr()
        e_ptr = s_ptr + 8 * Cg * N * n
        _lib.check(lib.mseg_cell_profile(lab.data_ptr(), pix, T, H, W, off_d.data_ptr(), n, *_channel_run(image, run),
                                         bbox_d.data_ptr(), dirs_d.data_ptr(), N, e_ptr + 16 * n, s_ptr, e_ptr, _stream(dev)),
                   "cell_profile")
        host = out.cpu().numpy()
        sums.append(host[:Cg * N * n].view(np.uint64).reshape(Cg, N, n))
        extent = host[Cg * N * n:Cg * N * n + 2 * n].reshape(2, n)
        count = host[Cg * N * n + 2 * n:].view(np.uint32)[:N * n].reshape(N, n)
        if not np.array_equal(count.sum(axis=0, dtype=np.int64), np.asarray(area).astype(np.int64)):
            raise RuntimeError("mseg_cell_profile: a cell has pixels outside the bounding box given for it")
    return count, np.concatenate(sums, axis=0), extent


def pole_bins(bins):
    """the POLE bins of a profile of N = ``bins`` bins, those whose centre lies in the outer quarters of the extent: 4 b + 2 < N
    (the end of bin 0) and 4 b + 2 > 3 N (the other end) -> (list, list); N = 2 and 3 have none"""
    N = int(bins)
    return [b for b in range(N) if 4 * b + 2 < N], [b for b in range(N) if 4 * b + 2 > 3 * N]


def profile_columns(count, sums):
    """(pole_mid_ratio, pole_asym, profile_peak) of one channel from the bin counts and bin sums (integers, sums < 2^53): count
    [N] and sums [N] of one cell -> three Python floats; count [N, n] and sums [N, n] of n cells -> three lists of n floats.
    pole_mid_ratio: the mean value of the pixels in the pole bins (``pole_bins``) over the mean of the pixels in the other
    bins; NaN when either group is empty (or both means are 0; inf over a mean of 0).  pole_asym: |A - B| / (A + B) with A, B
    the mean values of the pole bins at the two ends; NaN when an end is empty or A + B = 0.  profile_peak: the centre
    (2 b + 1) / N - 1 of the non-empty bin with the largest mean, ties to the smaller b, the means compared as the exact
    integers sum_i count_j against sum_j count_i; NaN without a pixel.  The group sums are numpy's (int64, exact), every
    quotient is one division of Python integers.  The peak starts from numpy's first largest fp64 mean: rounding is
    monotone, so the bin of the largest exact mean is among the bins that share the largest rounded one, and only cells
    where several bins share it are compared, in integers."""
    cnt, sm = np.asarray(count).astype(np.int64), np.asarray(sums).astype(np.int64)
    if cnt.ndim == 1:
        return tuple(col[0] for col in profile_columns(cnt[:, None], sm[:, None]))
    N, n = cnt.shape
    nan, inf = float("nan"), float("inf")
    lo, hi = pole_bins(N)
    ca, sa, cb, sb = cnt[lo].sum(axis=0), sm[lo].sum(axis=0), cnt[hi].sum(axis=0), sm[hi].sum(axis=0)
    cp, sp = ca + cb, sa + sb
    cm, smid = cnt.sum(axis=0) - cp, sm.sum(axis=0) - sp
    ratio = [nan if p == 0 or m == 0 or (u == 0 and v == 0) else ((v * m) / (p * u) if u else inf)
             for p, m, u, v in zip(cp.tolist(), cm.tolist(), smid.tolist(), sp.tolist())]
    asym = [abs(x * b - y * a) / (x * b + y * a) if a and b and x * b + y * a else nan
            for a, b, x, y in zip(ca.tolist(), cb.tolist(), sa.tolist(), sb.tolist())]
    mean = np.where(cnt > 0, sm / np.maximum(cnt, 1), -1.0)
    top, best = mean.max(axis=0, initial=-1.0), mean.argmax(axis=0)
    for s in np.flatnonzero(((mean == top).sum(axis=0) > 1) & (top >= 0)).tolist():
        k = -1
        for b in np.flatnonzero(mean[:, s] == top[s]).tolist():
            if k < 0 or int(sm[b, s]) * int(cnt[k, s]) > int(sm[k, s]) * int(cnt[b, s]):
                k = b
        best[s] = k
    peak = np.where(top >= 0, (2 * best + 1) / N - 1, np.nan)
    return ratio, asym, peak.tolist()


def axis_extent(qmin, qmax):
    """the pole-to-pole length of a cell's pixel set along its orientation, in pixels: (qmax - qmin) / 16384 + 1"""
    return (int(qmax) - int(qmin)) / PROFILE_UNIT + 1


def profiles_from_raw(off, area, channels, count, sums):
    """the DataFrame of ``cell_profiles`` from the integers of ``profile_raw``: one row per present cell, channel and bin,
    ordered by (frame, channel, label, bin); bin_pos = (2 b + 1) / N - 1, mean = sum / count, NaN for an empty bin"""
    off = np.asarray(off, np.int64)
    count, sums = np.asarray(count), np.asarray(sums)
    N, n = count.shape
    rows = {c: [] for c in PROFILE_TABLE_COLUMNS}
    pos = [(2 * b + 1) / N - 1 for b in range(N)]
    cnt = count.astype(np.int64).T.tolist()                       # [n][N]
    per_channel = [plane.T.tolist() for plane in sums]            # [C][n][N]
    for t in range(len(off) - 1):
        for ci, c in enumerate(channels):
            sm = per_channel[ci]
            for s in range(int(off[t]), int(off[t + 1])):
                if int(area[s]) == 0:
                    continue
                for b in range(N):
                    k, v = cnt[s][b], int(sm[s][b])
                    for name, val in zip(PROFILE_TABLE_COLUMNS, (t, int(c), s - int(off[t]) + 1, b, pos[b], k, v,
                                                                 v / k if k else float("nan"))):
                        rows[name].append(val)
    return pd.DataFrame(rows, columns=PROFILE_TABLE_COLUMNS)


def cell_profiles(mask, img, channels=None, bins=16, device=None):
    """ The intensity profiles of a segmented stack along every cell's axis: one row per cell, channel and bin, ordered by
    (frame, channel, label, bin).

    Every pixel (y, x) of a cell is projected on the cell's integer direction (uy, ux) = ``profile_direction`` of the table's
    ``orientation``: q = uy y + ux x; the bins divide the cell's own projected extent qmin .. qmax, from pole to pole of the
    pixel set, into ``bins`` (2 .. 32) equal parts: bin b = floor((q - qmin) bins / (qmax - qmin + 1)), exact (csrc/profile.hip
    ``mseg_cell_profile``).  ``count``: the pixels of the bin, ``sum``: the sum of the channel's values over
    them, ``mean`` = sum / count (NaN for an empty bin), ``bin_pos``: the bin's centre (2 b + 1) / bins - 1 in -1 .. 1.  Bin 0
    is the end with the smaller projection, the sense in which the spots' axis_pos grows; the sense is arbitrary, because a
    cell has no head.  ``channels``: indices into the channel axis of ``img`` (default: all).
    Whole pixels; the profile runs along the straight orientation axis, not along the midline: a strongly bent or
    filamentous cell is folded onto its chord; the bins divide the projected extent, not arc length; a bin thinner than a
    pixel row stays empty (count 0, mean NaN); no background subtraction, no normalisation across cells, no demograph
    image; uint8 / uint16 images only.
    :return: pandas.DataFrame with the columns PROFILE_TABLE_COLUMNS.
    """
    bins = check_profile(bins)
    if bins is None:
        raise ValueError("cell_profiles: a number of bins in 2 .. 32 is needed")
    _need_channels(img is not None, "no image given", profiles=True)
    st = _Stack(mask, img, channels, device)
    _need_channels(st.channels, "none is measured", profiles=True)
    with torch.cuda.device(st.dev):
        raw = measure_raw(st.lab, st.pix, st.off)
        count, sums, _ = profile_raw(st.lab, st.pix, st.off, st.image, st.channels, raw["bbox"], _cell_directions(raw), bins,
                                     raw["shape"][0])
    return profiles_from_raw(st.off, raw["shape"][0], st.channels, count, sums)


def assemble_tracks(frame, label, pred, overlap, min_overlap=1, gap=None):
    """ Track ids from overlap links; pure host code, O(cells).

    ``frame``, ``label``, ``pred``, ``overlap``: one entry per cell, in (frame, label) order; ``pred`` names a label of the
    previous frame (0 = none).  Links with ``overlap < min_overlap`` are dropped.  With n_succ(m) = the number of cells that
    name m: a cell whose predecessor has exactly one successor inherits its track_id and parent_track; a cell whose
    predecessor has two or more successors starts a new track whose parent_track is the predecessor's track (a division);
    a cell without predecessor starts a new track with parent_track 0.  Track ids count from 1 in order of first
    appearance.  A cell that loses a merge has no successor: its track ends.  ``gap``: per cell the number of frames back
    to its predecessor (``close_gaps``' pred_gap; entries of cells without one are not read), None: 1 everywhere.  The
    rules do not look at it: a predecessor with exactly one successor hands on its track whatever the gap.

    Overlap linking only: no motion model; gaps are closed before, by ``close_gaps``, not here.
    :return: (track_id int64 [n], parent_track int64 [n])
    """
    frame, label = np.asarray(frame, np.int64), np.asarray(label, np.int64)
    pred = np.where(np.asarray(overlap, np.int64) >= int(min_overlap), np.asarray(pred, np.int64), 0)
    back = np.ones(len(frame), np.int64) if gap is None else np.asarray(gap, np.int64)
    index = {(int(f), int(l)): i for i, (f, l) in enumerate(zip(frame, label))}
    src = np.full(len(frame), -1, np.int64)
    for i, (f, p, b) in enumerate(zip(frame, pred, back)):
        if p > 0:
            src[i] = index.get((int(f) - int(b), int(p)), -1)
    n_succ = np.bincount(src[src >= 0], minlength=len(frame))
    track, parent = np.zeros(len(frame), np.int64), np.zeros(len(frame), np.int64)
    nxt = 1
    for i in range(len(frame)):
        j = src[i]
        if j >= 0 and n_succ[j] == 1:
            track[i], parent[i] = track[j], parent[j]
            continue
        track[i], nxt = nxt, nxt + 1
        parent[i] = track[j] if j >= 0 else 0
    return track, parent


def _axes(n, sy, sx, syy, sxx, sxy):
    """(major, minor, orientation) of one cell from its exact sums: the formulas of rs_axes_kernel (csrc/analysis.hip) and
    the orientation of scikit-image 0.18.3 regionprops, whose inertia tensor is [[var_x, -cov], [-cov, var_y]]:
    0.5 * atan2(-2 b, c - a) with a = var_x, b = -cov, c = var_y, and +-pi/4 by the sign of b where a == c."""
    nn = float(n) * float(n)
    vy = float(n * syy - sy * sy) / nn
    vx = float(n * sxx - sx * sx) / nn
    cov = float(n * sxy - sx * sy) / nn
    h, q = 0.5 * (vy + vx), math.sqrt(0.25 * (vy - vx) * (vy - vx) + cov * cov)
    major, minor = 4.0 * math.sqrt(max(h + q, 0.0)), 4.0 * math.sqrt(max(h - q, 0.0))
    a, b, c = vx, -cov, vy
    if a - c == 0:
        orientation = -math.pi / 4.0 if b < 0 else math.pi / 4.0
    else:
        orientation = 0.5 * math.atan2(-2.0 * b, c - a)
    return major, minor, orientation


def _outline(area, h):
    """the outline columns of one cell from its area and the ten integers of ``mseg_cell_hull`` (HULL_COLUMNS order)"""
    per, _, area2, feret2, ay, ax, by, bx, num, den2 = h
    convex = area2 / 2
    return [per, convex, area / convex, math.sqrt(feret2), num / math.sqrt(den2), math.atan2(bx - ax, by - ay), ay, ax, by,
            bx]


def _midline(area, m):
    """the midline columns of one cell from its area and the twelve integers of ``mseg_cell_midline`` (MIDLINE_COLUMNS order)"""
    skel_n, n_orth, n_diag, n_end, n_branch, _, y0, x0, d0, y1, x1, d1 = m
    chain = n_orth + math.sqrt(2.0) * n_diag
    if (n_end == 2 and n_branch == 0) or skel_n == 1:
        length = chain + math.sqrt(d0) + math.sqrt(d1) - 1      # centre-to-centre at both ends -> centre-to-edge
    else:
        length = float("nan")                                   # a ring or a branched skeleton has no single midline
    return [skel_n, chain, n_end, n_branch, length, area / length, y0, x0, y1, x1]


def _neighborhood(v):
    """the neighbourhood columns of one cell from the nine integers of ``mseg_cell_neighbors`` (NEIGHBOR_COLUMNS order)"""
    contact, border, free, n_touch, n_near, nn_label, nn_d2, contact_label, contact_max = v
    dist = math.sqrt(nn_d2) if nn_label else float("nan")
    return [contact, border, contact / (contact + border + free), n_touch, n_near, nn_label, dist, dist - 1, contact_label,
            contact_max]


# ---- the column families ----------------------------------------------------------------------------------------------------
# A family is two functions.  ``names(channels, percentiles)``: its columns.  ``rows(tb)``: called once per table with the
# arguments of ``table_from_sums`` (and, as Python integers, ``tb.first``: the offsets, ``tb.slots`` = n, ``tb.sh``: raw["shape"]);
# it prepares what it can for all cells and returns ``row(t, s)`` -> the values of the cell in slot s of frame t, one per name.
# Python integers and one fp64 division or sqrt per value: n * sq - sv * sv passes int64.

def _planes(ints, count, slots):
    """the integers [count, n] of a ``*_raw`` call as Python integers, plane by plane"""
    return [[int(v) for v in plane] for plane in np.asarray(ints).reshape(count, slots)]


def _shape_rows(tb):
    """frame, label, area = n, the centroid sy / n, sx / n, the box of ``measure_raw``, the axes and the orientation of ``_axes``,
    and touches_border: the box reaches an edge of the H x W frame"""
    sh, first, H, W = tb.sh, tb.first, tb.H, tb.W
    boxes = np.asarray(tb.raw["bbox"]).tolist()
    def row(t, s):
        n = sh[0][s]
        major, minor, orientation = _axes(n, sh[1][s], sh[2][s], sh[3][s], sh[4][s], sh[5][s])
        r0, c0, r1, c1 = boxes[s]
        return [t, s - first[t] + 1, n, sh[1][s] / n, sh[2][s] / n, r0, c0, r1, c1, major, minor, orientation,
                bool(r0 == 0 or c0 == 0 or r1 == H or c1 == W)]
    return row


def _channel_rows(tb):
    """per measured channel, from the sums of ``measure_raw``: mean = sv / n, std = sqrt((n sq - sv^2) / n^2), min, max, sum
    = sv, and bg_mean, the mean over the frame's label-0 pixels (NaN for a frame without background)"""
    raw, sh, C = tb.raw, tb.sh, range(len(tb.channels))
    if not C:
        return lambda t, s: []
    sums, minmax, bg_sums = (np.asarray(raw[key]).tolist() for key in ("ch_sums", "ch_minmax", "bg_sums"))
    bg = [[bg_sums[1][t][ci] / bg_sums[0][t][ci] if bg_sums[0][t][ci] else float("nan") for ci in C]
          for t in range(len(tb.first) - 1)]
    def row(t, s):
        n, out = sh[0][s], []
        for ci in C:
            sv, sq = sums[0][ci][s], sums[1][ci][s]
            out += [sv / n, math.sqrt((n * sq - sv * sv) / (n * n)), minmax[0][ci][s], minmax[1][ci][s], sv, bg[t][ci]]
        return out
    return row


def _link_rows(tb):
    """``links`` = (pred, overlap): pred_label and overlap; track_id and parent_track are assembled over the whole table"""
    pred, overlap = ([int(v) for v in side] for side in tb.links)
    return lambda t, s: [pred[s], overlap[s], 0, 0]


def _drift_rows(tb):
    """``shift``: int [T, 2], the (dy, dx) of every frame against its predecessor the links were taken under (row 0 ignored):
    drift_y / drift_x, the shifts summed up to the frame, and centroid_y_reg / centroid_x_reg, the centroid minus them"""
    sh = tb.sh
    shift = np.asarray(tb.shift, np.int64).reshape(len(tb.first) - 1, 2).copy()
    shift[0] = 0
    total = [(int(a), int(b)) for a, b in np.cumsum(shift, axis=0)]      # against frame 0
    def row(t, s):
        (dy, dx), n = total[t], sh[0][s]
        return [dy, dx, sh[1][s] / n - dy, sh[2][s] / n - dx]
    return row


def _flow_rows(tb):
    """``field`` with ``tile``: int [T, ty, tx, 2], the field of ``pick_flow`` the links were taken under: flow_y / flow_x, the
    field value of the tile that holds the pixel (floor(centroid_y), floor(centroid_x)), 0 in frame 0"""
    sh, tile = tb.sh, int(tb.tile)
    field = np.asarray(tb.field, np.int64).copy()
    field[0] = 0
    field = field.tolist()
    return lambda t, s: field[t][sh[1][s] // sh[0][s] // tile][sh[2][s] // sh[0][s] // tile]


def _gap_rows(tb):
    """``gaps``: int [n], the pred_gap of ``close_gaps`` (with its pred and overlap as ``links``): pred_gap; the tracks are
    assembled over the gaps"""
    gaps = [int(v) for v in tb.gaps]
    return lambda t, s: [gaps[s]]


def _hull_rows(tb):
    """``hull``: int [10, n], the integers of ``hull_raw``: perimeter (exposed pixel edges), convex_area = hull_area2 / 2,
    solidity = area / convex_area, feret_max = sqrt(feret2), feret_min = num / sqrt(den2), feret_angle = atan2(bx - ax, by -
    ay) in (-pi/2, pi/2] from the row axis, and the chord's end points (``_outline``)"""
    sh, hl = tb.sh, _planes(tb.hull, 10, tb.slots)
    return lambda t, s: _outline(sh[0][s], [plane[s] for plane in hl])


def _midline_rows(tb):
    """``midline``: int [12, n], the integers of ``midline_raw``: skeleton_pixels = skel_n, skeleton_length = n_orth + sqrt(2)
    n_diag, skeleton_ends, skeleton_branches, midline_length = skeleton_length + sqrt(e0_d2) + sqrt(e1_d2) - 1 where the
    skeleton is one open chain (n_end == 2 and n_branch == 0) or one pixel, NaN otherwise, midline_width = area /
    midline_length, and the two end points, 0 where there are none (``_midline``)"""
    sh, ml = tb.sh, _planes(tb.midline, 12, tb.slots)
    return lambda t, s: _midline(sh[0][s], [plane[s] for plane in ml])


def _percentile_rows(tb):
    """``order_stats``: (percentiles, values uint32 [2 P, C, n], bg_values uint32 [2 P, T, C]): the integers of
    ``order_stats_raw`` for the ranks of ``percentile_ranks`` (cell counts: raw["shape"][0], background counts:
    raw["bg_sums"][0]): p{P}_ch{c} = ``percentile_value`` of the two order statistics, and bg_p{P}_ch{c} (NaN without
    background)"""
    pct, C, T = tb.pct, len(tb.channels), len(tb.first) - 1
    values = np.asarray(tb.order_stats[1]).reshape(2 * len(pct), C, tb.slots)
    bg_values = np.asarray(tb.order_stats[2]).reshape(2 * len(pct), T, C)
    bg_n = np.asarray(tb.raw["bg_sums"][0]).astype(np.int64)                                 # [T, C]
    g = percentile_ranks(np.asarray(tb.raw["shape"][0]).astype(np.int64), pct)[1]             # [P, n]
    cell_p = percentile_value(values[0::2], values[1::2], g[:, None, :]).tolist()             # [P, C, n], Python floats
    bg_p = np.where(bg_n[None] > 0, percentile_value(bg_values[0::2], bg_values[1::2], percentile_ranks(bg_n, pct)[1]),
                    np.nan).tolist()
    order = [(i, ci) for ci in range(C) for i in range(len(pct))]
    return lambda t, s: [cell_p[i][ci][s] for i, ci in order] + [bg_p[i][t][ci] for i, ci in order]


def _neighbor_rows(tb):
    """``neighbors``: int [9, n], the integers of ``neighbors_raw``: contact_length = contact_edges, border_length =
    border_edges, contact_fraction = contact_edges / (contact_edges + border_edges + free_edges), n_touching = n_touch,
    n_neighbors = n_near, nn_label, nn_distance = sqrt(nn_d2) and nn_gap = nn_distance - 1 (both NaN where no cell lies within
    the radius, nn_label then 0), contact_label and contact_max = contact_label_edges (both 0 where no cell shares an edge)
    (``_neighborhood``)"""
    nbl = _planes(tb.neighbors, 9, tb.slots)
    return lambda t, s: _neighborhood([plane[s] for plane in nbl])


def _spot_rows(tb):
    """``spots``: (scale, cell_count int32 [C, n], bg_count int32 [T, C], records), the scale and the three results of
    ``spots_raw``: per measured channel n_spots_ch{c} = cell_count, spot_max_ch{c} = the largest D among the cell's records /
    16^(2 scale) (NaN without a spot), spot_sum_ch{c} = the exact integer sum of their D / 16^(2 scale) (0 without),
    bg_spots_ch{c} = bg_count of the frame"""
    scale, cell_count, bg_count, records = tb.spots
    C, unit = range(len(tb.channels)), 1 << (8 * int(scale))
    count = np.asarray(cell_count).reshape(len(C), tb.slots).tolist()
    bg = np.asarray(bg_count).reshape(len(tb.first) - 1, len(C)).tolist()
    found = _spot_sums(records, tb.first, len(C))
    def row(t, s):
        out = []
        for ci in C:
            top, d_sum = found.get((ci, s), (None, 0))
            out += [count[ci][s], top / unit if top is not None else float("nan"), d_sum / unit, bg[t][ci]]
        return out
    return row


def _profile_rows(tb):
    """``profile``: (count [N, n], sums [C, N, n], extent [2, n]), the integers of ``profile_raw``: axis_extent = ``axis_extent``
    of the cell's extreme projections and, per measured channel, pole_mid_ratio_ch{c}, pole_asym_ch{c} and profile_peak_ch{c}
    = ``profile_columns`` of the cell's bins"""
    count, sums, extent = tb.profile
    q = np.asarray(extent).astype(np.int64).reshape(2, tb.slots)
    length = ((q[1] - q[0]) / PROFILE_UNIT + 1).tolist()                                     # ``axis_extent``, all cells at once
    bins = np.asarray(count).shape[0]                             # N: a stack without a cell still has its bins
    per_channel = [profile_columns(count, plane)                                              # [C][3][n]
                   for plane in np.asarray(sums).reshape(len(tb.channels), bins, tb.slots)]
    return lambda t, s: [length[s]] + [col[s] for cols in per_channel for col in cols]


def _per_channel(stencil):
    return lambda channels, pct: [name.format(c=int(c)) for c in channels for name in stencil]


_FAMILIES = (          # (the switch of ``columns``, names, rows) in the order of the table's columns
    (None, lambda channels, pct: SHAPE_COLUMNS, _shape_rows),
    (None, _per_channel(CHANNEL_COLUMNS), _channel_rows),
    ("link", lambda channels, pct: LINK_COLUMNS, _link_rows),
    ("drift", lambda channels, pct: DRIFT_COLUMNS, _drift_rows),
    ("flow", lambda channels, pct: FLOW_COLUMNS, _flow_rows),
    ("gap", lambda channels, pct: GAP_COLUMNS, _gap_rows),
    ("hull", lambda channels, pct: HULL_COLUMNS, _hull_rows),
    ("midline", lambda channels, pct: MIDLINE_COLUMNS, _midline_rows),
    ("percentiles", lambda channels, pct: [name.format(p=int(q), c=int(c)) for name in PERCENTILE_COLUMNS for c in channels
                                           for q in pct], _percentile_rows),
    ("neighbors", lambda channels, pct: NEIGHBOR_COLUMNS, _neighbor_rows),
    ("spots", _per_channel(SPOT_COLUMNS), _spot_rows),
    ("profile", lambda channels, pct: ['axis_extent'] + _per_channel(PROFILE_COLUMNS)(channels, pct), _profile_rows),
)


def table_from_sums(off, H, W, raw, channels=(), links=None, min_overlap=1, shift=None, hull=None, midline=None,
                    order_stats=None, neighbors=None, spots=None, field=None, tile=None, gaps=None, profile=None):
    """the DataFrame from the integer sums of ``measure_raw`` (and ``links`` = (pred, overlap) or None); host arithmetic in
    Python integers and fp64.  Every further argument is the integers of one column family, or None for a table without it;
    what it holds and what becomes of it stands with the family (``_drift_rows`` for ``shift``, ``_flow_rows`` for ``field``
    with ``tile``, which needs ``shift``, ``_gap_rows`` for ``gaps``, ``_hull_rows``, ``_midline_rows``, ``_percentile_rows`` for
    ``order_stats``, ``_neighbor_rows``, ``_spot_rows``, ``_profile_rows``).  The columns are those of ``columns`` in its order,
    whichever families are given; a row that does not bring exactly one value per column raises."""
    if field is not None and shift is None:
        raise ValueError("the flow columns follow the drift columns: field needs shift")
    pct = check_percentiles(order_stats[0]) if order_stats is not None else ()
    _need_channels(len(channels), "none is measured", percentiles=pct, spots=spots is not None, profiles=profile is not None)
    given = dict(link=links is not None, drift=shift is not None, hull=hull is not None, midline=midline is not None,
                 percentiles=pct, neighbors=neighbors is not None, spots=spots is not None, flow=field is not None,
                 gap=gaps is not None, profile=profile is not None)
    cols = columns(channels, **given)
    area = raw["shape"][0]
    first, slots, sh = [int(v) for v in off], len(area), _planes(raw["shape"], 6, len(area))
    tb = types.SimpleNamespace(**locals())      # the arguments, pct, first, slots and sh: what the families read
    families = [rows(tb) for key, _, rows in _FAMILIES if given.get(key, True)]
    lists = [[] for _ in cols]
    for t in range(len(first) - 1):
        for s in range(first[t], first[t + 1]):
            if sh[0][s] == 0:
                continue
            vals = []
            for row in families:
                vals += row(t, s)
            if len(vals) != len(cols):
                raise RuntimeError(f"cell table: {len(vals)} values for the {len(cols)} columns of the cell in slot {s}")
            for column, v in zip(lists, vals):
                column.append(v)
    df = pd.DataFrame(dict(zip(cols, lists)), columns=cols)
    assert int((area > 0).sum()) == len(df)
    if links is not None:
        df["track_id"], df["parent_track"] = assemble_tracks(df["frame"], df["label"], df["pred_label"], df["overlap"],
                                                             min_overlap, df["pred_gap"] if gaps is not None else None)
    return df


def measure_cells(mask, img=None, channels=None, link=True, min_overlap=1, device=None, drift=None, hull=False,
                  midline=False, percentiles=None, neighbors=None, spots=None, spot_scale=2, flow=None, flow_tile=64,
                  gap=None, profile=None):
    """ One row per cell of a segmented stack, ordered by (frame, label).

    :param mask: label stack [T, H, W] (or one frame [H, W]): host array or device tensor (int16 holding uint16 bits, or
        int32); 0 is background, a frame's cells are its ids 1 .. max.
    :param img: intensity image, uint8 / uint16, as [T, C, H, W], [T, H, W] or [H, W] with any strides (host array or
        device tensor; read in place), or None for the shape and link columns only.
    :param channels: indices into the channel axis of ``img`` to measure (default: all); they name the columns.
    :param link: add pred_label / overlap (the label of the previous frame sharing the most pixels, ties to the smaller
        label, 0 = none) and track_id / parent_track (``assemble_tracks``).  Overlap linking: no motion model, and no gap
        closing unless ``gap`` is given.
    :param min_overlap: links with fewer shared pixels are dropped before the tracks are assembled.
    :param drift: None (default): link at the same (y, x).  R, a whole number in 0 .. 128: take the stage drift out first.
        Every frame pair gets the integer shift (|dy|, |dx| <= R) under which the foregrounds of the two frames share the
        most pixels (``pick_drift``), the links are taken under it, and the table ends with drift_y / drift_x (the shift of
        the frame against frame 0, the same for all its rows) and centroid_y_reg / centroid_x_reg (the centroid minus that
        shift: a cell that only drifted keeps it).  Whole pixels, translation only; needs ``link``.
    :param flow: None (default): one shift per frame pair.  r, a whole number in 0 .. 32: link under a TILE-WISE displacement
        field, for cells that move against each other (a colony that expands from its centre).  Every ``flow_tile`` x
        ``flow_tile`` tile of frame t gets the shift within +-r pixels of the pair's drift under which the tile's foreground
        lies on most foreground of frame t - 1 (``pick_flow``; an empty tile keeps the drift), the links are taken under
        that field, and flow_y / flow_x follow the drift columns: the field value of the tile that holds the cell's
        centroid pixel, i.e. the cell's estimated motion against the previous frame, stage drift included (0 in frame 0).
        drift_y / drift_x and the registered centroids stay the global ones.  Whole pixels, one shift per tile: no
        smoothing or interpolation of the field, no rotation, no per-cell search; gaps are ``gap``'s.  Needs ``drift``.
    :param flow_tile: 64 (default), 128 or 256: the tile edge in pixels.  Small tiles follow a steep field, large tiles
        hold more cells to vote.  Read only with ``flow``.
    :param gap: None (default): a cell that is missed in one frame starts a new track.  G, a whole number in 1 .. 4: close
        gaps of up to G consecutive missed frames (``close_gaps``).  After the ordinary links, every cell without an
        accepted predecessor looks 2, then 3, .. G + 1 frames back among the cells that nothing followed, at the same
        (y, x) or, with ``drift`` / ``flow``, under the shifts summed over the gap (for a field per tile index: an
        approximation); the cell sharing the most pixels wins when it shares at least ``min_overlap``.  pred_label then
        names a label of frame ``frame - pred_gap``, overlap is the overlap under the summed motion, and the new column
        pred_gap (0 without predecessor, 1 for an ordinary link, g for a closed gap) follows the link, drift and flow
        columns.  The track goes on across the gap; two cells that find the same ended cell are a division.  No motion
        model, no per-cell search, no rows for the missed frames, no check that the skipped frames are empty under the
        cell.  Needs ``link``.
    :param hull: True: the table ends with the measures of every cell's pixel outline (HULL_COLUMNS): the crack perimeter,
        the area of the convex hull of the pixel corners and the solidity, the largest caliper (Feret diameter) with its
        angle and end points, and the smallest caliper.  The cell is the union of its pixel squares: no sub-pixel contour
        is fitted, a slanted edge's perimeter is overestimated by up to sqrt(2).  Does not need ``link``.
    :param midline: True: the table ends with the measures of every cell's skeleton (MIDLINE_COLUMNS).  Every cell is thinned
        alone to a one-pixel skeleton (Guo & Hall 1989) on the device; skeleton_length is its chain length (1 per step
        along a row or column, sqrt(2) per diagonal step), midline_length extends it at both end points to the cell's edge:
        the length of a bent or filamentous cell, where feret_max is only the chord.  NaN for a ring or a branched skeleton
        (skeleton_ends / skeleton_branches say which; boundary noise can branch a skeleton, nothing is pruned).  Chain
        lengths depend on the direction (about -11 % at 45 degrees): for straight rods feret_max is the better length, for
        round cells the midline means nothing.  Needs neither ``link`` nor ``hull``.
    :param percentiles: None or () (default): off.  1 .. 8 distinct whole numbers in 0 .. 100, e.g. (5, 50, 95): the table
        ends with p{P}_ch{c}, the P-th percentile of the cell's pixel values in every measured channel (p50 is the median),
        and bg_p{P}_ch{c}, the same over the frame's label-0 pixels (NaN for a frame without background): what one hot
        pixel, a bright neighbour or debris in the background does not move.  Linear interpolation between the two nearest
        order statistics, as ``np.percentile`` does by default; the order statistics are exact integers from the device.
        Needs ``img`` and at least one measured channel.
    :param neighbors: None (default): off.  R, a whole number in 1 .. 32: the table ends with every cell's neighbourhood
        within its frame (NEIGHBOR_COLUMNS): contact_length, the unit pixel edges it shares with other cells, border_length,
        those on the frame's border, contact_fraction, the first over all its exposed edges (= ``perimeter`` of ``hull``),
        n_touching, the cells it shares an edge with, n_neighbors, the cells with a pixel within R pixels of one of its own,
        nn_label / nn_distance / nn_gap, the nearest of them (ties to the smaller label; NaN and 0 if there is none within
        R) and contact_label / contact_max, the cell it shares the most edges with.  Whole pixels only: distances are
        centre-to-centre distances of pixels (two cells that share an edge are 1 apart, gap 0), no sub-pixel contour is
        fitted, no neighbour beyond R is seen, and this is no Voronoi or Delaunay neighbourhood.  ``cell_contacts`` gives the
        pairs themselves.  Needs neither ``link``, ``hull`` nor ``img``.
    :param spots: None (default): off.  THR, a whole number of grey levels in 1 .. 65535: the table ends with every cell's
        fluorescent FOCI in every measured channel (SPOT_COLUMNS): n_spots_ch{c}, the local maxima of the band-pass response
        (``cell_spots``; csrc/spots.hip) of at least THR grey levels under the cell, spot_max_ch{c} and
        spot_sum_ch{c}, the largest and the sum of their responses (NaN and 0 without a spot), and bg_spots_ch{c}, the
        frame's spots on label 0 (the same for all rows of a frame: how many detections to expect by chance).
        ``cell_spots`` gives the spots themselves, with their position along the cell.  Whole pixels, a fixed threshold: no
        sub-pixel positions or Gaussian fits, no automatic or noise-relative threshold, uint8 / uint16 images only, no
        linking of spots over time.  Needs ``img`` and at least one measured channel.
    :param spot_scale: s, a whole number in 1 .. 5 (default 2): the band-pass is the difference of two binomial smoothings
        with sigma = sqrt(s / 2) and sqrt(s) pixels: foci of about that radius answer best.  Read only with ``spots``.
    :param profile: None (default): off.  N, a whole number of bins in 2 .. 32: the table ends with WHERE ALONG THE CELL
        the signal of every measured channel sits.  The cell's pixels are projected on its ``orientation`` (as the integer
        direction ``profile_direction``), the projected extent is cut into N equal bins from pole to pole of the pixel set,
        and every bin's pixels and channel sums come from the device (``cell_profiles``; csrc/profile.hip).
        axis_extent: the pole-to-pole length of the pixel set along the orientation, in pixels; pole_mid_ratio_ch{c}: the
        mean value of the pixels in the pole bins (bin centre in the outer quarters of the extent) over the mean of the
        others (> 1: polar, < 1: mid-cell; NaN when either group is empty, as for N < 4); pole_asym_ch{c}: |A - B| / (A + B)
        of the two ends' pole means (0: both poles alike, 1: all at one pole); profile_peak_ch{c}: the centre, in -1 .. 1, of
        the bin with the largest mean (ties to the lower bin).  Bin 0 is the end with the smaller projection, the sense in
        which the spots' axis_pos grows; the sense is arbitrary, because a cell has no head: read |profile_peak|.  Whole
        pixels, along the straight orientation axis: a bent or filamentous cell is folded onto its chord, the bins divide
        the projected extent, not arc length; no background subtraction, no normalisation across cells.  ``cell_profiles``
        gives the profiles themselves.  Needs ``img`` and at least one measured channel.
    :return: pandas.DataFrame with the columns of ``columns(channels, link, drift is not None, hull, midline, percentiles,
        neighbors is not None, spots is not None, flow is not None, gap is not None, profile is not None)``.
    """
    drift = check_drift(drift)
    flow, flow_tile = check_flow(flow, flow_tile)
    if flow is not None and drift is None:
        raise ValueError("flow searches around the stage drift of every frame pair: it needs drift")
    percentiles = check_percentiles(percentiles)
    neighbors = check_neighbors(neighbors)
    spots = check_spots(spots, spot_scale)
    profile = check_profile(profile)
    _need_channels(img is not None, "no image given", profiles=profile is not None, percentiles=percentiles,
                   spots=spots is not None)
    if drift is not None and not link:
        raise ValueError("drift changes how cells are linked: it needs link=True")
    gap = check_gap(gap)
    if gap is not None and not link:
        raise ValueError("gap closes gaps in the links: it needs link=True")
    st = _Stack(mask, img, channels, device)
    lab, pix, off, image, channels = st.lab, st.pix, st.off, st.image, st.channels
    _need_channels(channels, "none is measured", percentiles=percentiles, spots=spots is not None,
                   profiles=profile is not None)
    with torch.cuda.device(st.dev):
        raw = measure_raw(lab, pix, off, image, channels)
        shift = pick_drift(drift_raw(lab, pix, off, drift)) if drift is not None else None
        field = pick_flow(flow_raw(lab, pix, off, shift, flow, flow_tile), shift) if flow is not None else None
        if field is not None:
            links = link_raw(lab, pix, off, field=field, tile=flow_tile)
        else:
            links = link_raw(lab, pix, off, shift=shift) if link else None
        gaps = None
        if gap is not None:
            *links, gaps = close_gaps(lab, pix, off, *links, min_overlap, gap, shift if field is None else None, field,
                                      flow_tile if field is not None else None)
        outline = hull_raw(lab, pix, off, raw["bbox"]) if hull else None
        skel = midline_raw(lab, pix, off, raw["bbox"]) if midline else None
        stats = None
        if percentiles:
            ranks = percentile_ranks(raw["shape"][0].astype(np.int64), percentiles)[0]
            bg_ranks = percentile_ranks(raw["bg_sums"][0, :, 0].astype(np.int64), percentiles)[0]
            stats = (percentiles,) + order_stats_raw(lab, pix, off, image, channels, raw["bbox"], ranks, bg_ranks)
        near = neighbors_raw(lab, pix, off, neighbors)[0] if neighbors is not None else None
        foci = (spots[1],) + spots_raw(lab, pix, off, image, channels, *spots) if spots is not None else None
        bins = profile_raw(lab, pix, off, image, channels, raw["bbox"], _cell_directions(raw), profile,
                           raw["shape"][0]) if profile is not None else None
    return table_from_sums(off, st.H, st.W, raw, channels, links, min_overlap, shift, outline, skel, stats, near, foci, field,
                           flow_tile if field is not None else None, gaps, bins)


def write_cells(df, csv_path):
    df.to_csv(csv_path, index=False)
