"""Plain numpy / fp64 restatement of the per-cell table (include/mseg_hip.h: mseg_cell_measure, mseg_cell_links; the
column rules of the issue), written from the header text: loops over labels with boolean masks, np.mean / np.std / np.min /
np.max / np.argwhere for the cells and np.bincount for the overlaps.  Imports nothing from the package."""
import math

import numpy as np
import pandas as pd

SHAPE_COLUMNS = ['frame', 'label', 'area', 'centroid_y', 'centroid_x', 'bbox_min_row', 'bbox_min_col', 'bbox_max_row',
                 'bbox_max_col', 'major_axis_length', 'minor_axis_length', 'orientation', 'touches_border']


def frame_tables(labels):
    """label_off of a stack whose frames hold the ids 1 .. max: int64 [T + 1]"""
    k = [max(int(f.max(initial=0)), 0) for f in labels]
    return np.concatenate([[0], np.cumsum(k)]).astype(np.int64)


def measure(labels, off, img=None):
    """labels [T, H, W]; off int64 [T + 1]; img [T, C, H, W] uint8 / uint16 or None -> the integer outputs of
    mseg_cell_measure (same names and layouts as the header)"""
    T, H, W = labels.shape
    n = int(off[-1])
    C = 0 if img is None else img.shape[1]
    out = {"shape": np.zeros((6, n), np.uint64), "bbox": np.zeros((n, 4), np.int32),
           "ch_sums": np.zeros((2, C, n), np.uint64), "ch_minmax": np.zeros((2, C, n), np.uint32),
           "bg_sums": np.zeros((3, T, C), np.uint64), "bg_minmax": np.zeros((2, T, C), np.uint32)}
    for t in range(T):
        for l in range(1, int(off[t + 1] - off[t]) + 1):
            m = labels[t] == l
            if not m.any():
                continue
            s = int(off[t]) + l - 1
            yx = np.argwhere(m).astype(object)                 # Python integers: exact
            y, x = yx[:, 0], yx[:, 1]
            out["shape"][:, s] = [len(y), y.sum(), x.sum(), (y * y).sum(), (x * x).sum(), (x * y).sum()]
            out["bbox"][s] = [y.min(), x.min(), y.max() + 1, x.max() + 1]
            for c in range(C):
                v = img[t, c][m].astype(object)
                out["ch_sums"][:, c, s] = [v.sum(), (v * v).sum()]
                out["ch_minmax"][:, c, s] = [v.min(), v.max()]
        b = labels[t] == 0
        for c in range(C):
            if b.any():
                v = img[t, c][b].astype(object)
                out["bg_sums"][:, t, c] = [len(v), v.sum(), (v * v).sum()]
                out["bg_minmax"][:, t, c] = [v.min(), v.max()]
    return out


def links(labels, off):
    """-> (pred int32 [n], overlap int32 [n]): per cell of frame t >= 1 the label 1 .. K_{t-1} of frame t - 1 with the most
    shared pixels (np.bincount over the cell's pixels; np.argmax takes the first = smallest label of a tie), 0 if none"""
    T = labels.shape[0]
    n = int(off[-1])
    pred, overlap = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for t in range(1, T):
        Kp = int(off[t] - off[t - 1])
        for l in range(1, int(off[t + 1] - off[t]) + 1):
            under = labels[t - 1][labels[t] == l].astype(np.int64)
            under = under[(under > 0) & (under <= Kp)]
            if under.size == 0:
                continue
            counts = np.bincount(under)
            m = int(np.argmax(counts))
            pred[int(off[t]) + l - 1], overlap[int(off[t]) + l - 1] = m, counts[m]
    return pred, overlap


# ---- the same two contracts without a loop over the labels: for stacks of millions of pixels and tens of thousands of ids ----
# Integers only: every sum is taken in uint64 (np.add.reduceat over the pixels sorted by slot), which is exact as long as the
# true value fits 64 bits.  tests/test_cells_structured_host.py holds them against measure / links above.
def _slots(labels, off):
    """-> (t, p, slot) of the pixels that are a cell of their frame, sorted by slot (stable: by t, p within a slot)"""
    T, H, W = labels.shape
    lab = labels.reshape(T, H * W).astype(np.int64)
    K = np.diff(np.asarray(off, np.int64))
    t, p = np.nonzero((lab > 0) & (lab <= K[:, None]))
    slot = np.asarray(off, np.int64)[t] + lab[t, p] - 1
    order = np.argsort(slot, kind="stable")
    return t[order], p[order], slot[order]


def measure_fast(labels, off, img=None):
    """measure(labels, off, img): same contract, same names, layouts and dtypes"""
    T, H, W = labels.shape
    n = int(off[-1])
    C = 0 if img is None else img.shape[1]
    out = {"shape": np.zeros((6, n), np.uint64), "bbox": np.zeros((n, 4), np.int32),
           "ch_sums": np.zeros((2, C, n), np.uint64), "ch_minmax": np.zeros((2, C, n), np.uint32),
           "bg_sums": np.zeros((3, T, C), np.uint64), "bg_minmax": np.zeros((2, T, C), np.uint32)}
    t, p, slot = _slots(labels, off)
    if slot.size:
        first = np.flatnonzero(np.r_[True, slot[1:] != slot[:-1]])
        s = slot[first]
        y, x = (p // W).astype(np.uint64), (p % W).astype(np.uint64)
        for j, v in enumerate((np.ones_like(y), y, x, y * y, x * x, x * y)):
            out["shape"][j, s] = np.add.reduceat(v, first)
        out["bbox"][s, 0], out["bbox"][s, 1] = np.minimum.reduceat(y, first), np.minimum.reduceat(x, first)
        out["bbox"][s, 2], out["bbox"][s, 3] = np.maximum.reduceat(y, first) + 1, np.maximum.reduceat(x, first) + 1
        for c in range(C):
            v = img[:, c].reshape(T, H * W)[t, p].astype(np.uint64)
            out["ch_sums"][0, c, s], out["ch_sums"][1, c, s] = np.add.reduceat(v, first), np.add.reduceat(v * v, first)
            out["ch_minmax"][0, c, s], out["ch_minmax"][1, c, s] = np.minimum.reduceat(v, first), np.maximum.reduceat(v, first)
    if C:
        bg = labels.reshape(T, H * W) == 0
        has = bg.any(axis=1)
        for c in range(C):
            v = img[:, c].reshape(T, H * W).astype(np.uint64)
            out["bg_sums"][0, :, c] = bg.sum(axis=1, dtype=np.uint64)
            out["bg_sums"][1, :, c] = (v * bg).sum(axis=1, dtype=np.uint64)
            out["bg_sums"][2, :, c] = (v * v * bg).sum(axis=1, dtype=np.uint64)
            out["bg_minmax"][0, :, c] = np.where(has, np.where(bg, v, np.uint64(2 ** 32)).min(axis=1), 0)
            out["bg_minmax"][1, :, c] = np.where(bg, v, np.uint64(0)).max(axis=1)
    return out


def pairs(labels, off, t):
    """the distinct (l, m) pairs of frame t over frame t - 1, both cells of their frames -> (l, m, count), sorted by l, m"""
    T, H, W = labels.shape
    l, m = labels[t].ravel().astype(np.int64), labels[t - 1].ravel().astype(np.int64)
    ok = (l > 0) & (l <= int(off[t + 1] - off[t])) & (m > 0) & (m <= int(off[t] - off[t - 1]))
    key, count = np.unique(l[ok] << 32 | m[ok], return_counts=True)
    return key >> 32, key & 0xFFFFFFFF, count


def links_fast(labels, off):
    """links(labels, off): same contract and layouts"""
    n = int(off[-1])
    pred, overlap = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for t in range(1, labels.shape[0]):
        l, m, count = pairs(labels, off, t)
        if l.size == 0:
            continue
        order = np.lexsort((m, -count, l))                     # per l: the largest count first, the smallest m of a tie first
        l, m, count = l[order], m[order], count[order]
        first = np.flatnonzero(np.r_[True, l[1:] != l[:-1]])
        s = int(off[t]) + l[first] - 1
        pred[s], overlap[s] = m[first], count[first]
    return pred, overlap


def tracks(frame, label, pred, overlap, min_overlap):
    """the track rules of the issue, restated with dictionaries"""
    cells = list(zip((int(f) for f in frame), (int(l) for l in label)))
    named, known = {}, set(cells)
    for (f, l), p, o in zip(cells, pred, overlap):
        if p > 0 and o >= min_overlap and (f - 1, int(p)) in known:
            named[(f, l)] = (f - 1, int(p))
    succ = {}
    for child, parent in named.items():
        succ[parent] = succ.get(parent, 0) + 1
    track, parent_track, nxt = {}, {}, 1
    for cell in cells:
        src = named.get(cell)
        if src is not None and succ[src] == 1:
            track[cell], parent_track[cell] = track[src], parent_track[src]
        else:
            track[cell], nxt = nxt, nxt + 1
            parent_track[cell] = track[src] if src is not None else 0
    return np.array([track[c] for c in cells], np.int64), np.array([parent_track[c] for c in cells], np.int64)


def cell_shape(mask):
    """regionprops-style values of one boolean frame mask in fp64: (area, cy, cx, bbox, major, minor, orientation,
    skip = the inertia eigenvalues differ by less than 1e-6 of the larger one: the angle is undefined)"""
    yx = np.argwhere(mask)
    y, x = yx[:, 0].astype(np.float64), yx[:, 1].astype(np.float64)
    cy, cx = np.mean(y), np.mean(x)
    vy, vx, cov = np.mean((y - cy) ** 2), np.mean((x - cx) ** 2), np.mean((y - cy) * (x - cx))
    h, q = 0.5 * (vy + vx), math.sqrt(0.25 * (vy - vx) ** 2 + cov ** 2)
    l1, l2 = h + q, h - q
    # scikit-image 0.18.3: inertia tensor [[a, b], [b, c]] = [[var_x, -cov], [-cov, var_y]]
    a, b, c = vx, -cov, vy
    if a - c == 0:
        ori = -math.pi / 4 if b < 0 else math.pi / 4
    else:
        ori = 0.5 * math.atan2(-2 * b, c - a)
    gap = bool((l1 - l2) < 1e-6 * l1)
    bbox = (int(yx[:, 0].min()), int(yx[:, 1].min()), int(yx[:, 0].max()) + 1, int(yx[:, 1].max()) + 1)
    return len(yx), cy, cx, bbox, 4 * math.sqrt(max(l1, 0.0)), 4 * math.sqrt(max(l2, 0.0)), ori, gap


def table(labels, img=None, channels=(), link=True, min_overlap=1):
    """the DataFrame of measure_cells; the extra column ``_skip`` marks cells without a defined orientation"""
    T, H, W = labels.shape
    off = frame_tables(labels)
    cols = list(SHAPE_COLUMNS)
    for c in channels:
        cols += [f"{k}_ch{c}" for k in ("mean", "std", "min", "max", "sum", "bg_mean")]
    if link:
        cols += ["pred_label", "overlap", "track_id", "parent_track"]
        pred, ovl = links(labels, off)
    rows = []
    for t in range(T):
        for l in range(1, int(off[t + 1] - off[t]) + 1):
            m = labels[t] == l
            if not m.any():
                continue
            n, cy, cx, bb, major, minor, ori, gap = cell_shape(m)
            row = [t, l, n, cy, cx, *bb, major, minor, ori, bool(bb[0] == 0 or bb[1] == 0 or bb[2] == H or bb[3] == W)]
            for c in channels:
                v = img[t, c][m]
                b = img[t, c][labels[t] == 0]
                row += [np.mean(v), np.std(v), int(np.min(v)), int(np.max(v)), int(v.astype(np.int64).sum()),
                        np.mean(b) if b.size else float("nan")]
            if link:
                s = int(off[t]) + l - 1
                row += [int(pred[s]), int(ovl[s]), 0, 0]
            rows.append(row + [gap])
    df = pd.DataFrame(rows, columns=cols + ["_skip"])
    if link:
        df["track_id"], df["parent_track"] = tracks(df["frame"], df["label"], df["pred_label"], df["overlap"], min_overlap)
    return df
