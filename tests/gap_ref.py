"""Plain numpy restatement of gap closing (include/mseg_hip.h: mseg_cell_links_gap; the pass rules of DESIGN.md §6w), written
from the semantics, not from the kernel: the source frame moved by slicing (or gathered through a field), the partners by
np.bincount + np.argmax, the orphan and open-end sets as Python sets.  Imports nothing from the package."""
import numpy as np

import cells_ref as ref
import drift_ref as dref
import flow_ref as fref


def links_gap(labels, off, g, want, open, shift=None, field=None, tile=None):
    """-> (pred int32 [n], overlap int32 [n]): per cell l of frame t >= g with want[slot] the label m of frame t - g with
    open[slot of m] that shares the most pixels with l, frame t - g moved by shift[t] (or gathered through field[t]) first; ties
    to the smaller label; 0 for every other cell.  The motion is taken as given: composed over the gap by the caller."""
    T = labels.shape[0]
    off = np.asarray(off, np.int64)
    n = int(off[-1])
    pred, overlap = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for t in range(g, T):
        Kp = int(off[t - g + 1] - off[t - g])
        src = labels[t - g]
        if field is not None:
            src = fref.gathered(src, field[t], tile)
        elif shift is not None:
            src = dref.moved(src, int(shift[t][0]), int(shift[t][1]))
        src = src.astype(np.int64)
        found = np.zeros(Kp + 1, bool)                                   # found[m]: m is a cell of frame t - g and open
        found[1:] = np.asarray(open[int(off[t - g]):int(off[t - g + 1])], bool)
        src = np.where((src > 0) & (src <= Kp), src, 0)
        src = np.where(found[src], src, 0)
        for l in range(1, int(off[t + 1] - off[t]) + 1):
            s = int(off[t]) + l - 1
            if not want[s]:
                continue
            under = src[labels[t] == l]
            under = under[under > 0]
            if under.size == 0:
                continue
            counts = np.bincount(under)
            m = int(np.argmax(counts))
            pred[s], overlap[s] = m, counts[m]
    return pred, overlap


def compose(moved, g):
    """D_g[t] = moved[t] + moved[t - 1] + ... + moved[t - g + 1] with row 0 counting as 0; zero rows for t < g -> int32"""
    moved = np.asarray(moved, np.int64)
    out = np.zeros(moved.shape, np.int32)
    for t in range(g, moved.shape[0]):
        acc = np.zeros(moved.shape[1:], np.int64)
        for k in range(g):
            if t - k > 0:
                acc = acc + moved[t - k]
        out[t] = acc
    return out


def present(labels, off):
    """bool [n]: the slot's cell has at least one pixel"""
    out = np.zeros(int(off[-1]), bool)
    for t in range(labels.shape[0]):
        K = int(off[t + 1] - off[t])
        out[int(off[t]):int(off[t + 1])] = np.bincount(labels[t].ravel().astype(np.int64), minlength=K + 1)[1:K + 1] > 0
    return out


def close_gaps(labels, off, pred, overlap, min_overlap, G, shift=None, field=None, tile=None):
    """the passes g = 2 .. G + 1 of DESIGN.md §6w -> (pred, overlap, pred_gap), int32 [n] each"""
    T = labels.shape[0]
    off = np.asarray(off, np.int64)
    n = int(off[-1])
    pred, overlap = np.array(pred, np.int32), np.array(overlap, np.int32)
    pred_gap = np.where(pred > 0, 1, 0).astype(np.int32)
    has = present(labels, off)
    frame_of = np.concatenate([np.full(int(off[t + 1] - off[t]), t) for t in range(T)]) if n else np.zeros(0, int)
    orphans, named = set(), set()
    for s in range(n):
        if pred[s] > 0 and overlap[s] >= min_overlap:
            named.add(int(off[frame_of[s] - 1]) + int(pred[s]) - 1)
        elif has[s]:
            orphans.add(s)
    open_ends = {s for s in range(n) if has[s] and s not in named}
    moved = field if field is not None else shift
    for g in range(2, G + 2):
        want, open_ = np.zeros(n, bool), np.zeros(n, bool)
        want[[s for s in orphans if frame_of[s] >= g]] = True
        open_[sorted(open_ends)] = True
        over = compose(moved, g) if moved is not None else None
        p, o = links_gap(labels, off, g, want, open_, shift=over if field is None else None,
                         field=over if field is not None else None, tile=tile)
        for s in sorted(orphans):
            if p[s] > 0 and o[s] >= min_overlap:
                pred[s], overlap[s], pred_gap[s] = p[s], o[s], g
                orphans.discard(s)
                open_ends.discard(int(off[frame_of[s] - g]) + int(p[s]) - 1)
    return pred, overlap, pred_gap


def tracks(frame, label, pred, overlap, min_overlap, gap=None):
    """cells_ref.tracks with the predecessor ``gap[i]`` frames back (None: 1 everywhere)"""
    cells = list(zip((int(f) for f in frame), (int(l) for l in label)))
    back = [1] * len(cells) if gap is None else [int(b) for b in gap]
    named, known = {}, set(cells)
    for (f, l), p, o, b in zip(cells, pred, overlap, back):
        if p > 0 and o >= min_overlap and (f - b, int(p)) in known:
            named[(f, l)] = (f - b, int(p))
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


def table(labels, img=None, channels=(), min_overlap=1, gap=None, shift=None, field=None, tile=None):
    """The DataFrame of measure_cells(labels, img, channels, gap=gap) under the given motion (``shift`` [T, 2] as picked for the
    stack: with the drift columns; ``field`` [T, ty, tx, 2] with ``tile`` as well: with the flow columns; neither: none):
    cells_ref.table with the links taken under that motion, the gaps closed, pred_gap (only with ``gap``) after the link,
    drift and flow columns, and the tracks over the gaps.  The extra column ``_skip`` stays last."""
    off = ref.frame_tables(labels)
    df = ref.table(labels, img, channels, True, min_overlap)
    if field is not None:
        pred, ovl = fref.links_field(labels, off, field, tile)
    elif shift is not None:
        pred, ovl = dref.links_shifted(labels, off, shift)
    else:
        pred, ovl = ref.links(labels, off)
    pred_gap = None
    if gap is not None:
        pred, ovl, pred_gap = close_gaps(labels, off, pred, ovl, min_overlap, gap, shift if field is None else None, field, tile)
    t, l = df["frame"].to_numpy(np.int64), df["label"].to_numpy(np.int64)
    slot = off[t] + l - 1
    df["pred_label"], df["overlap"] = pred[slot].astype(np.int64), ovl[slot].astype(np.int64)
    skip = df.pop("_skip")
    if shift is not None:
        moved = np.array(shift, np.int64)
        moved[0] = 0
        total = np.cumsum(moved, axis=0)
        df["drift_y"], df["drift_x"] = total[t, 0], total[t, 1]
        df["centroid_y_reg"], df["centroid_x_reg"] = df["centroid_y"] - total[t, 0], df["centroid_x"] - total[t, 1]
    if field is not None:
        j = np.floor(df["centroid_y"].to_numpy()).astype(np.int64) // tile
        i = np.floor(df["centroid_x"].to_numpy()).astype(np.int64) // tile
        value = np.where((t > 0)[:, None], np.asarray(field, np.int64)[t, j, i], 0)
        df["flow_y"], df["flow_x"] = value[:, 0], value[:, 1]
    if gap is not None:
        df["pred_gap"] = pred_gap[slot].astype(np.int64)
    df["track_id"], df["parent_track"] = tracks(df["frame"], df["label"], df["pred_label"], df["overlap"], min_overlap,
                                                df["pred_gap"] if gap is not None else None)
    df["_skip"] = skip
    return df
