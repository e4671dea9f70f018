"""Plain numpy / Python-integer restatement of the per-cell midline integers (include/mseg_hip.h: mseg_cell_midline; DESIGN.md
§6q), written from the rule: every cell is thinned ALONE by Guo & Hall 1989, algorithm A1 (fully parallel, two sub-passes per
round, decisions on the state before the sub-pass), then the surviving pixels are counted.  One boolean array per neighbour,
whole-array expressions on boolean arrays: no bit rows, no words, no boxes handed in (the route of the kernels).  Imports nothing from the package."""
import numpy as np

PLANES = ["skel_n", "n_orth", "n_diag", "n_end", "n_branch", "rounds", "e0_y", "e0_x", "e0_d2", "e1_y", "e1_x", "e1_d2"]


def neighbours(m):
    """boolean [h, w] -> [P2, P3, ..., P9], each [h, w]: clockwise from north, everything outside the array is False"""
    q = np.pad(np.asarray(m, bool), 1)
    return [q[:-2, 1:-1], q[:-2, 2:], q[1:-1, 2:], q[2:, 2:], q[2:, 1:-1], q[2:, :-2], q[1:-1, :-2], q[:-2, :-2]]


def deletable(m, k):
    """the pixels sub-pass k deletes from the boolean mask m"""
    P2, P3, P4, P5, P6, P7, P8, P9 = neighbours(m)
    i = lambda a: a.astype(np.int64)                                                    # noqa: E731
    C = i(~P2 & (P3 | P4)) + i(~P4 & (P5 | P6)) + i(~P6 & (P7 | P8)) + i(~P8 & (P9 | P2))
    N1 = i(P9 | P2) + i(P3 | P4) + i(P5 | P6) + i(P7 | P8)
    N2 = i(P2 | P3) + i(P4 | P5) + i(P6 | P7) + i(P8 | P9)
    N = np.minimum(N1, N2)
    keep = ((P6 | P7 | ~P9) & P8) if k == 0 else ((P2 | P3 | ~P5) & P4)
    return np.asarray(m, bool) & (C == 1) & (N >= 2) & (N <= 3) & ~keep


def thin(mask):
    """boolean mask of ONE cell -> (surviving pixels, rounds run including the last, empty one)"""
    m = np.array(mask, bool)
    rounds = 0
    while True:
        rounds += 1
        deleted = False
        for k in (0, 1):
            d = deletable(m, k)
            if d.any():
                deleted = True
                m = m & ~d
        if not deleted:
            return m, rounds


def counts(S):
    """(skel_n, n_orth, n_diag, n_end, n_branch, end points in (y, x) order) of the boolean skeleton S"""
    S = np.asarray(S, bool)
    P = neighbours(S)
    P2, P3, P4, P5, P6, P7, P8, P9 = P
    n_orth = int((S & P4).sum() + (S & P6).sum())                       # every pair once: with the right and the lower one
    n_diag = int((S & P5 & ~P4 & ~P6).sum() + (S & P7 & ~P8 & ~P6).sum())
    degree = sum(p.astype(np.int64) for p in P)
    ends = S & (degree == 1)
    crossing = sum((~a & b).astype(np.int64) for a, b in zip(P, P[1:] + P[:1]))
    return int(S.sum()), n_orth, n_diag, int(ends.sum()), int((S & (crossing >= 3)).sum()), \
        [(int(y), int(x)) for y, x in np.argwhere(ends)]


def nearest_outside2(cell, y, x):
    """squared distance from (y, x) to the nearest position that is not of the cell; rows -1 and H, columns -1 and W count"""
    out = ~np.pad(np.asarray(cell, bool), 1)
    ys, xs = np.nonzero(out)
    return int(((ys - 1 - y) ** 2 + (xs - 1 - x) ** 2).min())


def cell(frame, l, origin=(0, 0)):
    """-> (the twelve integers of cell l of one frame, its skeleton as a boolean image of the frame); ``origin``: the (row,
    column) of the frame's first pixel, for a frame that is a window of a larger one.  Works on the cell cut to its own extent:
    thinning never looks further than one pixel, and the nearest position outside the cell is never further out than the ring
    around that extent (test_midline_host.py checks it against the whole frame)"""
    whole = np.asarray(frame) == l
    if not whole.any():
        return [0] * 12, whole
    ys, xs = np.nonzero(whole.any(axis=1))[0], np.nonzero(whole.any(axis=0))[0]
    oy, ox = int(ys[0]), int(xs[0])
    m = whole[oy:int(ys[-1]) + 1, ox:int(xs[-1]) + 1]
    S, rounds = thin(m)
    n, n_orth, n_diag, n_end, n_branch, ends = counts(S)
    if n == 1:
        ends = [tuple(int(v) for v in np.argwhere(S)[0])]
    tail = [0] * 6
    if ends:
        (y0, x0), (y1, x1) = ends[0], ends[-1]
        dy, dx = oy + origin[0], ox + origin[1]
        tail = [y0 + dy, x0 + dx, nearest_outside2(m, y0, x0), y1 + dy, x1 + dx, nearest_outside2(m, y1, x1)]
    image = np.zeros(whole.shape, bool)
    image[oy:oy + m.shape[0], ox:ox + m.shape[1]] = S
    return [n, n_orth, n_diag, n_end, n_branch, rounds] + tail, image


def midline(labels, off):
    """labels [T, H, W]; off int64 [T + 1] -> (int64 [12, n], uint8 [T, H, W]), the outputs of mseg_cell_midline: ids 1 .. K_t
    of frame t; ids beyond the table and negative ids are not a cell.  Every cell is handed to ``cell`` in the window of the
    frame that its pixels span (one sort of the frame's cell pixels), so that a large frame costs no whole-frame pass per cell"""
    labels = np.asarray(labels)
    out = np.zeros((12, int(off[-1])), np.int64)
    skeleton = np.zeros(labels.shape, np.uint8)
    for t in range(labels.shape[0]):
        frame = labels[t].astype(np.int64)
        ys, xs = np.nonzero((frame >= 1) & (frame <= int(off[t + 1] - off[t])))
        if len(ys) == 0:
            continue
        ids = frame[ys, xs]
        order = np.argsort(ids, kind="stable")
        ids, ys, xs = ids[order], ys[order], xs[order]
        starts = np.flatnonzero(np.concatenate([[True], ids[1:] != ids[:-1]]))
        tops, lefts = np.minimum.reduceat(ys, starts), np.minimum.reduceat(xs, starts)
        bottoms, rights = np.maximum.reduceat(ys, starts), np.maximum.reduceat(xs, starts)
        for l, y0, x0, y1, x1 in zip(ids[starts].tolist(), tops.tolist(), lefts.tolist(), bottoms.tolist(), rights.tolist()):
            out[:, int(off[t]) + l - 1], S = cell(frame[y0:y1 + 1, x0:x1 + 1], l, (y0, x0))
            skeleton[t, y0:y1 + 1, x0:x1 + 1][S] = 1
    return out, skeleton
