"""Plain numpy restatement of drift-compensated linking (include/mseg_hip.h: mseg_stack_drift, mseg_cell_links_shifted; the
pick rule of the issue), written from the header text: the score surface by slicing two boolean frames against each other,
the shifted links by np.bincount over a shifted copy of the previous frame.  Imports nothing from the package."""
import numpy as np


def foreground(labels, off):
    """bool [T, H, W]: the id of a pixel is in 1 .. K_t"""
    k = np.diff(np.asarray(off, np.int64))
    lab = labels.astype(np.int64)
    return (lab > 0) & (lab <= k[:, None, None])


def overlap_at(cur, prev, dy, dx):
    """pixels where ``prev`` moved by (dy, dx) lies on ``cur`` (two boolean frames); moved out of the frame counts nothing"""
    H, W = cur.shape
    if abs(dy) >= H or abs(dx) >= W:
        return 0
    a = cur[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)]
    b = prev[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return int(np.count_nonzero(a & b))


def scores(lab, off, R):
    """-> uint32 [T - 1, 2R + 1, 2R + 1]: scores[t - 1, dy + R, dx + R] = overlap_at(F_t, F_{t-1}, dy, dx)"""
    fg = foreground(lab, off)
    T = lab.shape[0]
    out = np.zeros((max(T - 1, 0), 2 * R + 1, 2 * R + 1), np.uint32)
    for t in range(1, T):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                out[t - 1, dy + R, dx + R] = overlap_at(fg[t], fg[t - 1], dy, dx)
    return out


def pick(sc):
    """-> int32 [T, 2], row 0 = (0, 0): per pair the shift of the largest score; among equal scores the smallest
    dy^2 + dx^2, then the smaller dy, then the smaller dx; (0, 0) where the best score is 0"""
    R = sc.shape[1] // 2
    out = np.zeros((sc.shape[0] + 1, 2), np.int32)
    for t, surface in enumerate(sc, start=1):
        best = None
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                key = (-int(surface[dy + R, dx + R]), dy * dy + dx * dx, dy, dx)
                if best is None or key < best:
                    best = key
        if best[0] != 0:
            out[t] = best[2], best[3]
    return out


def moved(frame, dy, dx):
    """``frame`` moved by (dy, dx): out[y, x] = frame[y - dy, x - dx], 0 where that lies outside"""
    H, W = frame.shape
    out = np.zeros_like(frame)
    if abs(dy) >= H or abs(dx) >= W:
        return out
    out[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = \
        frame[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return out


def links_shifted(lab, off, shift):
    """cells_ref.links with frame t - 1 moved by shift[t] = (dy, dx) first -> (pred int32 [n], overlap int32 [n])"""
    T = lab.shape[0]
    n = int(off[-1])
    pred, overlap = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for t in range(1, T):
        Kp = int(off[t] - off[t - 1])
        prev = moved(lab[t - 1], int(shift[t][0]), int(shift[t][1]))
        for l in range(1, int(off[t + 1] - off[t]) + 1):
            under = prev[lab[t] == l].astype(np.int64)
            under = under[(under > 0) & (under <= Kp)]
            if under.size == 0:
                continue
            counts = np.bincount(under)
            m = int(np.argmax(counts))
            pred[int(off[t]) + l - 1], overlap[int(off[t]) + l - 1] = m, counts[m]
    return pred, overlap


def drifting_stack(H, W, T, n_cells, offsets, seed):
    """Non-overlapping small ellipses (semi-axes 2 - 4 px) on a canvas larger than the frame; frame t is the canvas moved by
    the sum of offsets[:t] (offsets: T - 1 pairs (dy, dx)), so frame_t(y, x) = frame_{t-1}(y - dy_t, x - dx_t) wherever both
    are inside: cells enter and leave at the borders, and a cell keeps its canvas id in every frame.
    -> (uint16 [T, H, W], canvas uint16)"""
    assert len(offsets) == T - 1
    rng = np.random.default_rng(seed)
    total = np.concatenate([[[0, 0]], np.cumsum(np.asarray(offsets, np.int64).reshape(-1, 2), axis=0)])
    margin = int(np.abs(total).max()) + 1
    Hc, Wc = H + 2 * margin, W + 2 * margin
    yy, xx = np.mgrid[:Hc, :Wc]
    canvas = np.zeros((Hc, Wc), np.uint16)
    placed = []
    for _ in range(200 * n_cells):
        if len(placed) == n_cells:
            break
        cy, cx = rng.uniform(4, Hc - 5), rng.uniform(4, Wc - 5)
        a, b, th = rng.uniform(2, 4), rng.uniform(2, 4), rng.uniform(0, np.pi)
        if any((cy - p[0]) ** 2 + (cx - p[1]) ** 2 <= (max(a, b) + p[2] + 1.5) ** 2 for p in placed):
            continue
        u = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th)
        v = -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
        placed.append((cy, cx, max(a, b)))
        canvas[(u / a) ** 2 + (v / b) ** 2 <= 1] = len(placed)
    assert len(placed) == n_cells, "canvas too crowded"
    lab = np.zeros((T, H, W), np.uint16)
    for t in range(T):
        y0, x0 = margin - int(total[t][0]), margin - int(total[t][1])
        lab[t] = canvas[y0:y0 + H, x0:x0 + W]
    return lab, canvas
