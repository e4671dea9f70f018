"""Plain numpy restatement of linking under a tile-wise displacement field (include/mseg_hip.h: mseg_stack_flow,
mseg_cell_links_field; the pick rule of DESIGN.md §6v), written from the header text: the tile scores by slicing a moved
boolean frame, the links by np.bincount over a previous frame gathered through the field.  Imports nothing from the package."""
import numpy as np

import drift_ref as dref


def tiles(H, W, B):
    return -(-H // B), -(-W // B)


def scores(lab, off, base, r, B):
    """-> uint32 [T - 1, ty, tx, 2r + 1, 2r + 1]: scores[t - 1, j, i, ey + r, ex + r] = pixels of tile (j, i) of frame t that
    are foreground and lie on the foreground of frame t - 1 moved by base[t] + (ey, ex)"""
    fg = dref.foreground(lab, off)
    T, H, W = lab.shape
    ty, tx = tiles(H, W, B)
    out = np.zeros((max(T - 1, 0), ty, tx, 2 * r + 1, 2 * r + 1), np.uint32)
    for t in range(1, T):
        for ey in range(-r, r + 1):
            for ex in range(-r, r + 1):
                both = fg[t] & dref.moved(fg[t - 1], int(base[t][0]) + ey, int(base[t][1]) + ex)
                for j in range(ty):
                    for i in range(tx):
                        out[t - 1, j, i, ey + r, ex + r] = np.count_nonzero(both[j * B:(j + 1) * B, i * B:(i + 1) * B])
    return out


def pick(sc, base):
    """-> int32 [T, ty, tx, 2], frame 0 zeros: per tile base[t] + the deviation of the largest score; among equal scores the
    smallest ey^2 + ex^2, then the smaller ey, then the smaller ex; deviation (0, 0) where the best score is 0"""
    pairs, ty, tx, side = sc.shape[:4]
    r = side // 2
    out = np.zeros((pairs + 1, ty, tx, 2), np.int32)
    for t in range(1, pairs + 1):
        for j in range(ty):
            for i in range(tx):
                best = None
                for ey in range(-r, r + 1):
                    for ex in range(-r, r + 1):
                        key = (-int(sc[t - 1, j, i, ey + r, ex + r]), ey * ey + ex * ex, ey, ex)
                        if best is None or key < best:
                            best = key
                dev = (best[2], best[3]) if best[0] != 0 else (0, 0)
                out[t, j, i] = int(base[t][0]) + dev[0], int(base[t][1]) + dev[1]
    return out


def gathered(frame, field_t, B):
    """out[y, x] = frame[y - field_t[y // B, x // B, 0], x - field_t[y // B, x // B, 1]], 0 where that lies outside"""
    H, W = frame.shape
    yy, xx = np.mgrid[:H, :W]
    f = np.asarray(field_t, np.int64)
    ys, xs = yy - f[yy // B, xx // B, 0], xx - f[yy // B, xx // B, 1]
    inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    out = np.zeros_like(frame)
    out[inside] = frame[ys[inside], xs[inside]]
    return out


def links_field(lab, off, field, B):
    """cells_ref.links with frame t - 1 gathered through field[t] first -> (pred int32 [n], overlap int32 [n]); the largest
    overlap, ties to the smaller label"""
    T = lab.shape[0]
    n = int(off[-1])
    pred, overlap = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for t in range(1, T):
        Kp = int(off[t] - off[t - 1])
        prev = gathered(lab[t - 1], field[t], B)
        for l in range(1, int(off[t + 1] - off[t]) + 1):
            under = prev[lab[t] == l].astype(np.int64)
            under = under[(under > 0) & (under <= Kp)]
            if under.size == 0:
                continue
            counts = np.bincount(under)
            m = int(np.argmax(counts))
            pred[int(off[t]) + l - 1], overlap[int(off[t]) + l - 1] = m, counts[m]
    return pred, overlap


def expanding_stack(H, W, T, n_cells, growth, offsets, seed):
    """A colony that expands about the frame's centre c and jumps with the stage: non-overlapping rods (ellipses with
    semi-axes 3 - 6 and 1.5 - 2.5 px) whose centres lie at c + (1 + growth)^t p_i + the sum of offsets[:t] in frame t
    (offsets: T - 1 pairs (dy, dx)); the rods keep size and direction, and cell i has the id i + 1 in every frame.  The p_i
    are drawn so far apart that the rods do not overlap in frame 0, and only move apart after it.  Cells (partly) outside the
    frame are cut.  -> uint16 [T, H, W]"""
    assert len(offsets) == T - 1
    rng = np.random.default_rng(seed)
    total = np.concatenate([[[0, 0]], np.cumsum(np.asarray(offsets, np.int64).reshape(-1, 2), axis=0)])
    c = np.array([(H - 1) / 2, (W - 1) / 2])
    placed = []
    for _ in range(500 * n_cells):
        if len(placed) == n_cells:
            break
        p = np.array([rng.uniform(-0.42 * H, 0.42 * H), rng.uniform(-0.42 * W, 0.42 * W)])
        a, b, th = rng.uniform(3, 6), rng.uniform(1.5, 2.5), rng.uniform(0, np.pi)
        if any(np.hypot(*(p - q[0])) <= a + q[1] + 1.5 for q in placed):
            continue
        placed.append((p, a, b, th))
    assert len(placed) == n_cells, "colony too crowded"
    yy, xx = np.mgrid[:H, :W]
    lab = np.zeros((T, H, W), np.uint16)
    for t in range(T):
        for k, (p, a, b, th) in enumerate(placed, start=1):
            cy, cx = c + (1 + growth) ** t * p + total[t]
            u = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th)
            v = -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
            inside = (u / a) ** 2 + (v / b) ** 2 <= 1
            assert not lab[t][inside].any(), "rods overlap"
            lab[t][inside] = k
    return lab
