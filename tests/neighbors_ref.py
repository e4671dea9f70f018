"""Plain numpy / Python-integer restatement of the per-cell neighbourhood (include/mseg_hip.h: mseg_cell_neighbors; DESIGN.md
§6s), written from the definitions.  Within one frame, for two cells a < b: edges(a, b) = unit pixel edges between them,
d2(a, b) = the smallest squared distance between a pixel of a and a pixel of b; the pair exists when d2 <= R^2.  ``brute``
enumerates all pixel pairs of all cell pairs; ``windowed`` compares the frame with its own shifted copy for every offset of
the disc.  Neither knows of tiles, halos, half windows or hash tables (the route of the kernels).  Imports nothing from the
package."""
import numpy as np

PLANES = ["contact_edges", "border_edges", "free_edges", "n_touch", "n_near", "nn_label", "nn_d2", "contact_label",
          "contact_label_edges"]
BRUTE_PIXELS = 12 * 14    # neighbors(): larger frames go through windowed
STEPS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def cells_only(frame, K):
    """the frame with everything that is not a cell of a table of K ids (ids beyond it, negative ids) set to 0 -> int64"""
    f = np.asarray(frame).astype(np.int64)
    return np.where((f >= 1) & (f <= K), f, 0)


def assemble(K, border, free, pairs):
    """border, free: per id 0 .. K; pairs: {(a, b): (edges, d2)} of the existing pairs, a < b -> (int64 [9, K], the sorted
    rows (a, b, edges, d2)): every per-cell plane follows from the pairs by the rules of the header"""
    out = np.zeros((9, K), np.int64)
    out[1], out[2] = border[1:], free[1:]
    nearest, main = {}, {}
    rows = []
    for (a, b), (e, d) in sorted(pairs.items()):
        assert 1 <= a < b <= K and d >= 1 and (e == 0 or d == 1)
        rows.append((a, b, e, d))
        for me, other in ((a, b), (b, a)):
            out[0, me - 1] += e
            out[3, me - 1] += e > 0
            out[4, me - 1] += 1
            if me not in nearest or (d, other) < nearest[me]:
                nearest[me] = (d, other)                    # the smallest d2, ties to the smallest label
            if e > 0 and (me not in main or (-e, other) < main[me]):
                main[me] = (-e, other)                      # the most edges, ties to the smallest label
    for me, (d, other) in nearest.items():
        out[5, me - 1], out[6, me - 1] = other, d
    for me, (e, other) in main.items():
        out[7, me - 1], out[8, me - 1] = other, -e
    return out, rows


def brute(frame, K, R):
    """one frame, straight from the definitions: all pixel pairs of all cell pairs.  For frames up to 12 x 14."""
    f = cells_only(frame, K)
    H, W = f.shape
    pix = {}
    border, free = [0] * (K + 1), [0] * (K + 1)
    for y in range(H):
        for x in range(W):
            a = int(f[y, x])
            if a == 0:
                continue
            pix.setdefault(a, []).append((y, x))
            for dy, dx in STEPS:
                ny, nx = y + dy, x + dx
                if not (0 <= ny < H and 0 <= nx < W):
                    border[a] += 1
                elif f[ny, nx] == 0:
                    free[a] += 1
    pairs = {}
    ids = sorted(pix)
    for i, a in enumerate(ids):
        P = np.array(pix[a], np.int64)
        for b in ids[i + 1:]:
            Q = np.array(pix[b], np.int64)
            d2 = ((P[:, None, :] - Q[None, :, :]) ** 2).sum(axis=2)
            if d2.min() <= R * R:
                pairs[(a, b)] = (int((d2 == 1).sum()), int(d2.min()))
    return assemble(K, border, free, pairs)


def boundary_pixels(f):
    """pixels with a 4-neighbour of another value, or at the frame's edge"""
    p = np.pad(f, 1, constant_values=-1)
    inner = p[1:-1, 1:-1]
    return (inner != p[:-2, 1:-1]) | (inner != p[2:, 1:-1]) | (inner != p[1:-1, :-2]) | (inner != p[1:-1, 2:])


def windowed(frame, K, R, boundary_only=False):
    """one frame: for every offset (dy, dx) != (0, 0) of the disc dy^2 + dx^2 <= R^2 the frame against its shifted copy;
    where the two hold different cells a < b the pair's d2 is lowered to the offset's, and the four unit offsets count the
    shared edges.  ``boundary_only``: d2 is taken over 4-boundary pixels only."""
    f = cells_only(frame, K)
    H, W = f.shape
    p = np.pad(f, 1, constant_values=-1)
    inner = p[1:-1, 1:-1]
    border, free = np.zeros(K + 1, np.int64), np.zeros(K + 1, np.int64)
    for nb in (p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]):
        border += np.bincount(inner[(inner > 0) & (nb == -1)], minlength=K + 1)
        free += np.bincount(inner[(inner > 0) & (nb == 0)], minlength=K + 1)
    g = np.where(boundary_pixels(f), f, 0) if boundary_only else f
    none = np.iinfo(np.int64).max
    d2 = np.full((K + 1, K + 1), none, np.int64)
    edges = np.zeros((K + 1, K + 1), np.int64)
    for dy in range(-min(R, H - 1), min(R, H - 1) + 1):
        for dx in range(-min(R, W - 1), min(R, W - 1) + 1):
            dd = dy * dy + dx * dx
            if dd == 0 or dd > R * R:
                continue
            ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            A, B = g[ya:yb, xa:xb], g[ya + dy:yb + dy, xa + dx:xb + dx]
            m = (A > 0) & (B > A)
            a, b = A[m], B[m]
            d2[a, b] = np.minimum(d2[a, b], dd)
            if dd == 1:
                A, B = f[ya:yb, xa:xb], f[ya + dy:yb + dy, xa + dx:xb + dx]
                m = (A > 0) & (B > A)
                np.add.at(edges, (A[m], B[m]), 1)
    pairs = {(int(a), int(b)): (int(edges[a, b]), int(d2[a, b])) for a, b in np.argwhere(d2 != none)}
    return assemble(K, border.tolist(), free.tolist(), pairs)


def neighbors(lab, off, R, fn=None):
    """labels [T, H, W]; off int64 [T + 1] -> (int64 [9, n], int32 [m, 5] = frame, a, b, edges, d2 sorted by (frame, a, b)),
    the outputs of mseg_cell_neighbors (the pair rows sorted): frames of up to 12 x 14 pixels by ``brute``, larger ones by
    ``windowed``, or all by ``fn``"""
    lab = np.asarray(lab)
    out = np.zeros((9, int(off[-1])), np.int64)
    rows = []
    for t in range(lab.shape[0]):
        K = int(off[t + 1] - off[t])
        one = fn or (brute if lab[t].size <= BRUTE_PIXELS else windowed)
        planes, pairs = one(lab[t], K, R)
        out[:, int(off[t]):int(off[t + 1])] = planes
        rows += [(t,) + r for r in pairs]
    return out, np.array(rows, np.int32).reshape(-1, 5)
