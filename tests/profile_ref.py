"""The per-cell intensity profile restated with numpy from the rule, never from the kernel: for cell s with the
integer direction (uy, ux), over its pixels (y, x) inside its box (clipped to the frame): q = uy y + ux x in int64, qmin / qmax
its extremes, bin b = floor((q - qmin) N / (qmax - qmin + 1)) clamped to 0 .. N - 1; count[b], sums[c][b], qmin, qmax.
Python / int64 arithmetic only."""
import numpy as np


def bins_of(q, N):
    """int64 projections of one cell's pixels -> (bins int64, qmin, qmax); exact: floor division of Python-sized integers"""
    q = np.asarray(q, np.int64)
    qmin, qmax = int(q.min()), int(q.max())
    D = qmax - qmin + 1
    if D * N < 2 ** 62:
        b = (q - qmin) * N // D
    else:
        b = np.array([(int(v) - qmin) * N // D for v in q.tolist()], np.int64)
    return np.clip(b, 0, N - 1), qmin, qmax


def profile(labels, off, img, bbox, dirs, N):
    """labels [T, H, W]; off int64 [T + 1]; img [T, C, H, W] uint8 / uint16; bbox int [n, 4] (r0, c0, r1, c1, half-open; zeros:
    absent); dirs int [n, 2] = (uy, ux) -> (count uint32 [N, n], sums uint64 [C, N, n], extent int64 [2, n]): the outputs of
    mseg_cell_profile.  Ids beyond the frame's table and negative ids belong to no slot; a box without a pixel of its cell
    gives zeros."""
    T, H, W = labels.shape
    n, C = int(off[-1]), img.shape[1]
    count, sums = np.zeros((N, n), np.uint32), np.zeros((C, N, n), np.uint64)
    extent = np.zeros((2, n), np.int64)
    bbox, dirs = np.asarray(bbox, np.int64).reshape(n, 4), np.asarray(dirs, np.int64).reshape(n, 2)
    for t in range(T):
        for s in range(int(off[t]), int(off[t + 1])):
            r0, c0 = max(int(bbox[s, 0]), 0), max(int(bbox[s, 1]), 0)
            r1, c1 = min(int(bbox[s, 2]), H), min(int(bbox[s, 3]), W)
            if r1 <= r0 or c1 <= c0:
                continue
            y, x = np.nonzero(labels[t, r0:r1, c0:c1].astype(np.int64) == s - int(off[t]) + 1)
            if y.size == 0:
                continue
            y, x = y.astype(np.int64) + r0, x.astype(np.int64) + c0
            b, extent[0, s], extent[1, s] = bins_of(int(dirs[s, 0]) * y + int(dirs[s, 1]) * x, N)
            count[:, s] = np.bincount(b, minlength=N)
            for c in range(C):
                v = img[t, c, y, x].astype(np.int64)
                lo, hi = np.bincount(b, weights=(v & 0xFF).astype(np.float64), minlength=N), \
                    np.bincount(b, weights=(v >> 8).astype(np.float64), minlength=N)      # < 2^31 * 255: exact in fp64
                sums[c, :, s] = [int(l) + (int(h) << 8) for l, h in zip(lo, hi)]
    return count, sums, extent
