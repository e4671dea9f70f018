"""numpy restatements of the band-pass response and the peak test of mseg_cell_spots; no GPU, no torch.

Two independent ways to D = 16^s B_s(v) - B_2s(v):
  (a) ``response``:        np.pad(mode='edge') by 2s, then an explicit loop over the binomial taps C(2k, j) in int64
  (b) ``response_passes``: the same padding, then k 'valid' passes of [1 2 1] per axis (valid convolutions compose, so the
                           2s-wide edge extension is consumed exactly: the same numbers)
``spots`` is a plain loop over the pixels."""
from math import comb

import numpy as np


def _taps_axis(p, k, axis):
    """'valid' correlation of the int64 array ``p`` with C(2k, j) along ``axis``: the axis shrinks by 2k"""
    n = p.shape[axis] - 2 * k
    out = np.zeros_like(np.take(p, range(n), axis=axis))
    for j in range(2 * k + 1):
        out += comb(2 * k, j) * np.take(p, range(j, j + n), axis=axis)
    return out


def smooth(v, k, pad):
    """B_k(v) of a plane padded by ``pad`` >= k edge pixels, cropped to the plane's size; int64"""
    p = np.pad(np.asarray(v).astype(np.int64), pad, mode='edge')
    c = pad - k
    p = p[c:p.shape[0] - c, c:p.shape[1] - c]
    return _taps_axis(_taps_axis(p, k, 1), k, 0)


def response(v, s):
    """(a): D, int64 [H, W]"""
    return (16 ** s) * smooth(v, s, 2 * s) - smooth(v, 2 * s, 2 * s)


def _passes(p, k):
    for _ in range(k):
        p = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    for _ in range(k):
        p = p[:-2] + 2 * p[1:-1] + p[2:]
    return p


def response_passes(v, s):
    """(b): D, int64 [H, W]"""
    p = np.pad(np.asarray(v).astype(np.int64), 2 * s, mode='edge')
    return (16 ** s) * _passes(p[s:p.shape[0] - s, s:p.shape[1] - s], s) - _passes(p, 2 * s)


def spots(d, thr, s):
    """the spots of one plane's response ``d``: [(y, x)] in raster order"""
    H, W = d.shape
    floor = int(thr) * 16 ** (2 * s)
    out = []
    for y in range(H):
        for x in range(W):
            v = int(d[y, x])
            if v < floor:
                continue
            ok = True
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if (dy == 0 and dx == 0) or not (0 <= yy < H and 0 <= xx < W):
                        continue
                    w = int(d[yy, xx])
                    before = (yy, xx) < (y, x)
                    if not (v > w or (v == w and not before)):
                        ok = False
            if ok:
                out.append((y, x))
    return out


def reference(labels, off, img, channels, thr, s):
    """what ``spots_raw`` returns for labels [T, H, W], the host table ``off`` [T + 1] and img [T, C, H, W]: (cell_count
    int32 [len(channels), n], bg_count int32 [T, len(channels)], records [(frame, channel index, y, x, label, value, d)]
    sorted by (frame, channel index, y, x))"""
    labels = np.asarray(labels).astype(np.int64)
    T = labels.shape[0]
    n = int(off[-1])
    cell = np.zeros((len(channels), n), np.int32)
    bg = np.zeros((T, len(channels)), np.int32)
    recs = []
    for t in range(T):
        for ci, c in enumerate(channels):
            d = response(img[t, c], s)
            for y, x in spots(d, thr, s):
                l = int(labels[t, y, x])
                if l == 0:
                    bg[t, ci] += 1
                elif 1 <= l <= int(off[t + 1] - off[t]):
                    cell[ci, int(off[t]) + l - 1] += 1
                recs.append((t, ci, y, x, l, int(img[t, c, y, x]), int(d[y, x])))
    return cell, bg, recs
