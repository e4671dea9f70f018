"""numpy restatement of ``(65535 * skimage.exposure.equalize_adapthist(img, clip_limit=0.01)).astype(np.uint16)`` as
scikit-image 0.18.3 computes it for one 2-D uint8 / uint16 image (DESIGN.md §6j lists the steps).  Written from the
algorithm, step by step and per tile, so that it shares no vectorised reshaping with the library: the fixtures of
tests/golden/clahe_library.npz pin it against the library itself (test_clahe_host.py), and it then serves as the
reference for shapes without a fixture and on machines without scikit-image.
"""
import numpy as np

GRAY = 16384                       # grey levels the library works on
NBINS = 256
BIN = 1 + GRAY // NBINS            # 65 levels per bin: only bins 0..252 are ever hit


def stretch(img):
    """steps 1-2: img_as_uint, then the stretch to 0..16383 (round half to even), uint16"""
    if img.dtype == np.uint8:
        v = img.astype(np.uint16) * np.uint16(257)
    elif img.dtype == np.uint16:
        v = img
    else:
        raise ValueError("clahe_ref: uint8 or uint16 images only")
    lo, hi = float(v.min()), float(v.max())
    f = v.astype(np.float64)
    if lo != hi:
        g = ((f - lo) / (hi - lo)) * float(GRAY - 1)
    else:
        g = np.minimum(f, float(GRAY - 1))
    return np.rint(g).astype(np.uint16)


def reflect(i, n):
    """index into an axis of length n padded by numpy's 'reflect' (the edge sample is not repeated)"""
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def clip_histogram(h, clim):
    """step 6, on a list of 256 Python ints; returns the clipped histogram"""
    h = [int(x) for x in h]
    n = len(h)
    excess = sum(x - clim for x in h if x > clim)
    h = [min(x, clim) for x in h]
    incr = excess // n
    upper = clim - incr
    for b in range(n):
        if h[b] < upper:
            h[b] += incr
            excess -= incr
    for b in range(n):                      # after the increments: a raised bin that reached `upper` is filled up too
        if upper <= h[b] < clim:
            excess += h[b] - clim
            h[b] = clim
    while excess > 0:
        prev = excess
        for index in range(n):
            under = [x < clim for x in h]
            step = max(1, sum(under) // excess)
            done = 0
            for b in range(index, n, step):
                if under[b]:
                    h[b] += 1
                    done += 1
            excess -= done
            if excess <= 0:
                break
        if prev == excess:
            break
    return h


def tile_maps(g, ky, kx):
    """steps 3-7: grey-level mapping [ny][nx][256] (int64) of every tile of the grid"""
    H, W = g.shape
    ny, nx = -(-H // ky), -(-W // kx)       # padded // k - 1
    bins = (g // BIN).astype(np.int64)
    clim = int(max(0.01 * (ky * kx), 1))
    scale = float(GRAY - 1) / float(ky * kx)
    maps = np.zeros((ny, nx, NBINS), np.int64)
    for i in range(ny):
        rows = reflect(np.arange(i * ky, (i + 1) * ky), H)
        for j in range(nx):
            cols = reflect(np.arange(j * kx, (j + 1) * kx), W)
            h = np.bincount(bins[np.ix_(rows, cols)].ravel(), minlength=NBINS)
            h = clip_histogram(h, clim)
            m = np.cumsum(np.asarray(h, np.int64)).astype(np.float64) * scale
            maps[i, j] = np.minimum(m, float(GRAY - 1)).astype(np.int64)
    return maps


def interpolate(g, maps, ky, kx):
    """step 8: bilinear blend of the four surrounding tile maps, fp64 products rounded to fp32 and summed in fp32"""
    H, W = g.shape
    ny, nx = maps.shape[:2]
    bins = (g // BIN).astype(np.int64)
    py, px = np.arange(H) + ky // 2, np.arange(W) + kx // 2          # position in the padded image
    bi, bj = py // ky, px // kx
    cy, cx = (py % ky) / float(ky), (px % kx) / float(kx)
    acc = np.zeros((H, W), np.float32)
    for e0 in (0, 1):
        ti = np.clip(bi + e0 - 1, 0, ny - 1)                         # the map grid is edge-replicated by one tile
        wy = cy if e0 else 1 - cy
        for e1 in (0, 1):
            tj = np.clip(bj + e1 - 1, 0, nx - 1)
            wx = cx if e1 else 1 - cx
            m = maps[ti[:, None], tj[None, :], bins]
            acc += (m * (wx[None, :] * wy[:, None])).astype(np.float32)
    return acc.astype(np.uint16)


def rescale_out(u):
    """step 9: img_as_float, rescale_intensity to 0..1, and the caller's uint16(65535 * f)"""
    f = u.astype(np.float64) * (1.0 / 65535)
    a, b = float(f.min()), float(f.max())
    f = (f - a) / (b - a) if a != b else np.clip(f, 0.0, 1.0)
    return (65535 * f).astype(np.uint16)


def clahe_ref(img):
    """uint8 / uint16 (H, W) -> uint16 (H, W)"""
    img = np.asarray(img)
    if img.ndim != 2 or min(img.shape) < 8:
        raise ValueError("clahe_ref: one 2-D image of at least 8 x 8")
    g = stretch(img)
    ky, kx = img.shape[0] // 8, img.shape[1] // 8
    return rescale_out(interpolate(g, tile_maps(g, ky, kx), ky, kx))
