"""Plain numpy references of the training-augmentation kernels of libmseg_hip (csrc/augment.hip), written from the formulas
in include/mseg_hip.h and the kernels' header comments alone; one plane [H][W] (or one sample) at a time:

  uint16 -> fp32                                                   mseg_aug_u16_to_f32
  the eight symmetries of the square                               mseg_aug_flip
  affine warp, bilinear / nearest, constant border 0               mseg_aug_affine
  separable Gaussian blur, radius int(4 sigma + 0.5), 'reflect'    mseg_aug_blur
  min / max / mean and the 65536-bin histogram                     mseg_aug_stats
  percentiles (linear interpolation between order statistics)      mseg_aug_contrast_params, mode 1
  the six parameters of contrast + gamma                           mseg_aug_contrast_params, mode 2
  percentile stretch, contrast + gamma                             mseg_aug_contrast
  CLAHE: interpolation between the tile mappings                   mseg_aug_clahe  (the mappings: oracle/augment_ref.py)
  min-max normalisation to [-1, 1]                                 mseg_aug_noise_normalize

tests/test_augment_ref_host.py pins them to numpy / scipy on the CPU; the GPU tests then use them as the yardstick.  The
smooth operations take a ``dtype``: np.float64 is the reference, np.float32 restates the same formula in the kernel's
order of operations and exists only to measure what that formula costs in the kernel's precision (e_ref).
"""
import numpy as np

GRAY, BINS, TILES = 16384, 256, 8


# ---- uint16 -> fp32, flips ----------------------------------------------------------------------------------------------------
def u16_to_f32(a):
    return np.asarray(a, dtype=np.uint16).astype(np.float32)


def flip(a, code):
    """out[i][j] = a[si][sj]: 0 identity, 1 left-right, 2 up-down, 3 rot90 (counter-clockwise), 4 rot180, 5 rot270,
    6 left-right then rot90, 7 up-down then rot90.  Codes >= 3 transpose: square planes only."""
    a = np.asarray(a)
    H, W = a.shape
    if code >= 3 and code != 4 and H != W:
        raise ValueError("a transposing flip needs a square plane")
    i, j = np.mgrid[0:H, 0:W]
    si, sj = {0: (i, j), 1: (i, W - 1 - j), 2: (H - 1 - i, j), 3: (j, W - 1 - i), 4: (H - 1 - i, W - 1 - j),
              5: (H - 1 - j, i), 6: (j, i), 7: (H - 1 - j, W - 1 - i)}[int(code)]
    return a[si, sj]


# ---- affine warp ----------------------------------------------------------------------------------------------------------------
def warp_coords(m, H, W, dtype=np.float64):
    """source coordinates (sx, sy) of every destination pixel: sx = m0 x + m1 y + m2, sy = m3 x + m4 y + m5, from the fp32
    matrix entries the kernel reads (evaluated in ``dtype``, left to right)"""
    m = np.asarray(m, dtype=np.float32).astype(dtype)
    y, x = np.mgrid[0:H, 0:W].astype(dtype)
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


def _at(a, yy, xx):
    """a[yy][xx] with the constant border 0"""
    H, W = a.shape
    ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
    return np.where(ok, a[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], a.dtype.type(0))


def affine_bilinear(a, m, dtype=np.float64):
    a = np.asarray(a).astype(dtype)
    H, W = a.shape
    sx, sy = warp_coords(m, H, W, dtype)
    fx, fy = np.floor(sx), np.floor(sy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = sx - fx, sy - fy
    one = dtype(1)
    return (one - ay) * ((one - ax) * _at(a, y0, x0) + ax * _at(a, y0, x0 + 1)) + \
        ay * ((one - ax) * _at(a, y0 + 1, x0) + ax * _at(a, y0 + 1, x0 + 1))


# Warps of the test set whose geometry puts more than 1 % of a plane's coordinates ON a rounding boundary, so that nearest
# sampling has no defined answer there: sin 30 = 1 / 2 about the integer centre (11, 8) of 17 x 23 (centre row and column);
# 45 degrees about (31.5, 31.5) (the anti-diagonal maps to x = 31.5); 1 / 1.1 about 31.5 (columns 26 and 37).
NEAREST_ON_BOUNDARY = {("rot30", (17, 23)), ("rot45", (64, 64)), ("scale1.1x0.9", (64, 64))}


def affine_nearest(a, m, margin=1e-4):
    """-> (plane, unsure): the source index is floor(s + 0.5) of the fp64 coordinate; ``unsure`` marks the pixels one of whose
    fp64 coordinates lies within ``margin`` px of a rounding boundary (k + 0.5), where fp32 may decide otherwise"""
    a = np.asarray(a)
    H, W = a.shape
    sx, sy = warp_coords(m, H, W)
    tx, ty = sx + 0.5, sy + 0.5
    unsure = (np.abs(tx - np.rint(tx)) < margin) | (np.abs(ty - np.rint(ty)) < margin)
    return _at(a, np.floor(ty).astype(np.int64), np.floor(tx).astype(np.int64)), unsure


# ---- blur -------------------------------------------------------------------------------------------------------------------------
def blur_radius(sigma):
    s = float(np.float32(sigma))
    r = int(4.0 * s + 0.5)
    assert r == int(np.float32(4.0) * np.float32(sigma) + np.float32(0.5)), "fp32 and fp64 disagree about the radius"
    return r


def _reflect(q, L):
    """scipy 'reflect' (d c b a | a b c d | d c b a): period 2 L, mirrored about -0.5 and L - 0.5, any distance"""
    q = np.mod(q, 2 * L)
    return np.where(q >= L, 2 * L - 1 - q, q)


def _blur_axis(a, sigma, axis, dtype):
    L = a.shape[axis]
    r = blur_radius(sigma)
    s = dtype(np.float32(sigma))
    inv2s2 = dtype(-0.5) / (s * s)
    c = np.arange(L)
    acc, wsum = np.zeros(a.shape, dtype), dtype(0)
    for k in range(-r, r + 1):                       # the kernel's order: k ascending, acc and the weight sum side by side
        wgt = np.exp(inv2s2 * dtype(k * k)).astype(dtype)
        acc = acc + wgt * np.take(a, _reflect(c + k, L), axis=axis)
        wsum = wsum + wgt
    return acc / wsum


def blur(a, sigma, dtype=np.float64):
    """rows first (axis 0), then columns, as scipy.ndimage.gaussian_filter orders its passes; sigma <= 0 copies"""
    a = np.asarray(a).astype(dtype)
    if not sigma > 0:
        return a
    return _blur_axis(_blur_axis(a, sigma, 0, dtype), sigma, 1, dtype)


# ---- statistics, percentiles --------------------------------------------------------------------------------------------------------
def stats(a):
    """-> (min, max, mean as float32(fp64 sum / hw), histogram of clip(floor(v + 0.5), 0, 65535)) of an fp32 plane"""
    v = np.asarray(a, dtype=np.float32).astype(np.float64).ravel()
    b = np.clip(np.floor(v + 0.5), 0, 65535).astype(np.int64)
    return np.float32(v.min()), np.float32(v.max()), np.float32(v.sum() / v.size), np.bincount(b, minlength=65536)


def percentile(values, q):
    """np.percentile's default: position q / 100 (n - 1) between the order statistics, linear in between; q is the fp32
    number the kernel reads"""
    v = np.sort(np.asarray(values, dtype=np.float64).ravel())
    pos = float(np.float32(q)) / 100.0 * (v.size - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, v.size - 1)
    return v[lo] + (pos - lo) * (v[hi] - v[lo])


def contrast_params_mode2(st, factor, gamma, dtype=np.float64):
    """par[0..5] = {2, mean, f, umin, umax - umin, gamma} from stats = {min, max, mean} (fp32) of v: statistics of
    u = (v / 65535 - mean) f + mean follow from the ends, the step being linear"""
    mn, mx, mean = (dtype(np.float32(x)) / dtype(65535) for x in st)
    f = dtype(np.float32(factor))
    a, b = (mn - mean) * f + mean, (mx - mean) * f + mean
    umin, umax = min(a, b), max(a, b)
    return np.array([2, mean, f, umin, umax - umin, dtype(np.float32(gamma))], dtype=dtype)


# ---- contrast, pointwise --------------------------------------------------------------------------------------------------------------
def contrast(v, par, dtype=np.float64):
    """-> (out, pre): out = floor(pre).  mode 1: pre = clip((v - p0) / (p1 - p0), 0, 1) 65535 + 0.5, and all zeros when
    p1 <= p0 (the project's rule: an empty percentile range maps the plane to 0); mode 2: u = (v / 65535 - mean) f + mean,
    pre = clip(((u - mn) / (rng + 1e-7))^gamma rng + mn, 0, 1) 65535; every other mode copies.  ``par``: the fp32 block."""
    v = np.asarray(v, dtype=np.float32).astype(dtype)
    q = np.asarray(par, dtype=np.float32).astype(dtype)
    mode = int(q[0])
    if mode == 1:
        d = q[2] - q[1]
        u = (v - q[1]) / d if d > 0 else np.zeros_like(v)
        pre = np.clip(u, 0, 1) * dtype(65535) + dtype(0.5)
    elif mode == 2:
        u = (v * (dtype(1) / dtype(65535)) - q[1]) * q[2] + q[1]
        base = (u - q[3]) / (q[4] + dtype(np.float32(1e-7)))
        w = np.power(np.maximum(base, 0), q[5]) * q[4] + q[3]
        pre = np.clip(w, 0, 1) * dtype(65535)
    else:
        return v, v
    return np.floor(pre), pre


# ---- CLAHE: bins and the interpolation between the tile mappings ---------------------------------------------------------------
def clahe_bin_coordinate(v):
    """fp64 grey-level coordinate v 16383 / 65535 + 0.5 whose floor is the grey level"""
    return np.asarray(v, dtype=np.float64) * ((GRAY - 1) / 65535.0) + 0.5


def clahe_apply(v, maps, dtype=np.float64):
    """-> (out, pre), out = floor(pre): the pixel's bin looked up in the mappings [8][8][256] of the four nearest tile centres
    and interpolated bilinearly (position in tile units relative to the centres, clamped at the outer tiles), divided by
    16383, clipped to [0, 1], times 65535"""
    v = np.asarray(v, dtype=np.float64)
    H, W = v.shape
    g = np.clip(np.floor(clahe_bin_coordinate(v)), 0, GRAY - 1).astype(np.int64)
    b = g // (GRAY // BINS)
    m = np.asarray(maps, dtype=np.float32).astype(dtype)
    yy, xx = np.mgrid[0:H, 0:W].astype(dtype)
    half, one = dtype(0.5), dtype(1)
    fy, fx = (yy + half) * dtype(TILES) / dtype(H) - half, (xx + half) * dtype(TILES) / dtype(W) - half
    ty0, tx0 = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
    ay, ax = fy - ty0.astype(dtype), fx - tx0.astype(dtype)
    ty1, tx1 = np.minimum(ty0 + 1, TILES - 1), np.minimum(tx0 + 1, TILES - 1)
    ty0, tx0 = np.maximum(ty0, 0), np.maximum(tx0, 0)
    mapped = (one - ay) * ((one - ax) * m[ty0, tx0, b] + ax * m[ty0, tx1, b]) + \
        ay * ((one - ax) * m[ty1, tx0, b] + ax * m[ty1, tx1, b])
    pre = np.clip(mapped / dtype(GRAY - 1), 0, 1) * dtype(65535)
    return np.floor(pre), pre


# ---- normalisation --------------------------------------------------------------------------------------------------------------------
def normalize_f32(v, vmin, vmax):
    """2 (clip(v, vmin, vmax) - vmin) / (vmax - vmin) - 1, every operation rounded to fp32: the bits the kernel must give"""
    v = np.asarray(v, dtype=np.float32)
    lo, hi = np.float32(vmin), np.float32(vmax)
    c = np.minimum(np.maximum(v, lo), hi)
    return (np.float32(2) * (c - lo)) / (hi - lo) - np.float32(1)


# ---- the band around a rounding boundary ------------------------------------------------------------------------------------------------
def near_integer(pre, half_width):
    """pixels whose pre-rounding value lies within ``half_width`` of an integer, where floor() may go either way"""
    pre = np.asarray(pre, dtype=np.float64)
    return np.abs(pre - np.rint(pre)) < half_width
