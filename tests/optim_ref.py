"""Plain fp64 references of the optimizer kernels of libmseg_hip (mseg_adam_amsgrad_step, mseg_adam_amsgrad_step_dev,
mseg_ranger_step, mseg_ranger_step_multi) and of mseg_bn_eval_coeffs, written from the formulas in include/mseg_hip.h
alone (numpy; nothing is imported from the package under test), each WITH THE ERROR BOUND of its fp32 evaluation.

Scalars.  The hyper-parameters arrive as doubles and are rounded to fp32 ONCE, as the header says: w1 = f32(1 - beta1),
beta2 = f32(beta2), w2 = f32(1 - beta2), eps = f32(eps); Adam: step_size = f32(lr / (1 - beta1^step)) and bc2_sqrt =
f32(sqrt(1 - beta2^step)), both evaluated in double; Ranger: also beta1, step_lr and alpha as fp32.  The references use
exactly these fp32 values, widened to fp64 (adam_scalars / ranger_scalars; rounded = False keeps the doubles, which is
what torch's own fp64 optimizers compute with: tests/test_optim_ref_host.py pins the formulas to them that way).

Return value.  Every function returns ``{name: (value, bound)}`` per element, in the spirit of conv_ref's (result, S).
The bound is the first-order forward propagation of one unit roundoff u = 2^-24 per fp32 operation of the header's
formula (a fused multiply-add rounds less, never more), plus A = 2^-140 absolute for results in fp32's subnormal range
(spacing 2^-149).  The bounds are conditions derived from the formulas, not measurements.

Adam (amsgrad), torch.optim.Adam semantics:
    m'    = m + (g - m) w1                       dm    = 3u (|m| + w1 |g - m|)       subtract, multiply, add
    v'    = v beta2 + w2 g g                     dv    = 4u v'                       every term is >= 0: at most 3
    vmax' = max(vmax, v')                        dvmax = 4u vmax'                      roundings on a term, 1 on the sum
    d     = sqrt(vmax') / bc2_sqrt + eps
    p'    = p - step_size m' / d                 dp    = u |p'| + step_size (dm / d + 10u |m'| / d)
  The 10u: d carries 2u (half of vmax's 4u) + u (sqrt) + u (divide) + u (add), the quotient m' / d one more, the product
  with step_size one more = 7u, and 3u of room for the second-order terms.

Ranger (RAdam + lookahead + gradient centralisation), one tensor; rows > 0: centralisation over rows of n / rows columns:
    mean = f32(sum_row g / cols)                 the sum in fp64 (its own error, ~cols 2^-53, is far below u)
    gi   = g - mean                              dgi   = u |mean| + u |gi|           rounding of the mean, subtraction
    v'   = v beta2 + w2 gi gi                    dv    = 4u v' + 2 w2 |gi| dgi
    m'   = m beta1 + w1 gi                       dm    = 2u (|m| beta1 + w1 |gi|) + w1 dgi
    s    = sqrt(v')                              ds    = min(sqrt(dv), dv / s) + u s
  |sqrt(a) - sqrt(b)| <= |a - b| / max(sqrt(a), sqrt(b)) and <= sqrt(|a - b|): the second covers v' = 0, where the
  first divides by zero (first order would be dv / 2s: the factor 2 is slack).
    d    = s + eps                               dd    = ds + u d
    upd  = m' / d    (rectified)                 dupd  = dm / d + |m'| dd / d^2 + u |upd|
    upd  = m'        (not rectified)             dupd  = dm
    p'   = p - step_lr upd                       dp    = step_lr dupd + u step_lr |upd| + u |p'|
  with the lookahead blend
    t    = p' - slow                             dt    = dp + u |t|
    a    = alpha t                               da    = alpha dt + u |a|
    slow'= slow + a;  p' = slow'                 dslow = da + u |slow'|
  Without the blend slow must come back bit-unchanged (bound 0).

mseg_bn_eval_coeffs:
    t     = rv + eps                             u t
    inv   = 1 / sqrt(t)                          u/2 (from t) + u (sqrt) + u (divide) = 2.5u relative
    scale = gamma inv                            dscale = 3.5u |scale|
    shift = beta - rm scale                      dshift = |rm| dscale + u |rm scale| + u |shift|
  gamma or beta may be None (1 and 0).

The planted inputs of the tests (adam_inputs, ranger_inputs) live here too so that the host test proves the references
stay inside their own bounds on exactly the values the GPU test uses."""
import numpy as np

U = 2.0 ** -24
A = 2.0 ** -140


def f32(x):
    """a double rounded to fp32 once, as a double"""
    return float(np.float32(x))


def _w(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, beta1, beta2, eps, step, rounded=True):
    r = f32 if rounded else float
    bc1 = 1.0 - float(beta1) ** float(step)
    bc2 = 1.0 - float(beta2) ** float(step)
    return dict(w1=r(1.0 - beta1), beta2=r(beta2), w2=r(1.0 - beta2), eps=r(eps), step_size=r(lr / bc1),
                bc2_sqrt=r(np.sqrt(bc2)), rounded=rounded)


def adam_step(p, g, m, v, vmax, sc):
    """one update of n elements; sc = adam_scalars(...) (or the same dict with step_size / bc2_sqrt as read back from the
    device form's state) -> {'p' | 'm' | 'v' | 'vmax': (value, bound)}"""
    if sc["rounded"]:
        p, g, m, v, vmax = _w(p), _w(g), _w(m), _w(v), _w(vmax)
    else:                                   # unrounded scalars: the fp64 pin, operands as they come
        p, g, m, v, vmax = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v, vmax))
    w1, beta2, w2, eps, ss, bc = (sc[k] for k in ("w1", "beta2", "w2", "eps", "step_size", "bc2_sqrt"))
    m1 = m + (g - m) * w1
    v1 = v * beta2 + w2 * g * g
    x1 = np.maximum(vmax, v1)
    d = np.sqrt(x1) / bc + eps
    p1 = p - ss * m1 / d
    dm = 3 * U * (np.abs(m) + w1 * np.abs(g - m)) + A
    dv = 4 * U * v1 + A
    dx = 4 * U * x1 + A
    dp = U * np.abs(p1) + ss * (dm / d + 10 * U * np.abs(m1) / d) + A
    return {"p": (p1, dp), "m": (m1, dm), "v": (v1, dv), "vmax": (x1, dx)}


# ---- Ranger -------------------------------------------------------------------------------------------------------------------
def ranger_scalars(beta1, beta2, eps, step_lr, alpha, rounded=True):
    r = f32 if rounded else float
    return dict(beta1=r(beta1), w1=r(1.0 - beta1), beta2=r(beta2), w2=r(1.0 - beta2), eps=r(eps), step_lr=r(step_lr),
                alpha=r(alpha), rounded=rounded)


def ranger_step(p, g, m, v, slow, rows, sc, rectified, lookahead):
    """one update of one tensor of n elements; rows > 0: gradient centralisation over rows of n / rows columns, rows = 0: none
    -> {'p' | 'm' | 'v' | 'slow': (value, bound)}"""
    if sc["rounded"]:
        p, g, m, v, slow = _w(p), _w(g), _w(m), _w(v), _w(slow)
    else:
        p, g, m, v, slow = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v, slow))
    n = g.size
    b1, w1, b2, w2, eps, lr, alpha = (sc[k] for k in ("beta1", "w1", "beta2", "w2", "eps", "step_lr", "alpha"))
    if rows > 0:
        assert n % rows == 0
        mean = g.reshape(rows, n // rows).sum(axis=1) / (n // rows)
        if sc["rounded"]:
            mean = _w(mean)
        mean = np.repeat(mean, n // rows)
    else:
        mean = np.zeros(n)
    gi = g - mean
    dgi = U * np.abs(mean) + U * np.abs(gi) if rows > 0 else np.zeros(n)
    v1 = v * b2 + w2 * gi * gi
    dv = 4 * U * v1 + 2 * w2 * np.abs(gi) * dgi + A
    m1 = m * b1 + w1 * gi
    dm = 2 * U * (np.abs(m) * b1 + w1 * np.abs(gi)) + w1 * dgi + A
    if rectified:
        s = np.sqrt(v1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ds = np.minimum(np.sqrt(dv), np.where(s > 0, dv / s, np.inf)) + U * s
        d = s + eps
        dd = ds + U * d
        upd = m1 / d
        dupd = dm / d + np.abs(m1) * dd / (d * d) + U * np.abs(upd)
    else:
        upd, dupd = m1, dm
    p1 = p - lr * upd
    dp = lr * dupd + U * lr * np.abs(upd) + U * np.abs(p1) + A
    if lookahead:
        t = p1 - slow
        dt = dp + U * np.abs(t)
        a = alpha * t
        da = alpha * dt + U * np.abs(a)
        s1 = slow + a
        ds1 = da + U * np.abs(s1) + A
        return {"p": (s1, ds1), "m": (m1, dm), "v": (v1, dv), "slow": (s1, ds1)}
    return {"p": (p1, dp), "m": (m1, dm), "v": (v1, dv), "slow": (slow, np.zeros(n))}


# ---- eval-mode BatchNorm coefficients -----------------------------------------------------------------------------------------
def bn_eval_coeffs(gamma, beta, rm, rv, eps):
    """-> {'scale' | 'shift': (value, bound)} per channel; gamma / beta may be None"""
    rm, rv = _w(rm), _w(rv)
    ga = np.ones_like(rv) if gamma is None else _w(gamma)
    be = np.zeros_like(rv) if beta is None else _w(beta)
    inv = 1.0 / np.sqrt(rv + f32(eps))
    scale = ga * inv
    shift = be - rm * scale
    dscale = 3.5 * U * np.abs(scale) + A
    dshift = np.abs(rm) * dscale + U * np.abs(rm * scale) + U * np.abs(shift) + A
    return {"scale": (scale, dscale), "shift": (shift, dshift)}


# ---- the inputs of the tests --------------------------------------------------------------------------------------------------
# planted (g, m, v, vmax): zero state; momentum alone over d = eps; g g in fp32's subnormal range (+-1e-20: 1e-40, inexact)
# and below it (+-1e-30: g g underflows to 0 in fp32); g g near 2^120; vmax equal to, half of and twice v (with g^2 > v the
# equal one is replaced, with g^2 < v it is kept)
BIG = 2.0 ** 60
# The first and the last tuple land on the first and the last element of a tensor: both change every array, so an element
# that a kernel skips there shows (the all-zero tuple would hide it: its update is the identity).
ADAM_PLANTS = [(0.5, 0.1, 0.04, 0.04), (0, 0, 0, 0), (0, 1, 0, 0), (1e-20, 0, 0, 0), (-1e-20, 0, 0, 0), (BIG, 0, 0, 0),
               (-BIG, 0, 0, 0), (1e-30, 0, 0, 0), (-1e-30, 0, 0, 0),
               (0.1, -0.1, 0.04, 0.04), (0.5, 0.1, 0.04, 0.02), (0.1, 0.1, 0.04, 0.02),
               (0.5, -0.1, 0.04, 0.08), (0.1, 0.1, 0.04, 0.08)]
RANGER_PLANTS = [(BIG, 0, 0), (0, 0, 0), (0, 1, 0), (1e-20, 0, 0), (-1e-20, 0, 0), (1e-30, 0, 0), (-1e-30, 0, 0), (-BIG, 0, 0)]

# the shapes of the Ranger tests: (rows, cols) with centralisation — one row, a row shorter than a wavefront, rows of 72
# (a 3x3 weight of 8 channels), ONE column (gi == 0 everywhere), rows longer than a workgroup pass, many rows — and element
# counts without it, around the 4096 elements a workgroup takes
GC_SHAPES = [(1, 64), (5, 12), (16, 72), (3, 1), (2, 9216), (256, 300)]
NOGC_SIZES = [1, 4095, 4096, 4097, 9000]


def _spread(rng, n, lo, hi, signed=True):
    x = 10.0 ** rng.uniform(lo, hi, size=n)
    if signed:
        x *= rng.choice([-1.0, 1.0], size=n)
    return x.astype(np.float32)


def plant_positions(n, k, seed):
    """where plant j goes: spread evenly from the first to the last element (the vector body and the scalar tail both get
    some); a tensor shorter than the list takes a window of it that moves with the seed"""
    if n >= k:
        return np.linspace(0, n - 1, k).astype(np.int64), np.arange(k)
    return np.arange(n), (np.arange(n) + seed) % k


def adam_inputs(n, seed, zero_state=False):
    """-> p, g, m, v, vmax (fp32): magnitudes spread over 1e-6 .. 1e2 (g, m) and 1e-12 .. 1e6 (v), vmax = v x {1/2, 1, 2},
    the planted tuples on top.  zero_state: the state of a first step, all zeros (no plants in the state)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = rng.normal(size=n).astype(np.float32)
    g, m = _spread(rng, n, -6, 2), _spread(rng, n, -6, 2)
    v = _spread(rng, n, -12, 6, signed=False)
    vmax = (v * rng.choice([0.5, 1.0, 2.0], size=n)).astype(np.float32)
    pos, which = plant_positions(n, len(ADAM_PLANTS), seed)
    P = np.array(ADAM_PLANTS, dtype=np.float32)[which]
    g[pos], m[pos], v[pos], vmax[pos] = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    if zero_state:
        m[:], v[:], vmax[:] = 0, 0, 0
    return p, g, m, v, vmax


def ranger_inputs(n, seed, plants=True, offset=0.0):
    """-> p, g, m, v, slow (fp32); offset is added to every gradient (cancellation against the row mean)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = rng.normal(size=n).astype(np.float32)
    slow = (p + 0.1 * rng.normal(size=n)).astype(np.float32)
    g, m = _spread(rng, n, -6, 2), _spread(rng, n, -6, 2)
    v = _spread(rng, n, -12, 6, signed=False)
    if plants:
        pos, which = plant_positions(n, len(RANGER_PLANTS), seed)
        P = np.array(RANGER_PLANTS, dtype=np.float32)[which]
        g[pos], m[pos], v[pos] = P[:, 0], P[:, 1], P[:, 2]
    if offset:
        g = (g + np.float32(offset)).astype(np.float32)
    return p, g, m, v, slow


def ranger_exact_inputs(n, rows, seed):
    """Small integers whose every intermediate is exact in fp32 under beta1 = 0.5, beta2 = 0.75, step_lr = 2^-3, alpha =
    0.5, not rectified.  rows > 0: cols must be a power of two; a row's first columns get +1 until the row sum is a
    multiple of cols (the mean is an integer; every |g| stays below 12).  -> p, g, m, v, slow"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = rng.integers(-8, 9, size=n).astype(np.int64)
    if rows > 0:
        cols = n // rows
        assert rows * cols == n and cols & (cols - 1) == 0
        G = g.reshape(rows, cols)
        G += np.arange(cols)[None, :] < ((-G.sum(axis=1)) % cols)[:, None]      # +1 on the first (-sum mod cols) columns
        G += rng.integers(-2, 3, size=(rows, 1))                                 # a mean that is not 0
        assert not (G.sum(axis=1) % cols).any()
        g = G.reshape(-1)
    ints = lambda: rng.integers(-8, 9, size=n).astype(np.float32)
    return ints(), g.astype(np.float32), ints(), np.abs(ints()), ints()


def bn_inputs(C, seed):
    """running_var 0, 2^-30, 1 and 1e6 planted among random values (as many as fit)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    gamma, beta, rm = (rng.normal(size=C).astype(np.float32) for _ in range(3))
    rv = (10.0 ** rng.uniform(-4, 2, size=C)).astype(np.float32)
    plants = np.array([0.0, 2.0 ** -30, 1.0, 1e6], dtype=np.float32)
    pos, which = plant_positions(C, 4, seed)
    rv[pos] = plants[which]
    return gamma, beta, rm, rv
