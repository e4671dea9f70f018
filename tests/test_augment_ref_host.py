"""CPU: the references of tests/augment_kernels_ref.py against numpy / scipy, so that tests/test_gpu_augment_kernels.py
measures the kernels against something that is itself pinned."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import augment_kernels_ref as R
from oracle import augment_ref

NP_FLIPS = [lambda a: a, lambda a: np.flip(a, 1), lambda a: np.flip(a, 0), lambda a: np.rot90(a), lambda a: np.rot90(a, 2),
            lambda a: np.rot90(a, 3), lambda a: np.rot90(np.flip(a, 1)), lambda a: np.rot90(np.flip(a, 0))]


def _noise(seed, h, w):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 65536, (h, w)).astype(np.float64)


def _smooth(seed, h, w):
    rng = np.random.Generator(np.random.PCG64(seed))
    a = ndi.gaussian_filter(rng.random((h + 16, w + 16)), 2.5)[8:-8, 8:-8]
    return np.floor((a - a.min()) / (a.max() - a.min()) * 60000 + 2000)


# ---- flips ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", range(8))
def test_flip_reference_equals_numpy(code):
    a = _noise(code, 6, 6)
    assert np.array_equal(R.flip(a, code), NP_FLIPS[code](a))
    if code in (0, 1, 2, 4):
        for shape in ((5, 12), (1, 7), (7, 1)):
            b = _noise(10 + code, *shape)
            assert np.array_equal(R.flip(b, code), NP_FLIPS[code](b))
    else:
        with pytest.raises(ValueError):
            R.flip(_noise(0, 5, 12), code)


# ---- warps ---------------------------------------------------------------------------------------------------------------------
def _scipy_warp(a, m, order):
    m = np.asarray(m, dtype=np.float32).astype(np.float64)
    return ndi.affine_transform(a, np.array([[m[4], m[3]], [m[1], m[0]]]), np.array([m[5], m[2]]), order=order,
                                mode="grid-constant", cval=0.0)


WARPS = [("rot30", lambda h, w: augment_ref.rotation_matrix(30.0, h, w)),
         ("rot-17.5", lambda h, w: augment_ref.rotation_matrix(-17.5, h, w)),
         ("rot45", lambda h, w: augment_ref.rotation_matrix(45.0, h, w)),
         ("scale1.1x0.9", lambda h, w: augment_ref.scale_matrix(1.1, 0.9, h, w)),
         ("scale0.87x1.13", lambda h, w: augment_ref.scale_matrix(0.87, 1.13, h, w)),
         ("shift-0.5", lambda h, w: (1, 0, -0.5, 0, 1, 0.5)),
         ("shift+3", lambda h, w: (1, 0, 3, 0, 1, -2)),
         ("shear", lambda h, w: (0.9317, 0.2113, 1.3729, -0.1731, 1.0719, -0.7307))]


@pytest.mark.parametrize("name,mk", WARPS, ids=[w[0] for w in WARPS])
@pytest.mark.parametrize("shape", [(17, 23), (64, 64)])
def test_bilinear_warp_reference_equals_scipy(name, mk, shape):
    a = _smooth(3, *shape)
    m = mk(*shape)
    got, want = R.affine_bilinear(a, m), _scipy_warp(a, m, 1)
    assert np.abs(got - want).max() <= 1e-9 * 65535, np.abs(got - want).max()


@pytest.mark.parametrize("name,mk", WARPS, ids=[w[0] for w in WARPS])
@pytest.mark.parametrize("shape", [(17, 23), (64, 64)])
def test_nearest_warp_reference_equals_scipy(name, mk, shape):
    if (name, shape) in R.NEAREST_ON_BOUNDARY:
        assert R.affine_nearest(_noise(4, *shape), mk(*shape))[1].mean() > 0.01
        return
    a = _noise(4, *shape)
    m = mk(*shape)
    got, unsure = R.affine_nearest(a, m)
    want = _scipy_warp(a, m, 0)
    if name.startswith("shift-0.5"):
        assert unsure.all()                       # every coordinate sits on a rounding boundary: nothing to compare
    else:
        assert unsure.mean() <= 0.01
        assert np.array_equal(got[~unsure], want[~unsure])


def test_bilinear_warp_fp32_restatement_is_close():
    a = _smooth(5, 17, 23)
    m = augment_ref.rotation_matrix(30.0, 17, 23)
    e = np.abs(R.affine_bilinear(a, m, np.float32).astype(np.float64) - R.affine_bilinear(a, m)).max()
    assert 0 < e < 0.1


# ---- blur ----------------------------------------------------------------------------------------------------------------------
SIGMAS = [1.0, 1.125, 1.375, 1.6, float(np.nextafter(np.float32(2), np.float32(0))), 1.9]


@pytest.mark.parametrize("shape", [(37, 53), (3, 5), (1, 9), (9, 1)])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_blur_reference_equals_scipy(sigma, shape):
    """also planes smaller than the radius: at 3 x 5 and sigma 1.9 the radius of 8 exceeds the period of the reflection"""
    a = _noise(6, *shape)
    s = float(np.float32(sigma))
    got, want = R.blur(a, sigma), ndi.gaussian_filter(a, s, order=0)
    assert np.abs(got - want).max() <= 1e-9, np.abs(got - want).max()
    assert R.blur_radius(sigma) == int(4.0 * s + 0.5)


def test_blur_radius_and_copy():
    assert [R.blur_radius(s) for s in SIGMAS] == [4, 5, 6, 6, 8, 8]
    a = _noise(7, 4, 6)
    assert np.array_equal(R.blur(a, 0.0), a)


def test_blur_fp32_restatement_error_is_a_small_fraction_of_a_grey_level():
    a = _noise(8, 37, 53)
    for s in (1.125, SIGMAS[4]):
        e = np.abs(R.blur(a, s, np.float32).astype(np.float64) - R.blur(a, s)).max()
        assert 0 < e < 0.05, e


# ---- statistics and percentiles -------------------------------------------------------------------------------------------------
def test_stats_reference():
    v = np.array([[0.5, 1.5, 2.49, -3.0], [70000.0, 65535.0, 65534.5, 7.0]], dtype=np.float32)
    mn, mx, mean, hist = R.stats(v)
    assert (mn, mx) == (-3.0, 70000.0) and mean == np.float32(v.astype(np.float64).mean())
    want = np.zeros(65536, np.int64)
    for b in (1, 2, 2, 0, 65535, 65535, 65535, 7):
        want[b] += 1
    assert np.array_equal(hist, want)


@pytest.mark.parametrize("q", [0.0, 0.1, 0.2, 37.5, 50.0, 99.8, 99.9, 100.0])
def test_percentile_reference_equals_numpy(q):
    rng = np.random.Generator(np.random.PCG64(9))
    for v in (rng.integers(0, 65536, 1), rng.integers(0, 65536, 2), rng.integers(0, 65536, 97 * 131),
              rng.integers(0, 4, 500) * 1000, np.array([255, 255, 256, 256])):
        want = np.percentile(v.astype(np.float64), float(np.float32(q)))
        assert abs(R.percentile(v, q) - want) <= 1e-9 * max(1.0, abs(want))


# ---- contrast ---------------------------------------------------------------------------------------------------------------------
def test_contrast_reference_equals_the_sample_pipeline_formulas():
    """the same two formulas as oracle/augment_ref.augment_sample (mytransforms.py:96-122), from parameters in fp64"""
    v = _smooth(11, 24, 40)
    p0, p1 = np.percentile(v, (0.2, 99.8))
    out, pre = R.contrast(v, [1, p0, p1, 0, 0, 0, 0, 0])
    want = np.round(np.clip((v - np.float32(p0)) / (np.float64(np.float32(p1)) - np.float32(p0)), 0, 1) * 65535)
    assert np.abs(out - want).max() <= 1 and (out != want).mean() < 0.01       # round half to even against floor(x + 0.5)
    assert np.array_equal(R.contrast(v, [1, 500.0, 500.0])[0], np.zeros_like(v))
    assert np.array_equal(R.contrast(v, [1, 600.0, 500.0])[0], np.zeros_like(v))
    st = (v.min(), v.max(), v.mean())
    par = R.contrast_params_mode2(st, 1.2, 0.8)
    u = v / 65535.0
    u = (u - u.mean()) * 1.2 + u.mean()
    assert abs(par[3] - u.min()) <= 1e-6 and abs(par[4] - (u.max() - u.min())) <= 1e-6
    out, _ = R.contrast(v, par.astype(np.float32))
    mn, rg = u.min(), u.max() - u.min()
    want = np.floor(np.clip(np.power((u - mn) / float(rg + 1e-7), 0.8) * rg + mn, 0, 1) * 65535)
    assert np.abs(out - want).max() <= 8                                         # fp32 mean / min / range in the block
    for mode in (0, 3):
        assert np.array_equal(R.contrast(v, [mode, 1, 2])[0], v)


def test_clahe_apply_reference_equals_the_oracle():
    """clahe_apply on the oracle's maps against the oracle's own (mixed fp32 / fp64) interpolation: within one grey level,
    equal away from the rounding boundary, in either precision"""
    v = _smooth(12, 24, 40)
    maps, _ = augment_ref.clahe_maps(v)
    want = augment_ref.clahe(v)
    out64, pre = R.clahe_apply(v, maps)
    sure = ~R.near_integer(pre, 0.05)
    assert sure.mean() > 0.5        # 3 x 5-pixel tiles: the mappings are multiples of 16383 / 15, many values land on integers
    for out in (out64, R.clahe_apply(v, maps, np.float32)[0]):
        assert np.abs(out - want).max() <= 1
        assert np.array_equal(out[sure], want[sure])


def test_normalize_reference():
    v = np.array([-5.0, 0.0, 10000.0, 22500.0, 35000.0, 65535.0, 70000.0], dtype=np.float32)
    assert R.normalize_f32(v, 0, 65535).tolist() == [-1.0, -1.0] + \
        [float(np.float32(np.float32(2 * x) / np.float32(65535)) - np.float32(1)) for x in (10000.0, 22500.0, 35000.0)] + [1.0, 1.0]
    assert R.normalize_f32(v, 10000, 35000).tolist() == [-1.0, -1.0, -1.0, 0.0, 1.0, 1.0, 1.0]
    assert R.normalize_f32(v, 0, 65535).dtype == np.float32
