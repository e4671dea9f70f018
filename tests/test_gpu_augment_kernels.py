"""GPU (MI355X): the nine entry points of csrc/augment.hip through the C ABI, each against the reference of
tests/augment_kernels_ref.py (which tests/test_augment_ref_host.py pins to numpy / scipy on the CPU).

Every batch has N >= 3 samples with different content and different parameters, so a kernel that reads sample 0's
parameters fails.  Outputs are pre-filled with NaN and carry a NaN guard band that must come back untouched.

Bounds.  Exact operations (conversion, flips, copies, integer and half-pixel translations, min / max, histogram, the
normalisation) are compared bit for bit.  Smooth quantities q follow e_hip <= max(4 e_ref, 4 ulp_fp32(max|ref|)) under
max|q - fp64|, where e_ref is the error of the fp32 restatement of the same formula on the CPU — never the kernel's own; the
blur's bound is capped at 0.2 grey levels on top (a radius that is one too small costs 1.7).  Quantities that are rounded to
a grey level at the end (contrast, CLAHE) must be within one grey level everywhere and equal outside a band around the
rounding boundary of the fp64 pre-rounding value; band and banded share are computed from the references alone.  The noise
generator is tested statistically with five-standard-error bounds; a numpy run of the intended algorithm over four seeds
stayed below 2.4 standard errors in every statistic.

Measured on the MI355X (first run), e_ref / e_hip: blur 0.0096-0.0151 / 0.0101-0.0135 grey levels at 37 x 53 (worst pair
sigma 1.6: 0.0096 / 0.0135 of 0.038 allowed); bilinear 0.007-0.163 / 0.006-0.163; mode-2 parameters 1.3e-8-1.2e-7 / the same;
percentiles <= 1.9e-3; nearest: nothing excluded, nothing different; contrast: <= 0.5 % of the pixels one level off, all in the
band; CLAHE: mappings bit-equal, <= 6.4 % one off in the band; noise: every statistic below 2.7 of its standard errors.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi
from scipy import special

import augment_kernels_ref as R
from oracle import augment_ref

pytestmark = pytest.mark.gpu

GUARD = 64
EINVAL = -1
NAN = float("nan")
SHAPES = [(17, 23), (64, 64)]
GOLDEN = 2654435761                        # the multiplier of the pixel index in the noise generator's key


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from microbeseg_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))               # a copy: cached planes are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def _nan_buf(n, dtype=torch.float32):
    return torch.full((n + GUARD,), NAN, dtype=dtype, device="cuda")


def _take(buf, n, shape=None):
    """-> the n output elements (fp32 numpy), after checking that the guard band still holds its NaNs and nothing was left out"""
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.isnan(host[n:]).all(), "the kernel wrote behind its output"
    assert not np.isnan(host[:n]).any(), "an output element was left unwritten"
    return host[:n] if shape is None else host[:n].reshape(shape)


def _ok(code):
    assert code == 0, f"libmseg_hip returned {code}"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what=""):
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {bad[0]}: " \
                          f"{got.ravel()[bad[0]]!r} != {np.asarray(want, np.float32).ravel()[bad[0]]!r}"


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _smooth_bound(got, ref32, ref64, what, cap=None):
    ref64 = np.asarray(ref64, dtype=np.float64)
    e_ref = float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max())
    e_hip = float(np.abs(np.asarray(got, dtype=np.float64) - ref64).max())
    bound = max(4 * e_ref, 4 * _ulp(np.abs(ref64).max()))
    if cap is not None:
        bound = min(bound, cap)
    print(f"    {what}: e_ref {e_ref:.3e} e_hip {e_hip:.3e} bound {bound:.3e}")
    assert e_hip <= bound, f"{what}: e_hip {e_hip:.3e} > {bound:.3e} (e_ref {e_ref:.3e})"


def _noise_planes(seed, n, h, w):
    """uint16 noise as fp32, every sample different"""
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 65536, (n, h, w)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _smooth_planes(seed, n, h, w):
    """smooth integer-valued planes in 2000 .. 62000, every sample different"""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = ndi.gaussian_filter(rng.random((n, h + 16, w + 16)), (0, 2.5, 2.5))[:, 8:-8, 8:-8]
    lo, hi = a.min(axis=(1, 2), keepdims=True), a.max(axis=(1, 2), keepdims=True)
    out = np.floor((a - lo) / (hi - lo) * 60000 + 2000).astype(np.float32)
    out.setflags(write=False)
    return out


# =================================================================================================================================
# uint16 -> fp32
# =================================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_u16_to_f32_bit_exact(lib, n):
    v = np.random.Generator(np.random.PCG64(n)).integers(0, 65536, n).astype(np.uint16)
    plant = [65535, 32768, 0]
    v[:min(n, 3)] = plant[:min(n, 3)]
    if n > 6:
        v[-3:] = plant
    src = torch.from_numpy(v.view(np.int16)).cuda()                # the int16 view the loader delivers
    out = _nan_buf(n)
    _ok(lib.mseg_aug_u16_to_f32(src.data_ptr(), out.data_ptr(), n, _stream()))
    _same_bits(_take(out, n), R.u16_to_f32(v), "u16_to_f32")


# =================================================================================================================================
# flips
# =================================================================================================================================
def _run_flip(lib, planes, codes):
    n, h, w = planes.shape
    src, cd, out = _dev(planes), _dev(np.asarray(codes, np.int32)), _nan_buf(planes.size)
    _ok(lib.mseg_aug_flip(src.data_ptr(), out.data_ptr(), n, h, w, cd.data_ptr(), _stream()))
    return _take(out, planes.size, planes.shape)


def test_flip_all_codes_square(lib):
    planes = _noise_planes(1, 8, 48, 48)
    got = _run_flip(lib, planes, np.arange(8)[::-1])               # sample s gets code 7 - s
    for s in range(8):
        _same_bits(got[s], R.flip(planes[s], 7 - s), f"code {7 - s}")


@pytest.mark.parametrize("shape", [(5, 12), (1, 7), (7, 1)])
def test_flip_non_square(lib, shape):
    codes = [4, 2, 0, 1]
    planes = _noise_planes(2, 4, *shape)
    got = _run_flip(lib, planes, codes)
    for s, c in enumerate(codes):
        _same_bits(got[s], R.flip(planes[s], c), f"code {c}")


def test_flip_argument_checks(lib):
    buf = _nan_buf(3 * 6 * 6)
    cd = _dev(np.zeros(3, np.int32))
    assert lib.mseg_aug_flip(buf.data_ptr(), buf.data_ptr(), 3, 6, 6, cd.data_ptr(), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


def test_device_augment_refuses_transposing_flips_of_non_square_crops(lib):
    """host path only: DeviceAugment.apply raises before it allocates or launches anything"""
    from microbeseg_amd.training import device_augment
    da = device_augment.DeviceAugment("distance", 0, 65535, seed=3)
    p = device_augment.draw_parameters(2)
    for code in (3, 4, 5, 6, 7):
        p["flip"][:] = (0, code)
        with pytest.raises(RuntimeError, match="square"):
            da.apply(torch.zeros((2, 5, 12), dtype=torch.int16), [], p)


# =================================================================================================================================
# affine warps
# =================================================================================================================================
def _run_affine(lib, planes, mats, apply, nearest):
    n, h, w = planes.shape
    src, md, ad = _dev(planes), _dev(np.asarray(mats, np.float32)), _dev(np.asarray(apply, np.int32))
    out = _nan_buf(planes.size)
    _ok(lib.mseg_aug_affine(src.data_ptr(), out.data_ptr(), n, h, w, md.data_ptr(), ad.data_ptr(), nearest, _stream()))
    return _take(out, planes.size, planes.shape)


def _shift(tx, ty):
    return (1, 0, tx, 0, 1, ty)


INTEGER_WARPS = [_shift(0, 0), _shift(3, 0), _shift(-2, 0), _shift(0, 4), _shift(0, -1), _shift(-5, 2)]
HALF_WARPS = [_shift(0.5, 0), _shift(-0.5, 0), _shift(0, -0.5), _shift(1.5, 0.5), _shift(-0.5, -0.5), _shift(0, 2.5)]


@pytest.mark.parametrize("shape", SHAPES)
def test_affine_exact_cases(lib, shape):
    """identity, the apply = 0 copy (beside a matrix that would move everything), integer translations in the four directions
    with zero fill, half-pixel translations — sx in (-1, 0) at the left / top edge, where truncation instead of floor would
    blend the wrong pair — bit for bit, bilinear; the integer ones also nearest, with no pixel excluded"""
    h, w = shape
    planes = _noise_planes(3, 7, h, w)
    mats = INTEGER_WARPS + [(0.3, 2.0, 5.0, -1.0, 0.2, 3.0)]
    apply = [1] * 6 + [0]
    for nearest in (0, 1):
        got = _run_affine(lib, planes, mats, apply, nearest)
        for s in range(6):
            if nearest:
                ref, unsure = R.affine_nearest(planes[s], mats[s])
                assert not unsure.any()
            else:
                ref = R.affine_bilinear(planes[s], mats[s])
            _same_bits(got[s], ref, f"nearest {nearest} matrix {mats[s]}")
        _same_bits(got[6], planes[6], "apply = 0")
        tx, ty = 3, 0
        assert (got[1][:, w - tx:] == 0).all() and np.array_equal(got[1][:, :w - tx], planes[1][:, tx:])
    got = _run_affine(lib, planes[:6], HALF_WARPS, [1] * 6, 0)
    for s in range(6):
        ref = R.affine_bilinear(planes[s], HALF_WARPS[s])
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
        _same_bits(got[s], ref, f"matrix {HALF_WARPS[s]}")
    assert np.array_equal(got[1][:, 0], planes[1][:, 0] * 0.5)     # sx = -0.5: half of the zero border, half of column 0


def _named_warps(shape):
    from microbeseg_amd.training.device_augment import rotation_matrices, scale_matrices
    h, w = shape
    rot = rotation_matrices(np.array([30.0, -17.5, 45.0], np.float32), h, w)
    sc = scale_matrices(np.array([(1.1, 0.9), (0.87, 1.13)], np.float32), h, w)
    names = ["rot30", "rot-17.5", "rot45", "scale1.1x0.9", "scale0.87x1.13"]
    return names, np.concatenate([rot, sc]).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
def test_affine_bilinear_smooth(lib, shape):
    """rotations and scalings from rotation_matrices / scale_matrices on smooth planes, whole plane, border included"""
    names, mats = _named_warps(shape)
    planes = _smooth_planes(4, len(names), *shape)
    got = _run_affine(lib, planes, mats, [1] * len(names), 0)
    for s, name in enumerate(names):
        _smooth_bound(got[s], R.affine_bilinear(planes[s], mats[s], np.float32), R.affine_bilinear(planes[s], mats[s]),
                      f"bilinear {shape} {name}")


@pytest.mark.parametrize("shape", SHAPES)
def test_affine_nearest(lib, shape):
    """reference index floor(s + 0.5) in fp64 from the same fp32 matrix; a pixel is excluded only within 1e-4 px of a rounding
    boundary (<= 1 % of a plane, from the reference alone); elsewhere equal, and every value is an input value or the fill"""
    names, mats = _named_warps(shape)
    keep = [i for i, nm in enumerate(names) if (nm, shape) not in R.NEAREST_ON_BOUNDARY]
    assert len(keep) >= 3
    names, mats = [names[i] for i in keep], mats[keep]
    planes = _noise_planes(5, len(names), *shape)
    got = _run_affine(lib, planes, mats, [1] * len(names), 1)
    for s, name in enumerate(names):
        ref, unsure = R.affine_nearest(planes[s], mats[s])
        share = unsure.mean()
        print(f"    nearest {shape} {name}: excluded {share:.4f}, differing there {(got[s] != ref)[unsure].sum()}")
        assert share <= 0.01
        assert np.array_equal(got[s][~unsure], ref[~unsure].astype(np.float32)), name
        assert np.isin(got[s], np.append(planes[s].ravel(), 0)).all()


# =================================================================================================================================
# blur
# =================================================================================================================================
BLUR_SIGMAS = np.array([1.0, 1.125, 1.375, 1.6, np.nextafter(np.float32(2), np.float32(0)), 0.0], dtype=np.float32)


@pytest.mark.parametrize("shape", [(37, 53), (3, 5), (1, 9), (9, 1)])
def test_blur(lib, shape):
    """uint16 noise, one sigma per sample (radii 4, 5, 6, 6, 8; 0 copies); the small planes are shorter than the radius, 3 x 5 at
    sigma just below 2 shorter than half of it (the reflection is periodic)"""
    h, w = shape
    n = len(BLUR_SIGMAS)
    planes = _noise_planes(6, n, h, w)
    src, sig = _dev(planes), _dev(BLUR_SIGMAS)
    tmp, out = _nan_buf(planes.size), _nan_buf(planes.size)
    _ok(lib.mseg_aug_blur(src.data_ptr(), tmp.data_ptr(), out.data_ptr(), n, h, w, sig.data_ptr(), _stream()))
    got = _take(out, planes.size, planes.shape)
    _take(tmp, planes.size)
    for s, sigma in enumerate(BLUR_SIGMAS):
        if sigma > 0:
            _smooth_bound(got[s], R.blur(planes[s], sigma, np.float32), R.blur(planes[s], sigma),
                          f"blur {shape} sigma {float(sigma):.7f}", cap=0.2)
        else:
            _same_bits(got[s], planes[s], "sigma = 0")


def test_blur_argument_checks(lib):
    a, b = _nan_buf(3 * 5 * 5), _nan_buf(3 * 5 * 5)
    sig = _dev(np.ones(3, np.float32))
    assert lib.mseg_aug_blur(a.data_ptr(), a.data_ptr(), b.data_ptr(), 3, 5, 5, sig.data_ptr(), _stream()) == EINVAL
    assert lib.mseg_aug_blur(a.data_ptr(), b.data_ptr(), b.data_ptr(), 3, 5, 5, sig.data_ptr(), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(a).all() and torch.isnan(b).all()


# =================================================================================================================================
# statistics
# =================================================================================================================================
def _run_stats(lib, planes, with_hist):
    n, h, w = planes.shape
    src, st = _dev(planes), _nan_buf(3 * n)
    hist = torch.full((n * 65536 + GUARD,), -1, dtype=torch.int32, device="cuda")          # 0xFF bytes
    _ok(lib.mseg_aug_stats(src.data_ptr(), n, h, w, st.data_ptr(), hist.data_ptr() if with_hist else None, _stream()))
    stats = _take(st, 3 * n, (n, 3))
    hh = hist.cpu().numpy()
    assert (hh[n * 65536:] == -1).all(), "the kernel wrote behind the histogram"
    return stats, hh[:n * 65536].reshape(n, 65536)


@pytest.mark.parametrize("shape", [(1, 1), (1, 255), (16, 16), (257, 1), (97, 131)])
def test_stats_and_histogram(lib, shape):
    h, w = shape
    rng = np.random.Generator(np.random.PCG64(7 + h * w))
    ints = rng.integers(0, 65536, (3, h, w)).astype(np.float32)
    ints[1] = rng.integers(300, 340, (h, w))                         # heavy ties
    frac = (rng.integers(0, 65536 * 8, (3, h, w)) / 8).astype(np.float32)               # the grid k / 8: k + 0.5 among them
    if h * w >= 255:
        for s in range(3):
            frac[s].flat[[0, 1, 2, 3, h * w - 1]] = (7.5 + s, 65534.5, -3.25 - s, 65535.75 + 100 * s, 12.5)
    for name, planes in (("integer", ints), ("k / 8", frac)):
        stats, hist = _run_stats(lib, planes, True)
        for s in range(3):
            mn, mx, mean, hh = R.stats(planes[s])
            assert stats[s, 0] == mn and stats[s, 1] == mx, (name, s)
            if name == "integer":
                assert stats[s, 2] == mean, (name, s, stats[s, 2], mean)
            else:
                assert abs(float(stats[s, 2]) - float(mean)) <= _ulp(mean), (name, s, stats[s, 2], mean)
            assert np.array_equal(hist[s], hh), (name, s)
        stats2, hist2 = _run_stats(lib, planes, False)               # hist == NULL: same statistics, the buffer untouched
        assert np.array_equal(_bits(stats2), _bits(stats)) and (hist2 == -1).all()


# =================================================================================================================================
# contrast parameters
# =================================================================================================================================
PCT_BOUND = 2 * 2.0 ** -7          # "2 ulp of 65535", 0.0156: three fp32 roundings of magnitudes <= 65535


def _percentile_planes():
    """name -> integer planes [3][HW], every sample different"""
    rng = np.random.Generator(np.random.PCG64(8))
    smooth = _smooth_planes(9, 3, 97, 131).reshape(3, -1).astype(np.int64)
    ties = rng.integers(0, 4, (3, 500)) * np.array([[1000], [700], [16384]])               # a few values, empty chunks between
    top = rng.integers(65280, 65536, (3, 300))                                               # all mass in the last chunk
    top[:, :5] = 65535
    top[1, :] = 65535
    straddle = np.array([[255, 255, 256, 256], [255, 256, 256, 256], [0, 255, 256, 65535]])  # order statistics across a chunk edge
    one = np.array([[0], [65535], [256]])
    two = np.array([[255, 256], [65535, 0], [511, 512]])
    return {"smooth": smooth, "ties": ties, "last-chunk": top, "straddle": straddle, "hw1": one, "hw2": two}


PCT_Q = [[(0.2, 99.8), (0.1, 99.9), (37.5, 50.0)], [(0.0, 100.0), (25.0, 75.0), (50.0, 62.5)],
         [(99.9, 100.0), (0.0, 0.1), (33.0, 67.0)]]


@pytest.mark.parametrize("name", ["smooth", "ties", "last-chunk", "straddle", "hw1", "hw2"])
def test_contrast_params_percentiles(lib, name):
    """mode 1 against np.percentile of the same integers (q = the fp32 number): q = 0 and 100 are the minimum and the maximum"""
    v = _percentile_planes()[name]
    n, hw = v.shape
    hist = np.stack([np.bincount(v[s], minlength=65536) for s in range(n)]).astype(np.int32)
    hd, st = _dev(hist), _dev(np.zeros((n, 3), np.float32))
    for qs in PCT_Q:
        choice = np.array([(1, a, b, 0) for a, b in qs], dtype=np.float32)
        par = torch.zeros(8 * n + GUARD, device="cuda")
        par[8 * n:] = NAN
        cd = _dev(choice)
        _ok(lib.mseg_aug_contrast_params(st.data_ptr(), hd.data_ptr(), cd.data_ptr(), n, hw, par.data_ptr(),
                                         _stream()))
        got = _take(par, 8 * n, (n, 8))
        for s, (a, b) in enumerate(qs):
            want = [np.percentile(v[s].astype(np.float64), float(np.float32(q))) for q in (a, b)]
            assert [R.percentile(v[s], q) for q in (a, b)] == pytest.approx(want, abs=1e-9)
            err = [abs(float(got[s, 1 + e]) - want[e]) for e in range(2)]
            print(f"    percentiles {name} q {(a, b)}: got {got[s, 1:3]} want {want} err {max(err):.2e}")
            assert got[s, 0] == 1 and max(err) <= PCT_BOUND, (name, s, got[s], want)
            assert (got[s, 3:] == 0).all()
            if a == 0.0:
                assert got[s, 1] == v[s].min()
            if b == 100.0:
                assert got[s, 2] == v[s].max()


def test_contrast_params_other_modes(lib):
    """mode 2: the six parameters against the fp64 formula on the same fp32 statistics; modes 0 and 3: par[0] == 0 and the
    pre-zeroed slots untouched"""
    stats = np.array([(2000, 62000, 30123.25), (0, 0, 0), (5, 9, 7), (100, 65535, 40000.5), (12000, 12800, 12345.75)],
                     dtype=np.float32)
    choice = np.array([(2, 1.2, 0.8, 0), (0, 9, 9, 9), (3, 9, 9, 9), (2, 0.75, 1.3, 0), (2, 1.25, 0.7, 0)], dtype=np.float32)
    n = len(stats)
    hd = torch.zeros(n * 65536, dtype=torch.int32, device="cuda")
    par = torch.zeros(8 * n + GUARD, device="cuda")
    par[8 * n:] = NAN
    sd, cd = _dev(stats), _dev(choice)            # held until the results are back: a freed block is handed out again at once
    _ok(lib.mseg_aug_contrast_params(sd.data_ptr(), hd.data_ptr(), cd.data_ptr(), n, 97 * 131,
                                     par.data_ptr(), _stream()))
    got = _take(par, 8 * n, (n, 8))
    for s in range(n):
        if choice[s, 0] != 2:
            assert (got[s] == 0).all(), got[s]
            continue
        r64 = R.contrast_params_mode2(stats[s], choice[s, 1], choice[s, 2])
        r32 = R.contrast_params_mode2(stats[s], choice[s, 1], choice[s, 2], np.float32)
        assert got[s, 0] == 2 and got[s, 2] == choice[s, 1] and got[s, 5] == choice[s, 2]          # passed through
        smooth = [1, 3, 4]                                               # mean, umin, umax - umin: one quantity
        e_ref = max(abs(float(r32[k]) - r64[k]) for k in smooth)
        e_hip = max(abs(float(got[s, k]) - r64[k]) for k in smooth)
        floor = 4 * _ulp(max(abs(r64[k]) for k in smooth))
        print(f"    mode 2 sample {s}: e_ref {e_ref:.2e} e_hip {e_hip:.2e} (4 ulp {floor:.2e})")
        assert e_hip <= max(4 * e_ref, floor), (s, got[s], r64)
        assert (got[s, 6:] == 0).all()


# =================================================================================================================================
# contrast, pointwise
# =================================================================================================================================
# Half-width of the band around the rounding boundary: 4 x the largest pre-rounding difference of the fp32 restatement, and
# never more than 0.01 (stretch) / 0.03 (contrast + gamma) — the restatement differs by 0.004 / 0.012, and only with these
# widths (1.9 % / 6 % of a smooth plane) can the banded share stay below the 3 % / 8 % it is capped at.
BAND_CAP = {1: 0.01, 2: 0.03}
SHARE_CAP = {1: 0.03, 2: 0.08}


def _banded(got, v, par, mode, what):
    out64, pre64 = R.contrast(v, par)
    _, pre32 = R.contrast(v, par, np.float32)
    d = float(np.abs(pre32.astype(np.float64) - pre64).max())
    band = R.near_integer(pre64, min(4 * d, BAND_CAP[mode]))
    diff = np.abs(got.astype(np.float64) - out64)
    print(f"    {what}: restatement differs by {d:.4f} before rounding, banded share {band.mean():.4f}, "
          f"{int((diff > 0).sum())} of {diff.size} pixels one off")
    assert band.mean() <= SHARE_CAP[mode], what
    assert diff.max() <= 1, what
    assert np.array_equal(got[~band].astype(np.float64), out64[~band]), f"{what}: a pixel away from the boundary differs"


@functools.lru_cache(maxsize=None)
def _contrast_case(shape):
    """six samples: stretch 0.2 / 99.8, contrast + gamma, mode 0, mode 3, stretch 0.1 / 99.9, contrast + gamma the other way;
    the parameter block is what the parameter kernel's formulas give in fp32"""
    planes = _smooth_planes(10, 6, *shape)
    par = np.zeros((6, 8), np.float32)
    for s, q in ((0, (0.2, 99.8)), (4, (0.1, 99.9))):
        par[s, :3] = (1, R.percentile(planes[s], q[0]), R.percentile(planes[s], q[1]))
    for s, (f, g) in ((1, (1.2, 0.8)), (5, (0.8, 1.25))):
        par[s, :6] = R.contrast_params_mode2(R.stats(planes[s])[:3], f, g, np.float32)
    par[2, :3], par[3, :3] = (0, 7, 9), (3, 7, 9)
    return planes, par


def _run_contrast(lib, planes, par):
    n, h, w = planes.shape
    src, pd, out = _dev(planes), _dev(par), _nan_buf(planes.size)
    _ok(lib.mseg_aug_contrast(src.data_ptr(), out.data_ptr(), n, h, w, pd.data_ptr(), _stream()))
    return _take(out, planes.size, planes.shape)


@pytest.mark.parametrize("shape", SHAPES + [(97, 131)])
def test_contrast(lib, shape):
    planes, par = _contrast_case(shape)
    got = _run_contrast(lib, planes, par)
    for s in range(6):
        mode = int(par[s, 0])
        if mode in (1, 2):
            _banded(got[s], planes[s], par[s], mode, f"contrast {shape} sample {s} mode {mode}")
        else:
            _same_bits(got[s], planes[s], f"mode {mode} copies")
    assert got[0].min() == 0 and got[0].max() == 65535


def test_contrast_stretch_of_an_empty_range_is_zero(lib):
    """the project's rule (kernel and oracle/augment_ref.py alike): p1 <= p0 maps the plane to 0"""
    planes = _smooth_planes(11, 3, 17, 23)
    par = np.zeros((3, 8), np.float32)
    par[:, :3] = ((1, 30000, 30000), (1, 40000, 20000), (1, 20000, 40000))
    got = _run_contrast(lib, planes, par)
    assert (got[0] == 0).all() and (got[1] == 0).all() and got[2].max() == 65535
    assert not np.signbit(got[:2]).any()


# =================================================================================================================================
# CLAHE
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def _clahe_planes(shape):
    """smooth integer planes whose grey-level coordinate v 16383 / 65535 + 0.5 stays >= 1e-3 away from an integer (a pixel that
    does not is moved up by one grey value), so that the binning is not in question"""
    v = _smooth_planes(12, 3, *shape).astype(np.float64)
    for _ in range(3):
        c = R.clahe_bin_coordinate(v)
        v = np.where(np.abs(c - np.rint(c)) < 2e-3, v + 1, v)
    c = R.clahe_bin_coordinate(v)
    assert (np.abs(c - np.rint(c)) >= 1e-3).all() and v.max() <= 65535
    return v.astype(np.float32)


@pytest.mark.parametrize("shape", [(24, 40), (8, 8), (13, 9)])
def test_clahe(lib, shape):
    """tiles of 3 x 5 pixels, of one pixel (clip limit 1) and of unequal sizes; samples 0 and 2 are equalised, sample 1 (mode 1)
    is copied.  The tile mappings read back from the workspace equal oracle/augment_ref.py's bit for bit."""
    h, w = shape
    planes = _clahe_planes(shape)
    choice = np.array([(3, 0, 0, 0), (1, 0.2, 99.8, 0), (3, 0, 0, 0)], dtype=np.float32)
    nbytes = lib.mseg_aug_clahe_workspace_bytes(3)
    assert nbytes == 3 * 64 * 256 * 4
    ws = _nan_buf(nbytes // 4)
    src, out = _dev(planes), _nan_buf(planes.size)
    cd = _dev(choice)
    _ok(lib.mseg_aug_clahe(src.data_ptr(), out.data_ptr(), 3, h, w, cd.data_ptr(), ws.data_ptr(), _stream()))
    got = _take(out, planes.size, planes.shape)
    torch.cuda.synchronize()
    maps = ws.cpu().numpy()
    assert np.isnan(maps[nbytes // 4:]).all(), "the kernel wrote behind its workspace"
    maps = maps[:nbytes // 4].reshape(3, 8, 8, 256)
    _same_bits(got[1], planes[1], "mode != 3 copies")
    assert np.isnan(maps[1]).all()
    for s in (0, 2):
        want_maps, _ = augment_ref.clahe_maps(planes[s].astype(np.float64))
        _same_bits(maps[s], want_maps, f"maps of sample {s}")
        out64, pre64 = R.clahe_apply(planes[s], want_maps)
        _, pre32 = R.clahe_apply(planes[s], want_maps, np.float32)
        d = float(np.abs(pre32.astype(np.float64) - pre64).max())
        band = R.near_integer(pre64, 4 * d)
        diff = np.abs(got[s].astype(np.float64) - out64)
        print(f"    clahe {shape} sample {s}: restatement differs by {d:.4f} before rounding, banded share {band.mean():.3f}, "
              f"{int((diff > 0).sum())} of {diff.size} pixels one off")
        assert diff.max() <= 1
        assert np.array_equal(got[s][~band].astype(np.float64), out64[~band])
        assert np.abs(got[s] - augment_ref.clahe(planes[s].astype(np.float64))).max() <= 1


def test_clahe_argument_checks(lib):
    a, b = _nan_buf(3 * 7 * 16), _nan_buf(3 * 7 * 16)
    ws = _nan_buf(3 * 64 * 256)
    ch = _dev(np.full((3, 4), 3, np.float32))
    assert lib.mseg_aug_clahe(a.data_ptr(), b.data_ptr(), 3, 7, 16, ch.data_ptr(), ws.data_ptr(), _stream()) == EINVAL
    assert lib.mseg_aug_clahe(a.data_ptr(), b.data_ptr(), 3, 16, 7, ch.data_ptr(), ws.data_ptr(), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(b).all() and torch.isnan(ws).all()


# =================================================================================================================================
# normalisation, noise
# =================================================================================================================================
def _run_noise(lib, planes, frac, stats, seed, vmin=0.0, vmax=65535.0):
    n, h, w = planes.shape
    src, fd, sd = _dev(planes), _dev(np.asarray(frac, np.float32)), _dev(np.asarray(stats, np.float32))
    out = _nan_buf(planes.size)
    _ok(lib.mseg_aug_noise_normalize(src.data_ptr(), out.data_ptr(), n, h, w, fd.data_ptr(), sd.data_ptr(),
                                     C.c_uint32(seed % 2 ** 32), vmin, vmax, _stream()))
    return _take(out, planes.size, planes.shape)


@pytest.mark.parametrize("lo,hi", [(0.0, 65535.0), (10000.0, 35000.0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_normalize_without_noise(lib, shape, lo, hi):
    planes = _noise_planes(13, 3, *shape)
    planes[:, 0, :6] = (0, 65535, 10000, 35000, 9999, 35001)
    stats = np.tile(np.array([0, 65535, 30000], np.float32), (3, 1))
    got = _run_noise(lib, planes, np.zeros(3), stats, 5, lo, hi)
    _same_bits(got, R.normalize_f32(planes, lo, hi), "normalisation")
    assert (got[planes <= lo] == -1).all() and (got[planes >= hi] == 1).all()
    assert got.min() == -1 and got.max() == 1


def test_normalize_argument_checks(lib):
    a, b = _nan_buf(3 * 25), _nan_buf(3 * 25)
    fr, st = _dev(np.zeros(3, np.float32)), _dev(np.zeros((3, 3), np.float32))
    for lo, hi in ((5.0, 5.0), (6.0, 5.0)):
        assert lib.mseg_aug_noise_normalize(a.data_ptr(), b.data_ptr(), 3, 5, 5, fr.data_ptr(), st.data_ptr(),
                                            C.c_uint32(1), lo, hi, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(b).all()


NOISE_SEED = 123456789
NOISE_FRAC = np.array([0.01, 0.05, 0.02, 0.03], dtype=np.float32)
NOISE_N, NOISE_S = 4, 128


def _noise_sigma():
    return (NOISE_FRAC * np.float32(40000)).astype(np.float64)


@pytest.fixture(scope="module")
def noise_fields(lib):
    """seed -> d = (grey - 30000) / sigma of the 4 x 128 x 128 constant plane 30000 with stats max = 40000, computed once"""
    cache = {}
    planes = np.full((NOISE_N, NOISE_S, NOISE_S), 30000, np.float32)
    stats = np.tile(np.array([30000, 40000, 30000], np.float32), (NOISE_N, 1))

    def get(seed):
        seed %= 2 ** 32
        if seed not in cache:
            out = _run_noise(lib, planes, NOISE_FRAC, stats, seed).astype(np.float64)
            grey = (out + 1) / 2 * 65535
            assert np.abs(grey - np.rint(grey)).max() <= 0.01, "grey values do not come back integer-valued"
            cache[seed] = (np.rint(grey) - 30000) / _noise_sigma()[:, None, None]
        return cache[seed]
    return get


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_noise_moments_and_distribution(noise_fields):
    d = noise_fields(NOISE_SEED)
    n = d.size
    x = d.ravel()
    mean, var = x.mean(), x.var()
    z = (x - mean) / math.sqrt(var)
    skew, kurt = (z ** 3).mean(), (z ** 4).mean() - 3
    want_var = 1 + float(np.mean(1 / (12 * _noise_sigma() ** 2)))                 # the rounding to a grey value adds 1 / 12
    xs = np.sort(x)
    cdf = 0.5 * (1 + special.erf(xs / math.sqrt(2)))
    ks = max(np.abs(np.arange(1, n + 1) / n - cdf).max(), np.abs(np.arange(n) / n - cdf).max())
    lag_x, lag_y, lag_s = _corr(d[:, :, 1:], d[:, :, :-1]), _corr(d[:, 1:], d[:, :-1]), _corr(d[1:], d[:-1])
    r = math.sqrt(n)
    print(f"    noise n {n}: mean {mean * r:.2f} / sqrt n, var - want {(var - want_var) / math.sqrt(2 / n):.2f} se, "
          f"skew {skew / math.sqrt(6 / n):.2f} se, kurtosis {kurt / math.sqrt(24 / n):.2f} se, KS {ks * r:.2f} / sqrt n, "
          f"lag x {lag_x * r:.2f} y {lag_y * r:.2f} sample {lag_s * r:.2f} / sqrt n")
    assert abs(mean) <= 5 / r
    assert abs(var - want_var) <= 5 * math.sqrt(2 / n)
    assert abs(skew) <= 5 * math.sqrt(6 / n)
    assert abs(kurt) <= 5 * math.sqrt(24 / n)
    assert ks <= 2 / r
    assert max(abs(lag_x), abs(lag_y), abs(lag_s)) <= 5 / r


def test_noise_sigma_is_per_sample_and_follows_the_statistics(noise_fields):
    """frac 0.01 against 0.05: the standard deviations in grey values are 1 : 5 within 5 standard errors (each has a relative
    standard error of 1 / sqrt(2 n), their ratio of 1 / sqrt(n)); and sigma = frac * stats max = frac * 40000 although the
    plane's own maximum is 30000 (which would give every sample a variance of 0.5625 in these units)"""
    d = noise_fields(NOISE_SEED)
    grey_std = d.reshape(NOISE_N, -1).std(axis=1) * _noise_sigma()
    n = NOISE_S * NOISE_S
    ratio = grey_std[1] / grey_std[0]
    print(f"    noise std per sample {grey_std}, ratio {ratio:.4f}")
    assert abs(ratio - 5) <= 5 * 5 / math.sqrt(n)
    for s in range(NOISE_N):
        assert abs(d[s].var() - (1 + 1 / (12 * _noise_sigma()[s] ** 2))) <= 5 * math.sqrt(2 / n)


def test_noise_same_seed_same_bits_and_next_seed_uncorrelated(lib, noise_fields):
    planes = np.full((NOISE_N, NOISE_S, NOISE_S), 30000, np.float32)
    stats = np.tile(np.array([30000, 40000, 30000], np.float32), (NOISE_N, 1))
    a = _run_noise(lib, planes, NOISE_FRAC, stats, NOISE_SEED)
    b = _run_noise(lib, planes, NOISE_FRAC, stats, NOISE_SEED)
    _same_bits(a, b, "two runs with one seed")
    c = _corr(noise_fields(NOISE_SEED), noise_fields(NOISE_SEED + 1))
    print(f"    seeds s, s + 1: correlation {c * math.sqrt(a.size):.2f} / sqrt n")
    assert abs(c) <= 5 / math.sqrt(a.size)


@pytest.mark.parametrize("j", [-1, 1, 2])
def test_noise_seeds_a_multiplier_apart_are_uncorrelated(noise_fields, j):
    """the key multiplies the pixel index by 2654435761: with the seed added beside it, seed + j * 2654435761 gave the field of
    seed shifted by j pixels (correlation 1 at lag j)"""
    a = noise_fields(NOISE_SEED).ravel()
    b = noise_fields(NOISE_SEED + j * GOLDEN).ravel()
    n = a.size
    for lag in range(-2, 3):
        c = _corr(a[max(lag, 0):n + min(lag, 0)], b[max(-lag, 0):n + min(-lag, 0)])
        print(f"    seeds s, s {j:+d} * 2654435761, lag {lag:+d}: correlation {c * math.sqrt(n):.2f} / sqrt n")
        assert abs(c) <= 5 / math.sqrt(n), (j, lag, c)


def test_noise_clips_at_zero(lib):
    """v = 100 under sigma = 0.05 * 40000 = 2000: no output below -1, and the share that is exactly -1 (grey value 0, i.e.
    v + sigma g < 0.5) matches the normal tail within 5 standard errors"""
    n, s = 3, 128
    planes = np.full((n, s, s), 100, np.float32)
    stats = np.tile(np.array([100, 40000, 100], np.float32), (n, 1))
    got = _run_noise(lib, planes, np.full(n, 0.05), stats, 987654321)
    assert got.min() >= -1
    p = 0.5 * (1 + math.erf((0.5 - 100) / 2000 / math.sqrt(2)))
    share = float((got == -1).mean())
    se = math.sqrt(p * (1 - p) / got.size)
    print(f"    clipped share {share:.5f}, normal tail {p:.5f}, {abs(share - p) / se:.2f} se")
    assert abs(share - p) <= 5 * se
