"""GPU (MI355X): the small element-wise / reduction kernels through the C ABI against the fp64 references of
tests/pointwise_ref.py (which tests/test_pointwise_ref_host.py pins to torch on the CPU):

  mseg_regression_loss / _bwd, mseg_ce_dice_fwd / _bwd            csrc/loss.hip
  mseg_maxpool2x2_fwd / _bwd, mseg_activation                     csrc/norm.hip
  mseg_softmax3_hwc                                               csrc/head.hip
  mseg_f32_to_bf16, mseg_pack_weight, mseg_pack_weights_multi     csrc/igemm.hip

Outputs are pre-filled with NaN and carry a NaN guard band behind them that must come back untouched.  Inputs whose branch
decisions matter lie on binary grids, so that no decision depends on a rounding.  Bounds are derived from the number of
fp32 roundings of each formula; the two that are measured (ce_dice backward, fp32 activations) follow the suite's rule
e_hip <= max(4 e_ref, floor) with fp64 as the yardstick and e_ref = what torch's CPU fp32 achieves on the same inputs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R
from helpers import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24             # unit roundoff of fp32
GUARD = 64                 # elements of guard band behind an output
EINVAL = -1
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from microbeseg_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return (t if dtype is None else t.to(dtype)).contiguous().cuda()


def _nan_buf(n, dtype=torch.float32):
    """n output elements + the guard band, all NaN"""
    return torch.full((n + GUARD,), NAN, dtype=dtype, device="cuda")


def _take(buf, n):
    """-> the n output elements on the CPU, after checking that the guard band still holds its NaNs"""
    torch.cuda.synchronize()
    host = buf.cpu()
    assert torch.isnan(host[n:].float()).all(), "the kernel wrote behind its output"
    return host[:n]


def _ok(code):
    assert code == 0, f"libmseg_hip returned {code}"


# =================================================================================================================================
# regression losses
# =================================================================================================================================
RESIDUALS = [0.0, 1.0, -1.0, 1 - 2.0 ** -10, -(1 - 2.0 ** -10), 1 + 2.0 ** -10, -(1 + 2.0 ** -10), 50.0, -50.0]
PLANT_AT = [0, 1, 2, 17, 63, 64, 100, 128, 200]          # the residuals above, where the index exists
REG_N = [1, 3, 255, 256, 257, 262144 + 257]             # the forward's grid stride starts at 1024 * 256 elements
REG_N_BWD = REG_N + [1048576 + 259]                      # the backward's at 4 * 1024 * 256


@functools.lru_cache(maxsize=None)
def _reg_case(n):
    """pred, target (fp32, on the grid k 2^-10 in [-64, 64]: every residual is exact in fp32) with planted residuals of
    exactly 0, +-1, +-(1 -+ 2^-10), +-50 at fixed indices, and -1 / 0 / +1 on the last three elements (the grid-stride tail of
    the large sizes); plus the fp64 loss values and unit-scale gradients of the three kinds"""
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    pred = rng.integers(-65536, 65537, n).astype(np.float64) / 1024
    target = rng.integers(-65536, 65537, n).astype(np.float64) / 1024
    # near residuals too (|d| < 4): half of the elements, so both smooth-L1 branches are populated
    near = rng.random(n) < 0.5
    target[near] = np.clip(pred[near] + rng.integers(-4096, 4097, int(near.sum())) / 1024, -64, 64)
    for i, r in zip(PLANT_AT, RESIDUALS):
        if i < n:
            pred[i], target[i] = 0.25 + r, 0.25
    if n >= 255:
        for i, r in ((n - 1, -1.0), (n - 2, 0.0), (n - 3, 1.0)):
            pred[i], target[i] = -3.5 + r, -3.5
    p32, t32 = pred.astype(np.float32), target.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), pred) and np.array_equal(t32.astype(np.float64), target)
    d = pred - target
    assert np.array_equal((p32 - t32).astype(np.float64), d), "a residual is not exact in fp32"
    if n >= 255:
        assert all((d == r).any() for r in RESIDUALS)
    loss = {k: R.reg_loss(pred, target, k) for k in range(3)}
    grad = {k: R.reg_grad(pred, target, k).numpy() for k in range(3)}
    return torch.from_numpy(p32), torch.from_numpy(t32), loss, grad


@pytest.mark.parametrize("n", REG_N)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_regression_loss_value(lib, kind, n):
    """relative error to fp64 <= 1e-6: every term is non-negative and costs at most four fp32 roundings (the residual is
    exact), the accumulation is fp64 and there is one final rounding: about 3e-7 in truth"""
    pred, target, loss, _ = _reg_case(n)
    p, t = _dev(pred), _dev(target)
    out = _nan_buf(1)
    ws = torch.empty(lib.mseg_loss_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    _ok(lib.mseg_regression_loss(p.data_ptr(), t.data_ptr(), n, kind, out.data_ptr(), ws.data_ptr(), _stream()))
    got = float(_take(out, 1)[0])
    err = abs(got - loss[kind])
    print(f"regression value kind {kind} n {n}: got {got!r} ref {loss[kind]!r} rel {err / max(abs(loss[kind]), 1e-300):.2e}")
    assert err <= 1e-6 * abs(loss[kind])


@pytest.mark.parametrize("n", REG_N_BWD)
@pytest.mark.parametrize("gscale", [None, 0.37])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_regression_loss_gradient(lib, kind, gscale, n):
    """per element |got - ref| <= 4 * 2^-24 |ref| (gscale / (float)n and its product with the exact per-element factor are two
    roundings), and exactly 0 where the reference is 0"""
    pred, target, _, grad = _reg_case(n)
    p, t = _dev(pred), _dev(target)
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device="cuda")
    scale = 1.0 if gs is None else float(gs.cpu()[0])           # the fp32 value the kernel reads
    out = _nan_buf(n)
    _ok(lib.mseg_regression_loss_bwd(p.data_ptr(), t.data_ptr(), n, kind, None if gs is None else gs.data_ptr(),
                                     out.data_ptr(), _stream()))
    got = _take(out, n).double().numpy()
    ref = grad[kind] * scale
    assert not np.isnan(got).any()
    assert np.array_equal(got[ref == 0], ref[ref == 0]), "a gradient that is exactly 0 came back non-zero"
    err = np.abs(got - ref)
    nz = ref != 0
    if nz.any():
        print(f"regression gradient kind {kind} n {n} gscale {gscale}: max rel {np.max(err[nz] / np.abs(ref[nz])) / U:.2f} u")
    bad = np.flatnonzero(err > 4 * U * np.abs(ref))
    assert bad.size == 0, (f"{bad.size} elements off, first at {bad[0]}: d = {float(pred[bad[0]] - target[bad[0]])!r}, "
                           f"got {got[bad[0]]!r}, ref {ref[bad[0]]!r}")


@pytest.mark.parametrize("kind,name", [(1, "l1"), (2, "l2")])
def test_regression_loss_through_get_loss(lib, kind, name):
    """get_loss(kind, 'distance'): (0.37 * loss).backward() against torch.nn on fp64 CPU copies.  Value as above; gradient
    4 u from the kernel + 1 u because the factor reaches it as fp32(0.37)"""
    from microbeseg_amd.training.losses import get_loss
    pred, target, _, _ = _reg_case(2 * 33 * 41)
    shape = (2, 1, 33, 41)
    crit = get_loss(name, "distance")
    assert set(crit) == {"border", "cell"}
    ref_mod = {1: torch.nn.L1Loss(), 2: torch.nn.MSELoss()}[kind]
    p64 = pred.double().reshape(shape).requires_grad_(True)
    ref = ref_mod(p64, target.double().reshape(shape))
    (0.37 * ref).backward()
    for head in ("border", "cell"):
        p = pred.reshape(shape).cuda().requires_grad_(True)
        loss = crit[head](p, target.reshape(shape).cuda())
        (0.37 * loss).backward()
        assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
        got, want = p.grad.cpu().double(), p64.grad
        assert torch.equal(got[want == 0], want[want == 0])
        assert ((got - want).abs() <= 5 * U * want.abs()).all()


# =================================================================================================================================
# ce_dice
# =================================================================================================================================
CE_SHAPES = [(1, 1), (3, 37 * 5), (2, 131329)]           # the forward's grid stride starts at 262144 pixels
CE_SHAPES_BWD = CE_SHAPES + [(3, 349531)]                # the backward's at 1048576
# Floor of the measured bound of test_ce_dice_backward.  First run on the MI355X, over all shapes, modes and gscale values:
# e_ref 4.0e-8 .. 3.2e-7, e_hip 4.0e-8 .. 3.0e-7 (worst pair: (3, 349531), two-ranks, gscale 0.37: e_ref 3.21e-7, e_hip 2.98e-7).
# 4 e_ref is the working bound almost everywhere; the floor only catches a tensor on which torch's fp32 happens to round
# well ((1, 1): e_ref 4.0e-8).  1e-6 = 17 u, about three times the largest e_hip: the chain is three expf, a three-term sum,
# a division, the product with 1 / total_px and, per Dice class, about eight more multiply-adds and two divisions by B.
CE_BWD_FLOOR = 1e-6


def _logits(rng, N, HW):
    """N(0, 3) logits [N][3][HW] with planted pixels: spreads of +-80 (a probability that underflows to 0 in fp32) in three
    orders, and three equal logits"""
    l = (rng.standard_normal((N, 3, HW)) * 3).astype(np.float32)
    plant = [(80.0, 0.0, -80.0), (-80.0, 80.0, 0.0), (0.0, -80.0, 80.0), (1.5, 1.5, 1.5), (0.0, 0.0, 0.0), (-80.0, -80.0, 80.0)]
    for j, v in enumerate(plant):
        n, p = j % N, (j * 7919 + 3) % HW
        if HW > 8 * len(plant):
            l[n, :, p] = v
        if HW > 100000 and n == N - 1:
            l[n, :, HW - 1 - j] = v             # the grid-stride tail
    return l


@functools.lru_cache(maxsize=None)
def _ce_case(N, HW, absent=False):
    rng = np.random.Generator(np.random.PCG64(77 + N * 1000003 + HW + absent))
    logits = _logits(rng, N, HW)
    labels = rng.integers(0, 2 if absent else 3, (N, HW)).astype(np.int64)
    if HW == 1:          # one pixel: a planted one (three equal logits), so that max|grad| is of the order of 1 / total_px as in
        labels[:] = 1    # any real tensor (a lone confident pixel has gradients far below the rounding of its probabilities)
        logits[0, :, 0] = 1.5
    elif not absent:
        labels[0, :3] = [0, 1, 2]
    sums6, ce_sum = R.ce_dice_fwd(logits, labels)
    return torch.from_numpy(logits), torch.from_numpy(labels), sums6, ce_sum


def _ce_cases():
    return [(N, HW, False) for N, HW in CE_SHAPES] + [(3, 37 * 5, True)]


@pytest.mark.parametrize("N,HW,absent", _ce_cases())
def test_ce_dice_forward(lib, N, HW, absent):
    """sums6 relative <= 2e-6 (non-negative terms, every probability within ~5 ulp, fp64 sums; a sum whose reference is 0 —
    an absent class — must be exactly 0); ce_sum absolute <= 8 * 2^-24 (max|logit| + 1) N HW (lse - l_y cancels); with_dice
    changes neither output"""
    logits, labels, sums6, ce_sum = _ce_case(N, HW, absent)
    if absent:
        assert sums6[3] == 0 and sums6[5] == 0
    elif HW > 1:
        assert sums6[2] > 0 and sums6[5] > 0 and sums6[2] + sums6[5] < N * HW
    l, y = _dev(logits), _dev(labels)
    ws = torch.empty(lib.mseg_loss_workspace_bytes(N * HW), dtype=torch.uint8, device="cuda")
    outs = []
    for with_dice in (0, 1):
        s = _nan_buf(6, torch.float64)
        c = _nan_buf(1, torch.float64)
        _ok(lib.mseg_ce_dice_fwd(l.data_ptr(), y.data_ptr(), N, HW, with_dice, s.data_ptr(), c.data_ptr(), ws.data_ptr(),
                                 _stream()))
        outs.append((_take(s, 6).numpy(), float(_take(c, 1)[0])))
    (s0, c0), (s1, c1) = outs
    assert np.array_equal(s0, s1) and c0 == c1
    err = np.abs(s1 - sums6)
    print(f"ce_dice fwd ({N}, {HW}): sums rel {np.max(err / np.maximum(np.abs(sums6), 1e-300)):.2e}, "
          f"ce_sum abs {abs(c1 - ce_sum):.3e} of bound {8 * U * (float(logits.abs().max()) + 1) * N * HW:.3e}")
    assert (err <= 2e-6 * np.abs(sums6)).all(), (s1, sums6)
    assert abs(c1 - ce_sum) <= 8 * U * (float(logits.abs().max()) + 1) * N * HW


def _ce_bwd_modes(sums6, total):
    """(name, with_dice, sums passed in, total_px, dice_weight)"""
    return [("own", 1, sums6, float(total), 1.0),
            ("two-ranks", 1, 2.0 * sums6, 2.0 * total, 2.0),       # a second rank with the same pixels: every sum doubles
            ("ce", 0, sums6, float(total), 1.0)]


@pytest.mark.parametrize("gscale", [None, 0.37])
@pytest.mark.parametrize("N,HW,absent", [(N, HW, False) for N, HW in CE_SHAPES_BWD] + [(3, 37 * 5, True)])
def test_ce_dice_backward(lib, N, HW, absent, gscale):
    """The gradient against the analytic fp64 gradient for the sums6 PASSED IN: own sums with dice_weight 1; the sums two
    ranks would all-reduce with dice_weight 2 and total_px = 2 N HW; with_dice = 0.  Bound: e_hip <= max(4 e_ref, floor) under
    helpers.rel_err, e_ref = the same formula in torch CPU fp32.
    Measured on the MI355X (first run): e_ref / e_hip = 3.99e-8 / 3.99e-8 at (1, 1), 1.80e-7 / 1.80e-7 at (3, 185),
    2.73e-7 / 2.73e-7 at (2, 131329), 3.21e-7 / 2.98e-7 at (3, 349531), 2.91e-7 / 2.91e-7 with class 2 absent (the worst mode
    of each shape; equal pairs: both round the largest gradient to the same fp32 number); channel sums <= 5.5 u.
    Also: the three channel gradients of a pixel sum to 0 analytically (softmax), here to <= 8 * 2^-24 max|grad| — a wrong
    plane offset breaks this even when the max-norm looks fine."""
    logits, labels, sums6, _ = _ce_case(N, HW, absent)
    l, y = _dev(logits), _dev(labels)
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device="cuda")
    scale = 1.0 if gs is None else float(gs.cpu()[0])
    for name, with_dice, sums, total, dw in _ce_bwd_modes(sums6, N * HW):
        s = _dev(sums, torch.float64)
        out = _nan_buf(N * 3 * HW)
        _ok(lib.mseg_ce_dice_bwd(l.data_ptr(), y.data_ptr(), N, HW, with_dice, s.data_ptr(), total, dw,
                                 None if gs is None else gs.data_ptr(), out.data_ptr(), _stream()))
        got = _take(out, N * 3 * HW).double().reshape(N, 3, HW)
        assert not torch.isnan(got).any()
        ref = R.ce_dice_grad(logits, labels, sums, total, dw, scale, bool(with_dice))
        ref32 = R.ce_dice_grad(logits, labels, sums, total, dw, scale, bool(with_dice), dtype=torch.float32)
        e_ref, e_hip = rel_err(ref32, ref), rel_err(got, ref)
        csum = got.sum(dim=1).abs().max().item() / got.abs().max().item()
        print(f"ce_dice bwd ({N}, {HW}) absent {absent} gscale {gscale} {name}: e_ref {e_ref:.3e} e_hip {e_hip:.3e} "
              f"channel sum {csum / U:.2f} u")
        assert e_hip <= max(4 * e_ref, CE_BWD_FLOOR), f"{name}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}"
        assert csum <= 8 * U, f"{name}: the channel gradients of a pixel sum to {csum / U:.1f} u of max|grad|"


def test_cross_entropy_through_get_loss(lib):
    """get_loss('ce', 'boundary') (with_dice = 0 on the device) against F.cross_entropy in fp64: value within the per-pixel
    mean of the ce_sum bound + the final fp32 rounding, gradient under the rule of test_ce_dice_backward"""
    from microbeseg_amd.training.losses import get_loss
    N, H, W = 3, 37, 5
    logits, labels, _, _ = _ce_case(N, H * W)
    crit = get_loss("ce", "boundary")
    l64 = logits.double().reshape(N, 3, H, W).requires_grad_(True)
    ref = F.cross_entropy(l64, labels.reshape(N, H, W))
    (0.37 * ref).backward()
    l32 = logits.reshape(N, 3, H, W).clone().requires_grad_(True)
    (0.37 * F.cross_entropy(l32, labels.reshape(N, H, W))).backward()
    l = logits.reshape(N, 3, H, W).cuda().requires_grad_(True)
    loss = crit(l, labels.reshape(N, H, W).cuda())
    (0.37 * loss).backward()
    assert abs(loss.item() - ref.item()) <= 8 * U * (float(logits.abs().max()) + 1) + U * abs(ref.item())
    e_ref, e_hip = rel_err(l32.grad, l64.grad), rel_err(l.grad.cpu(), l64.grad)
    print(f"get_loss('ce'): e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip <= max(4 * e_ref, CE_BWD_FLOOR)


# =================================================================================================================================
# max-pool
# =================================================================================================================================
# (N, C, H, W).  A thread owns 4 channels of one window and the grid is capped at 8192 * 256 threads.  The largest of
# POOL_SHAPES has 2 * 64 * 68 * 16 = 139 264 such work items (many blocks, one trip each); POOL_STRIDE_SHAPE has
# 1 * 364 * 362 * 16 = 2 108 288, so there — and only there — the grid-stride loops take a second trip.
POOL_SHAPES = [(1, 4, 2, 2), (2, 8, 6, 10), (3, 12, 4, 2), (2, 64, 128, 136)]
POOL_STRIDE_SHAPE = (1, 64, 728, 724)


@functools.lru_cache(maxsize=None)
def _pool_case(shape, act, per_sample):
    """z on the grid k / 8 in [-4, 4], scale in +-{0.5, 1, 2}, shift in {0, +-1}: act(z) * scale + shift is exact in fp32 with
    or without FMA contraction, so both directions can be compared bit for bit.  gout and the old gin on the grid k / 16."""
    N, Cc, H, W = shape
    rng = np.random.Generator(np.random.PCG64(5 + N + 10 * Cc + 1000 * H + 100000 * W + per_sample))
    z = rng.integers(-32, 33, (N, H, W, Cc)).astype(np.float32) / 8
    tab = (N, Cc) if per_sample else (Cc,)
    scale = (rng.choice([0.5, 1.0, 2.0], tab) * rng.choice([-1.0, 1.0], tab)).astype(np.float32)
    if Cc >= 4:
        scale.reshape(-1)[:2] = [-2.0, 0.5]                     # both signs whatever the draw
    shift = rng.choice([0.0, 1.0, -1.0], tab).astype(np.float32)
    gout = rng.integers(-16, 17, (N, H // 2, W // 2, Cc)).astype(np.float32) / 16
    old = rng.integers(-16, 17, (N, H, W, Cc)).astype(np.float32) / 16
    out, arg = R.maxpool_fwd(z, act, scale, shift)
    assert torch.equal(out.float().double(), out)
    return z, scale, shift, gout, old, out, arg


def _pool_preconditions(z, act, scale, shift, out, arg):
    """so that the case cannot go vacuous: ties for the maximum, at every window position, and windows whose raw-tensor argmax
    differs from the argmax of the transformed tensor (negative scales)"""
    w = R._windows(R.transform(z, act, scale, shift))
    is_max = w == out[None]
    tied = is_max.sum(0) >= 2
    raw_arg = R.maxpool_fwd(z, "none")[1]
    stats = {"tie": tied.double().mean().item(), "flip": (raw_arg != arg).double().mean().item(),
             "tie_at": [bool((is_max[k] & tied).any()) for k in range(4)],
             "first_at": [bool(((arg == k) & tied).any()) for k in range(3)]}
    return stats


def _src(lib_mod, z, act, scale, shift, per_sample, dtype=0):
    s = lib_mod.MsegSrc()
    s.ptr, s.C, s.act, s.dtype = z.data_ptr(), z.shape[-1], R.ACTS.index(act), dtype
    s.scale, s.shift = scale.data_ptr(), shift.data_ptr()
    s.ss = z.shape[-1] if per_sample else 0
    return s


def _run_pool(lib, shape, act, per_sample, accumulate, case=None):
    from microbeseg_amd import _lib
    N, Cc, H, W = shape
    z, scale, shift, gout, old, out, arg = case or _pool_case(shape, act, per_sample)
    zd, sc, sh, gd = _dev(z), _dev(scale), _dev(shift), _dev(gout)
    s = _src(_lib, zd, act, sc, sh, per_sample)
    n_out, n_in = N * (H // 2) * (W // 2) * Cc, N * H * W * Cc
    ob = _nan_buf(n_out)
    _ok(lib.mseg_maxpool2x2_fwd(C.byref(s), N, H, W, ob.data_ptr(), _stream()))
    got = _take(ob, n_out).reshape(out.shape)
    assert torch.equal(got.view(torch.int32), out.float().view(torch.int32)), "forward differs from the exact result"
    gb = _nan_buf(n_in)
    if accumulate:
        gb[:n_in] = _dev(old).reshape(-1)
    _ok(lib.mseg_maxpool2x2_bwd(C.byref(s), N, H, W, gd.data_ptr(), gb.data_ptr(), accumulate, _stream()))
    gin = _take(gb, n_in).reshape(N, H, W, Cc)
    ref = R.maxpool_bwd(arg, gout, old if accumulate else None)
    assert torch.equal(ref.float().double(), ref)
    assert torch.equal(gin.double(), ref), "backward differs from first-maximum routing"
    if accumulate:
        routed = R.maxpool_bwd(arg, torch.ones(gout.shape, dtype=torch.float64)) != 0
        assert torch.equal(gin[~routed].view(torch.int32), torch.from_numpy(old)[~routed].view(torch.int32)), \
            "a position without gradient lost its old value"
    else:
        assert torch.equal(gin.view(torch.int32), ref.float().view(torch.int32))       # the zeros are +0


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("act", ["relu", "none"])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_forward_backward_bit_exact(lib, shape, act, per_sample, accumulate):
    N, Cc, H, W = shape
    z, scale, shift, _, _, out, arg = _pool_case(shape, act, per_sample)
    st = _pool_preconditions(z, act, scale, shift, out, arg)
    if out.numel() >= 64:                  # all but the 4-window shape: fractions mean something
        assert (scale < 0).any() and (scale > 0).any()
        assert st["flip"] >= 0.10, st
        if act == "relu":
            assert st["tie"] >= 0.05, st
    if out.numel() >= 200 and act == "relu":
        assert all(st["tie_at"]) and all(st["first_at"]), st
    _run_pool(lib, shape, act, per_sample, accumulate)


def test_maxpool_grid_stride(lib):
    """more windows x channel groups than the 8192 * 256 threads of the capped grid: the only shape at which the kernels'
    grid-stride loops take a second trip"""
    N, Cc, H, W = POOL_STRIDE_SHAPE
    assert N * (H // 2) * (W // 2) * (Cc // 4) > 8192 * 256
    _run_pool(lib, POOL_STRIDE_SHAPE, "relu", True, 0, case=_pool_case.__wrapped__(POOL_STRIDE_SHAPE, "relu", True))


def test_maxpool_argument_checks(lib):
    """odd H or W, C % 4 != 0 and a source that is not stored as fp32 are MSEG_EINVAL; a rejected call launches nothing (the
    buffers are valid and large enough all the same, and come back untouched)"""
    from microbeseg_amd import _lib
    z = torch.zeros((2, 6, 6, 8), dtype=torch.float32, device="cuda")
    sc, sh = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
    gout = torch.ones(2 * 3 * 3 * 8, device="cuda")
    for N, H, W, Cc, dtype in ((2, 5, 6, 8, 0), (2, 6, 5, 8, 0), (2, 6, 6, 6, 0), (2, 6, 6, 8, _lib.ST_BF16), (2, 6, 6, 8, 7)):
        s = _src(_lib, z, "relu", sc, sh, False, dtype)
        s.C = Cc
        out, gin = _nan_buf(z.numel()), _nan_buf(z.numel())
        assert lib.mseg_maxpool2x2_fwd(C.byref(s), N, H, W, out.data_ptr(), _stream()) == EINVAL
        assert lib.mseg_maxpool2x2_bwd(C.byref(s), N, H, W, gout.data_ptr(), gin.data_ptr(), 0, _stream()) == EINVAL
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(gin).all()
    s = _src(_lib, z, "relu", sc, sh, False, _lib.ST_F32)
    out = _nan_buf(2 * 3 * 3 * 8)
    _ok(lib.mseg_maxpool2x2_fwd(C.byref(s), 2, 6, 6, out.data_ptr(), _stream()))
    assert (_take(out, 2 * 3 * 3 * 8) == 0).all()


# =================================================================================================================================
# softmax over the three classes + crop + CHW -> HWC
# =================================================================================================================================
# pad_y != pad_x and Hp != Wp throughout, so that a swap cannot cancel
SOFTMAX_CASES = [(1, 1, 0, 0), (9, 14, 0, 0), (9, 14, 3, 0), (9, 14, 0, 5), (17, 23, 4, 9), (300, 259, 12, 3)]


@pytest.mark.parametrize("Hp,Wp,pad_y,pad_x", SOFTMAX_CASES)
def test_softmax3_hwc(lib, Hp, Wp, pad_y, pad_x):
    """every probability within 8 * 2^-24 absolute of fp64 (three expf at <= 1 ulp, a three-term sum, a division), each pixel's
    three values sum to 1 within the same bound, the guard band behind probs_hwc stays NaN"""
    rng = np.random.Generator(np.random.PCG64(31 + Hp * 1000 + Wp + 7 * pad_y + 13 * pad_x))
    logits = _logits(rng, 1, Hp * Wp)[0].reshape(3, Hp, Wp)
    ref = R.softmax_crop_hwc(logits, pad_y, pad_x)
    H, W = Hp - pad_y, Wp - pad_x
    assert ref.shape == (H, W, 3)
    out, ld = _nan_buf(H * W * 3), _dev(logits)
    _ok(lib.mseg_softmax3_hwc(ld.data_ptr(), Hp, Wp, pad_y, pad_x, out.data_ptr(), _stream()))
    got = _take(out, H * W * 3).double().reshape(H, W, 3)
    assert not torch.isnan(got).any()
    err = (got - ref).abs().max().item()
    one = (got.sum(dim=2) - 1).abs().max().item()
    print(f"softmax ({Hp}, {Wp}, {pad_y}, {pad_x}): max abs {err / U:.2f} u, sum - 1 {one / U:.2f} u")
    assert err <= 8 * U
    assert one <= 8 * U


def test_softmax3_hwc_argument_checks(lib):
    logits = torch.zeros((3, 9, 14), device="cuda")
    for pad_y, pad_x in ((9, 0), (0, 14), (-1, 0), (0, -1), (12, 20)):
        out = _nan_buf(9 * 14 * 3)
        assert lib.mseg_softmax3_hwc(logits.data_ptr(), 9, 14, pad_y, pad_x, out.data_ptr(), _stream()) == EINVAL
        torch.cuda.synchronize()
        assert torch.isnan(out).all()


# =================================================================================================================================
# activation (the eval-mode BatchNorm path of mish / elu / leakyrelu)
# =================================================================================================================================
ACT_PLANTED = [0.0, 2.0 ** -20, -2.0 ** -20, 20.0, -20.0, 20 + 2.0 ** -4, 20 - 2.0 ** -4, 60.0, -60.0, -100.0]
# Floor of the measured bound of test_activation_fp32.  First run on the MI355X, e_ref / e_hip at (2, 4099, 64): leakyrelu
# 8.11e-8 / 8.11e-8 (the fp32 slope), elu 5.97e-8 / 8.39e-8, mish 2.06e-7 / 2.80e-7; none and relu 0 / 0.  At (1, 1, 4) e_ref is as
# small as 1.5e-13 (elu) and the floor is what bounds: 5e-7 = 8 u, not quite twice the largest e_hip — mish is expf (<= 1 ulp),
# two multiply-adds, a division and a multiplication.
ACT_FLOOR = 5e-7


def _act_input(N, HW, Cc, seed):
    """N(0, 3) plus planted 0, +-2^-20, +-20, 20 +- 2^-4, +-60 and -100 (the mish threshold, ELU saturating to -1, the mish tail
    reaching -0), at the front and — where there is room — at the very end of the tensor"""
    rng = np.random.Generator(np.random.PCG64(seed))
    z = (rng.standard_normal(N * HW * Cc) * 3).astype(np.float32)
    k = min(len(ACT_PLANTED), z.size)
    z[:k] = ACT_PLANTED[:k]
    if z.size >= 4 * len(ACT_PLANTED):
        z[-k:] = ACT_PLANTED[::-1]
    return z


@pytest.mark.parametrize("N,HW,Cc", [(1, 1, 4), (3, 37, 12), (2, 4099, 64)])
@pytest.mark.parametrize("act", R.ACTS)
def test_activation_fp32(lib, act, N, HW, Cc):
    """fp32 storage against fp64: per element |got - ref| <= max(4 e_ref, floor) * max(|ref|, 2^-20), e_ref = the same measure of
    torch's CPU fp32 activation.  relu and none are exact.
    Measured on the MI355X (first run), e_ref / e_hip: mish 2.06e-7 / 2.80e-7, elu 5.97e-8 / 8.39e-8, leakyrelu
    8.11e-8 / 8.11e-8 at (2, 4099, 64); 1.50e-7 / 2.04e-7, 5.41e-8 / 6.39e-8, 7.82e-8 / 7.82e-8 at (3, 37, 12)."""
    z = _act_input(N, HW, Cc, 41 + N + HW + Cc)
    n = z.size
    out, zd = _nan_buf(n), _dev(z)
    _ok(lib.mseg_activation(zd.data_ptr(), N, HW, Cc, 0, R.ACTS.index(act), out.data_ptr(), _stream()))
    got = _take(out, n).double()
    assert not torch.isnan(got).any()
    ref = R.activation(z, act)
    ref32 = {"none": lambda v: v, "relu": F.relu, "leakyrelu": lambda v: F.leaky_relu(v, 0.01), "elu": F.elu,
             "mish": lambda v: v * torch.tanh(F.softplus(v))}[act](torch.from_numpy(z)).double()
    den = torch.clamp(ref.abs(), min=2.0 ** -20)
    e_ref = ((ref32 - ref).abs() / den).max().item()
    e_hip = ((got - ref).abs() / den).max().item()
    print(f"activation fp32 {act} ({N}, {HW}, {Cc}): e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    if act in ("none", "relu"):
        assert torch.equal(got, ref)
    assert e_hip <= max(4 * e_ref, ACT_FLOOR)


@pytest.mark.parametrize("N,HW,Cc", [(3, 37, 8), (2, 4099, 8), (3, 37, 24), (2, 4099, 24)])
@pytest.mark.parametrize("act", R.ACTS)
def test_activation_bf16(lib, act, N, HW, Cc):
    """bf16 storage (a thread owns 8 channels; fast-math mish / elu): |got - ref64| <= 2^-8 |ref| + 2^-133 — half a bf16 ulp for
    the rounding and half for the evaluation; relu, leakyrelu and none must equal the RNE of the exact value bit for bit (the
    exact value of leakyrelu being z times the fp32 slope the header's 0.01 denotes)"""
    z16 = torch.from_numpy(_act_input(N, HW, Cc, 43 + N + HW + Cc)).to(torch.bfloat16)
    n = z16.numel()
    out, zd = _nan_buf(n, torch.bfloat16), z16.cuda()
    _ok(lib.mseg_activation(zd.data_ptr(), N, HW, Cc, 1, R.ACTS.index(act), out.data_ptr(), _stream()))
    got16 = _take(out, n)
    got = got16.double()
    assert not torch.isnan(got).any()
    z = z16.double()
    ref = R.activation(z, act)
    err = (got - ref).abs()
    print(f"activation bf16 {act} ({N}, {HW}, {Cc}): max err / bound {(err / (2.0 ** -8 * ref.abs() + 2.0 ** -133)).max().item():.3f}")
    bad = torch.nonzero(err > 2.0 ** -8 * ref.abs() + 2.0 ** -133).reshape(-1)
    assert bad.numel() == 0, (f"{bad.numel()} elements off, first: z = {z[bad[0]].item()!r}, got {got[bad[0]].item()!r}, "
                              f"ref {ref[bad[0]].item()!r}")
    if act in ("none", "relu", "leakyrelu"):
        exact = R.activation(z, act, slope=float(np.float32(0.01))).numpy()
        want = R.bf16_round(exact)
        assert np.array_equal(got16.view(torch.int16).numpy().view(np.uint16), want)


# =================================================================================================================================
# fp32 -> bf16
# =================================================================================================================================
def _bf16_specials():
    u = []
    for hi in (0x3f80, 0x3f81, 0x4000, 0x0080, 0x7f7e, 0x0001, 0x007f):        # even and odd kept halves; normal and subnormal
        for lo in (0x8000, 0x8001, 0x7fff):                                  # the tie, just above, just below
            u += [(hi << 16) | lo, 0x80000000 | (hi << 16) | lo]
    u += [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff,      # +-0, +-inf, +-FLT_MAX (-> +-inf)
          0x7f7f8000, 0x7f7f7fff,                                                     # the largest tie (-> inf) and below it
          0x00000001, 0x00008000, 0x00008001, 0x00010000, 0x0001ffff, 0x007fffff, 0x80000001, 0x80008000,    # bf16 subnormals
          0x7fc00000, 0xffc00001, 0x7f800001]                                          # NaNs: compared with isnan only
    return np.array(u, dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("n", [1, 7, 257, 2097152 + 261])               # the grid stride starts at 8192 * 256 elements
def test_f32_to_bf16_equals_torch(lib, n):
    """bit for bit torch.Tensor.to(torch.bfloat16) (round to nearest even, pinned by the host tests): random normals, exact
    ties with even and odd upper halves in both signs, just above and below a tie, +-0, +-inf, +-FLT_MAX -> +-inf, the
    bf16-subnormal range; NaN compared with isnan only"""
    rng = np.random.Generator(np.random.PCG64(53 + n))
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-140, 120, n))).astype(np.float32)
    sp = _bf16_specials()
    if n == 1:
        x[0] = np.array([0x3f818000], dtype=np.uint32).view(np.float32)[0]
    else:
        k = min(n, sp.size)
        x[:k] = sp[:k]
        if n >= 2 * sp.size:
            x[-sp.size:] = sp                                       # the tail of the last grid-stride trip
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    fin = ~np.isnan(x)
    assert np.array_equal(want[fin], R.bf16_rne_bits(x)[fin])
    out = torch.full((n + GUARD,), 0x7fc1, dtype=torch.int16, device="cuda")             # a NaN pattern the kernel never makes
    xd = _dev(x)
    _ok(lib.mseg_f32_to_bf16(xd.data_ptr(), out.data_ptr(), n, _stream()))
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint16)
    assert (host[n:] == 0x7fc1).all(), "the kernel wrote behind its output"
    got = host[:n]
    bad = np.flatnonzero((got != want) & fin)
    assert bad.size == 0, (f"{bad.size} of {n} differ, first at {bad[0]}: {x.view(np.uint32)[bad[0]]:#010x} -> "
                           f"{got[bad[0]]:#06x}, torch {want[bad[0]]:#06x}")
    assert np.isnan(R.bf16_bits_to_f64(got[~fin])).all()


# =================================================================================================================================
# weight repack
# =================================================================================================================================
def _pack_jobs():
    """(id, weight shape, T, R, Rpad, C, Cpad, st, sr, sc): the four stride sets of the engine — 3x3 forward, 3x3 data
    gradient, ConvTranspose forward (taps merged: Rpad = R) and ConvTranspose data gradient — with R and C off the padding
    (Rpad % 128 == 0, Cpad % 32 == 0) and at it; the 384 x 320 forward operand has more elements than the 4096 * 256 threads of
    the capped grid"""
    up = lambda v, m: (v + m - 1) // m * m
    jobs = []
    for co, ci in ((40, 72), (128, 96), (384, 320)):
        jobs.append((f"conv-fwd-{co}x{ci}", (co, ci, 3, 3), 9, co, up(co, 128), ci, up(ci, 32), 1, ci * 9, 9))
        if co < 384:
            jobs.append((f"conv-dgrad-{co}x{ci}", (co, ci, 3, 3), 9, ci, up(ci, 128), co, up(co, 32), 1, 9, ci * 9))
    for ci, co in ((24, 40), (128, 64)):
        jobs.append((f"up-fwd-{ci}x{co}", (ci, co, 2, 2), 4, co, co, ci, up(ci, 32), 1, 4, co * 4))
        jobs.append((f"up-dgrad-{ci}x{co}", (ci, co, 2, 2), 4, ci, up(ci, 128), co, up(co, 32), 1, co * 4, 4))
    return jobs


def _pack_weight(shape):
    rng = np.random.Generator(np.random.PCG64(61 + sum(shape)))
    w = rng.standard_normal(shape).astype(np.float32)
    w.reshape(-1)[::97] = -0.0                       # a padded element must be +0 whatever the weights hold
    return w


def _check_packed(got, ref, T, R, Rpad, Cc, Cpad):
    assert not np.isnan(got).any(), "an element of the operand was left unwritten"
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    inside = np.zeros((T, Rpad, Cpad), dtype=bool)
    inside[:, :R, :Cc] = True
    assert (got.reshape(T, Rpad, Cpad).view(np.uint32)[~inside] == 0).all(), "a pad element is not +0.0"


@pytest.mark.parametrize("job", _pack_jobs(), ids=lambda j: j[0])
def test_pack_weight_equals_header_layout(lib, job):
    """dst[(t Rpad + r) Cpad + c] = (r < R && c < C) ? src[t st + r sr + c sc] : 0 into a NaN-filled buffer: equal to the numpy
    construction bit for bit, every pad element +0.0, no NaN left, nothing written behind T Rpad Cpad"""
    _, shape, T, Rr, Rpad, Cc, Cpad, st, sr, sc = job
    w = _pack_weight(shape)
    ref = R.pack_weight(w, T, Rr, Rpad, Cc, Cpad, st, sr, sc)
    n = T * Rpad * Cpad
    out, wd = _nan_buf(n), _dev(w)
    _ok(lib.mseg_pack_weight(wd.data_ptr(), out.data_ptr(), T, Rr, Rpad, Cc, Cpad, st, sr, sc, _stream()))
    _check_packed(_take(out, n).numpy(), ref, T, Rr, Rpad, Cc, Cpad)


@pytest.mark.parametrize("job", [j for j in _pack_jobs() if j[0] in ("conv-fwd-40x72", "conv-dgrad-40x72", "up-fwd-24x40",
                                                                      "up-dgrad-24x40")], ids=lambda j: j[0])
def test_pack_weights_multi_one_job_with_bf16(lib, job):
    """one mseg_pack_weights_multi job with dst16 set: dst equals the header's layout as above, dst16 its RNE bf16"""
    from microbeseg_amd import _lib
    _, shape, T, Rr, Rpad, Cc, Cpad, st, sr, sc = job
    w = _pack_weight(shape)
    ref = R.pack_weight(w, T, Rr, Rpad, Cc, Cpad, st, sr, sc)
    n = T * Rpad * Cpad
    wd, out = _dev(w), _nan_buf(n)
    out16 = torch.full((n + GUARD,), 0x7fc1, dtype=torch.int16, device="cuda")
    j = _lib.MsegPackJob()
    j.src, j.dst, j.dst16 = wd.data_ptr(), out.data_ptr(), out16.data_ptr()
    j.T, j.R, j.Rpad, j.C, j.Cpad, j.st, j.sr, j.sc = T, Rr, Rpad, Cc, Cpad, st, sr, sc
    j.first_block = 0
    blocks = lib.mseg_pack_job_blocks(T, Rpad, Cpad)
    assert blocks == ((Rpad + 31) // 32) * ((Cpad + 31) // 32)
    tab = torch.frombuffer(bytearray(bytes(j)), dtype=torch.uint8).cuda()
    _ok(lib.mseg_pack_weights_multi(tab.data_ptr(), 1, blocks, _stream()))
    _check_packed(_take(out, n).numpy(), ref, T, Rr, Rpad, Cc, Cpad)
    host16 = out16.cpu().numpy().view(np.uint16)
    assert (host16[n:] == 0x7fc1).all(), "the kernel wrote behind dst16"
    assert np.array_equal(host16[:n], R.bf16_rne_bits(ref))
