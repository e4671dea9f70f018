"""CPU: the fp64 reference of tests/norm_ref.py against torch on the CPU in fp64 — F.batch_norm, F.group_norm(., 8, .) and
F.instance_norm applied to act(z), autograd for every gradient — so that tests/test_gpu_norm.py measures the kernels against
something that is itself pinned.

Agreement: 1e-12 relative, element by element, for the tables; where a reference value is exactly 0, 1e-12 of the largest
entry.  The sums (mean, dgamma, dbeta, dbias) are held to 1e-12 of the sum of the absolute values of their terms: they cancel —
the bias gradient in front of Batch / InstanceNorm without an activation is 0 analytically and holds nothing but the rounding of
its terms — and no formula error hides below that scale.  dz is compared per (sample, channel) plane — the maximum
error of the plane against its largest entry with the floor |k1| max|gy|, the measure of the GPU test — because single entries
cancel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as NR
import pointwise_ref as R

REL = 1e-12
EPS, MOMENTUM = 1e-5, 0.1
# (N, HW as (H, W), C): HW == 1, N == 1, C / 8 == 3 and 9, several samples with C / 8 == 2
SHAPES = [(2, (1, 1), 24), (1, (2, 3), 72), (3, (5, 1), 16), (4, (3, 3), 8)]


def _torch_act(x, act):
    return {"none": lambda v: v, "relu": F.relu, "leakyrelu": lambda v: F.leaky_relu(v, 0.01), "elu": F.elu,
            "mish": lambda v: v * torch.tanh(F.softplus(v))}[act](x)


def _inputs(N, H, W, Cc, seed=0):
    g = torch.Generator().manual_seed(100 + seed + N + 10 * H * W + 1000 * Cc)
    z = torch.randn(N, H, W, Cc, generator=g, dtype=torch.float64) * 1.5 + 0.3
    z[0, 0, 0, 0] = 0.0                                  # the derivative conventions at z == 0
    z[-1, -1, -1, 1] = 19.5                              # both sides of the softplus threshold
    z[-1, -1, -1, 2] = 20.5
    gy = torch.randn(N, H, W, Cc, generator=g, dtype=torch.float64)
    gamma = torch.randn(Cc, generator=g, dtype=torch.float64) * 0.3 + 1
    gamma[0], gamma[Cc - 1] = -0.7, 0.0
    beta = torch.randn(Cc, generator=g, dtype=torch.float64) * 0.1
    rm = torch.randn(Cc, generator=g, dtype=torch.float64) * 0.1
    rv = torch.rand(Cc, generator=g, dtype=torch.float64) + 0.5
    return z, gy, gamma, beta, rm, rv


def _close(got, want, terms=None, what=""):
    """element by element: 1e-12 |want|; a SUM (``terms`` = the sum of the absolute values of its terms) 1e-12 of that scale"""
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    err = (got - want).abs()
    if terms is None:
        bound = torch.where(want == 0, REL * want.abs().max(), REL * want.abs())
    else:
        bound = REL * torch.as_tensor(terms, dtype=torch.float64) * torch.ones_like(want)
    bad = torch.nonzero(err > bound)
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} off, first {bad[0].tolist()}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def _planes_close(got, want, k1, gy, what):
    """[N][HW][C]: max error of a (sample, channel) plane <= 1e-12 of its largest entry, or of |k1| max|gy| of the plane (the scale
    of the terms that cancel in dz = k1 gy + k2 a + k3; with two values per statistic they cancel almost completely)"""
    err = (got - want).abs().amax(dim=1)
    top = torch.maximum(want.abs().amax(dim=1), k1.abs() * gy.abs().amax(dim=1))
    assert (err <= REL * top).all(), f"{what}: {(err / torch.clamp(top, min=1e-300)).max().item():.3e}"


# running statistics (BatchNorm only): absent and given
NORM_CASES = [("bn", False), ("bn", True), ("gn", False), ("in", False)]


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("norm,running", NORM_CASES)
@pytest.mark.parametrize("N,hw,Cc", SHAPES)
def test_reference_equals_torch(N, hw, Cc, norm, running, act):
    H, W = hw
    z, gy, gamma, beta, rm, rv = _inputs(N, H, W, Cc)
    # torch's NCHW, contiguous (F.instance_norm misreads a one-sample tensor with channels-last strides)
    zt = z.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a = _torch_act(zt, act)
    rm_t, rv_t = rm.clone(), rv.clone()
    if norm == "bn":
        y = F.batch_norm(a, rm_t if running else None, rv_t if running else None, gt, bt, True, MOMENTUM, EPS)
    elif norm == "gn":
        y = F.group_norm(a, 8, gt, bt, EPS)
    elif H * W > 1:
        y = F.instance_norm(a, eps=EPS)
    else:
        y = F.group_norm(a, Cc, None, None, EPS)          # F.instance_norm refuses one pixel; one group per channel is the same
    y.backward(gy.permute(0, 3, 1, 2).contiguous())
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(N, H * W, Cc)

    z3, gy3 = z.reshape(N, H * W, Cc), gy.reshape(N, H * W, Cc)
    fw = NR.forward(z3, act, norm, gamma, beta, EPS, MOMENTUM, rm if running else None, rv if running else None)
    sc = fw["scale"] if norm != "bn" else fw["scale"][None]
    sh = fw["shift"] if norm != "bn" else fw["shift"][None]
    assert fw["scale"].shape == ((Cc,) if norm == "bn" else (N, Cc))
    assert fw["mean"].shape == {"bn": (Cc,), "gn": (N, 8), "in": (N, Cc)}[norm] == fw["rstd"].shape
    y_ref = fw["a"] * sc[:, None, :] + sh[:, None, :]
    terms = fw["a"].abs() * sc.abs()[:, None, :] + sh.abs()[:, None, :]
    want_y = flat(y.detach())
    assert ((y_ref - want_y).abs() <= REL * terms).all(), "a * scale + shift is not the normalised tensor"
    # mean / rstd against the statistics of torch's activated tensor
    ad = flat(a.detach())
    f = NR._fold(ad, norm)
    _close(fw["mean"].reshape(-1), f.mean(dim=(1, 3)).reshape(-1), terms=f.abs().mean(dim=(1, 3)).reshape(-1), what="mean")
    _close(fw["rstd"].reshape(-1), (1.0 / torch.sqrt(f.var(dim=(1, 3), unbiased=False) + EPS)).reshape(-1), what="rstd")
    if running:
        _close(fw["running_mean"], rm_t, what="running_mean")
        _close(fw["running_var"], rv_t, what="running_var")
    else:
        assert "running_mean" not in fw

    bw = NR.backward(gy3, z3, act, norm, gamma, EPS)
    _planes_close(bw["dz"], flat(zt.grad), bw["k1"], gy3, "dz")
    assert bw["dz_stored"] is bw["dz"]
    _close(bw["dbias"], flat(zt.grad).sum(dim=(0, 1)), terms=bw["dbias_terms"], what="dbias")
    if norm != "in":
        _close(bw["dgamma"], gt.grad, terms=bw["dgamma_terms"], what="dgamma")
        _close(bw["dbeta"], bt.grad, terms=bw["dbeta_terms"], what="dbeta")
    assert (bw["dz_terms"] >= bw["dz"].abs() * (1 - 1e-9)).all()


def test_one_pixel_per_statistic():
    """count == 1: mean = a, var = 0, rstd = 1 / sqrt(eps), y = beta, every gradient but dbeta is 0; the running variance takes
    the variance 0 without the count / (count - 1) correction (torch refuses the case)"""
    z, gy, gamma, beta, rm, rv = _inputs(1, 1, 1, 8)
    z3, gy3 = z.reshape(1, 1, 8), gy.reshape(1, 1, 8)
    for norm in ("bn", "in"):
        fw = NR.forward(z3, "elu", norm, gamma, beta, EPS, MOMENTUM, rm, rv)
        a = R.activation(z3, "elu").reshape(-1)
        assert torch.equal(fw["mean"].reshape(-1), a) and torch.equal(fw["var"].reshape(-1), torch.zeros(8, dtype=torch.float64))
        assert torch.equal(fw["rstd"].reshape(-1), torch.full((8,), 1.0 / np.sqrt(EPS), dtype=torch.float64))
        bw = NR.backward(gy3, z3, "elu", norm, gamma, EPS)
        assert torch.equal(bw["dz"], torch.zeros_like(bw["dz"])) and torch.equal(bw["dgamma"], torch.zeros(8, dtype=torch.float64))
        assert torch.equal(bw["dbeta"], gy3.reshape(-1))
        if norm == "bn":
            assert torch.isfinite(fw["running_var"]).all()
            assert torch.equal(fw["running_var"], (1.0 - MOMENTUM) * rv)
            assert torch.equal(fw["running_mean"], (1.0 - MOMENTUM) * rm + MOMENTUM * a)


def test_instance_norm_ignores_the_affine_parameters():
    z, gy, gamma, beta, _, _ = _inputs(2, 3, 2, 8)
    z3 = z.reshape(2, 6, 8)
    a, b = NR.forward(z3, "relu", "in", gamma, beta), NR.forward(z3, "relu", "in")
    assert torch.equal(a["scale"], b["scale"]) and torch.equal(a["shift"], b["shift"])


def test_activation_derivative_conventions():
    """at z == 0: ReLU 0, LeakyReLU the slope, ELU exp(0) = 1; Mish on both sides of the softplus threshold; everything equal to
    torch's autograd"""
    z = torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 1.7, -1.7, 19.5, 20.0, 20.5, 60.0, -60.0], dtype=torch.float64)
    at0 = {"none": 1.0, "relu": 0.0, "leakyrelu": 0.01, "elu": 1.0, "mish": 0.6}
    for i, act in enumerate(R.ACTS):
        zt = z.clone().requires_grad_(True)
        _torch_act(zt, act).sum().backward()
        d = NR.activation_grad(z, act)
        assert torch.equal(d, NR.activation_grad(z, i))
        assert d[0].item() == at0[act] and d[1].item() == at0[act], act
        assert ((d - zt.grad).abs() <= 1e-15 * zt.grad.abs()).all(), act
    m = NR.activation_grad(z, "mish")
    # up to the threshold softplus' = sigmoid: at 19.5 and 20 the derivative is not yet 1; above it, it is tanh(z) + z sech^2(z)
    s = lambda x: np.tanh(np.log1p(np.exp(x))) + x * (1 - np.tanh(np.log1p(np.exp(x))) ** 2) / (1 + np.exp(-x))
    assert m[6].item() == pytest.approx(s(19.5), rel=1e-15) and m[7].item() == pytest.approx(s(20.0), rel=1e-15)
    assert m[8].item() == pytest.approx(np.tanh(20.5) + 20.5 * (1 - np.tanh(20.5) ** 2), rel=1e-15) and m[9].item() == 1.0
    f32 = NR.activation_grad(z, "elu", dtype=torch.float32)
    assert f32.dtype == torch.float32 and f32[0].item() == 1.0


def test_bf16_storage_contract():
    """one channel pair, hand-made: the materialised activation is rounded BEFORE the statistics (1 + 2^-9 is not a bf16 number
    and rounds to 1: the channel becomes constant), the not-materialised one is not; dz is rounded when stored and dbias is the
    sum of the rounded values"""
    h = 2.0 ** -9
    z = torch.tensor([[[1.0 + h, 3.0], [1.0, 5.0], [1.0 + h, 7.0], [1.0, 9.0]]], dtype=torch.float64)       # [1][4][2]
    assert torch.equal(NR.bf16_store(z)[0, :, 0], torch.ones(4, dtype=torch.float64))
    assert torch.equal(NR.bf16_store(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)), torch.tensor([1 + 2.0 ** -7], dtype=torch.float64))
    plain = NR.forward(z, "none", "in", bf16=True, materialised=False)
    mat = NR.forward(z, "none", "in", bf16=True, materialised=True)
    assert plain["mean"][0, 0].item() == 1.0 + h / 2 and plain["var"][0, 0].item() == h * h / 4
    assert mat["mean"][0, 0].item() == 1.0 and mat["var"][0, 0].item() == 0.0
    assert mat["rstd"][0, 0].item() == 1.0 / np.sqrt(1e-5)
    assert torch.equal(mat["a"][0, :, 0], torch.ones(4, dtype=torch.float64))
    assert mat["mean"][0, 1].item() == 6.0 and mat["var"][0, 1].item() == 5.0       # bf16 numbers pass unchanged
    given = NR.forward(z, "none", "in", bf16=True, materialised=True, a=z)            # a stored tensor is taken as it is
    assert given["mean"][0, 0].item() == 1.0 + h / 2
    # backward: the sums over rounded values
    gy = torch.tensor([[[0.5, 1.0], [-0.25, 0.125], [1.5, -2.0], [0.75, 3.0]]], dtype=torch.float64)
    gamma = torch.tensor([1.0, 0.3], dtype=torch.float64)
    exact = NR.backward(gy, z, "none", "bn", gamma)
    b = NR.backward(gy, z, "none", "bn", gamma, bf16=True)
    assert torch.equal(b["dz"], exact["dz"])
    assert torch.equal(b["dz_stored"], NR.bf16_store(exact["dz"])) and not torch.equal(b["dz_stored"], b["dz"])
    assert torch.equal(b["dbias"], b["dz_stored"].sum(dim=(0, 1)))
    assert not torch.equal(b["dbias"], exact["dbias"])
    assert torch.equal(exact["dbias"], exact["dz"].sum(dim=(0, 1)))
    # the materialised activation of the backward is the rounded one: channel 0 is constant, xhat = 0, dgamma = 0
    bm = NR.backward(gy, z, "none", "bn", gamma, bf16=True, materialised=True)
    assert bm["dgamma"][0].item() == 0.0 and b["dgamma"][0].item() != 0.0


def test_tables_from_partial_sums():
    """part[rows][2][C] of a tensor's rows give the tables of forward() on that tensor (E[a^2] - mean^2 against the two-pass
    variance: agreement to the conditioning of the subtraction, (1 + mean^2 / var) 2^-52)"""
    g = torch.Generator().manual_seed(5)
    rows, k, Cc = 7, 11, 8
    a = torch.randn(rows, k, Cc, generator=g, dtype=torch.float64) * 1.5 + 0.3
    part = torch.stack([a.sum(dim=1), (a * a).sum(dim=1)], dim=1)
    gamma, beta = torch.randn(Cc, generator=g, dtype=torch.float64), torch.randn(Cc, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(Cc, generator=g, dtype=torch.float64), torch.rand(Cc, generator=g, dtype=torch.float64) + 0.5
    want = NR.forward(a.reshape(1, rows * k, Cc), "none", "bn", gamma, beta, EPS, MOMENTUM, rm, rv)
    got = NR.forward_from_partials(part, rows * k, gamma, beta, EPS, MOMENTUM, rm, rv)
    for key in ("scale", "mean", "rstd", "running_mean", "running_var"):
        assert ((got[key] - want[key]).abs() <= 1e-13 * want[key].abs()).all(), key
    assert ((got["shift"] - want["shift"]).abs() <= 1e-13 * want["shift_terms"]).all()
    # a constant channel: the subtraction may go negative by rounding and is clamped
    c = torch.full((3, 2, 4), 100.7, dtype=torch.float64).to(torch.float32).to(torch.float64)
    cp = torch.stack([c.sum(dim=1) * (1 + 2.0 ** -40), (c * c).sum(dim=1)], dim=1)
    assert (NR.forward_from_partials(cp, 6)["var"] == 0).all()
