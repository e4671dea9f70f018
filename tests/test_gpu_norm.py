"""GPU (MI355X): the normalisation kernels of csrc/norm.hip — mseg_norm_stats, mseg_norm_bwd, mseg_norm_stats_from_conv —
through the C ABI against the fp64 reference of tests/norm_ref.py (which tests/test_norm_ref_host.py pins to torch), per
channel, per (sample, group) and per (sample, channel) plane instead of per tensor: a wrong table for one small channel or one
(sample, group) cannot hide under the largest entry of the tensor.

Shapes: the smallest (N, HW, C) that reach each geometry of norm_geom — a non-power-of-two number of channel groups per
workgroup (with idle threads), several channel slices with a ragged last one, GroupNorm groups that straddle a thread's vector
and a slice boundary, more than 128 per-sample groups, the 1024-thread and the two-round forms of the finishing kernel, HW = 1 —
asserted by test_geometry_of_the_shapes with a copy of that arithmetic, so that a retuned geometry says which shapes to re-pick.

Measures, each relative to the quantity's OWN scale.  A table entry: |got - ref| / |ref|; shift against |beta| + |mean gamma rstd|
and the updated running mean against |(1 - momentum) old| + |momentum mean|, the terms they are the sum of.  A sum (mean, dgamma, dbeta, dbias): |got - ref| / the sum of the absolute values of its
terms — the relative error where nothing cancels, and the only scale a sum's rounding knows where it does: dbeta of N(0, 1)
gradients is ~ sqrt(M) with terms ~ M, the bias gradient in front of Batch / InstanceNorm without an activation is 0
analytically, and an entry-wise relative error there would measure the draw, not the kernel.  A wrong table, group or slice
still misses by ~ M^-1/2 of that scale, 1e-2 at these shapes, against bounds near 1e-6.  dz: per (sample, channel) plane,
max|got - ref| / max(max|ref|, |k1| max|gy|) of the plane (dz = (k1 gy + k2 a + k3) act'(z): a plane whose terms cancel — one
live pixel, gamma = 0 under GroupNorm — is held to the scale of its terms, one that is 0 exactly must be 0).
Bounds.  The suite's rule e_hip <= max(4 e_ref, floor constant): e_ref = the same measure of the SAME reference formulas
evaluated in fp32 on the CPU; the floor constants were measured on the first run on the MI355X and are documented where they are
defined.  The statistics also meet the a-priori bound of their arithmetic (fp32 sums of at most 8 values per trip, fp64 above:
|var - var_ref| <= 8 * 2^-24 (var + mean^2) + the fp32 rounding of the stored rstd), whatever the inputs' mean / std ratio.
bf16 storage: the tables are taken over the values as stored and keep the fp32 bounds; dz gets 2^-8 |ref| per element on top;
dbias is compared with the fp64 sum of the dz the kernel RETURNED.  Where bf16 storage materialises the activation, the
reference takes its statistics over the returned act_out — which is itself held to 2^-8 |ref| + 2^-133 of the reference
activation: its one-ulp freedom at a rounding tie is not the statistics' error.
Every output carries a NaN guard band; every case runs the backward with dz aliasing gy and apart, bit for bit equal."""
import collections
import functools
import itertools

import numpy as np
import pytest
import torch

import norm_ref as NR
import pointwise_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24             # unit roundoff of fp32
GUARD = 64                 # elements of guard band behind an output
EINVAL = -1
NAN = float("nan")
EPS = float(np.float32(1e-5))          # the fp32 numbers the library receives
MOMENTUM = float(np.float32(0.1))
RSTD0 = np.float32(1.0 / np.sqrt(EPS))  # rstd of a statistic with variance 0

# (N, HW, C) per storage; see test_geometry_of_the_shapes for what each one reaches
F32_SHAPES = [(1, 1, 4), (3, 7, 8), (2, 4160, 4), (2, 1400, 12), (3, 255, 24), (2, 391, 40), (2, 1023, 64), (2, 1023, 72),
              (3, 300, 136), (9, 130, 260), (2, 600, 132), (65, 5, 16)]
BF16_SHAPES = [(1, 1, 8), (2, 2100, 24), (2, 1023, 72), (3, 513, 128), (2, 300, 136), (9, 130, 264), (65, 5, 16)]
SHAPES = {"f32": F32_SHAPES, "bf16": BF16_SHAPES}
ONLY_NORMS = {("f32", (9, 130, 260)): ("bn", "in"), ("f32", (2, 600, 132)): ("in",)}
EXPENSIVE_AT = {"f32": (12, 64, 72), "bf16": (24, 72, 128)}         # channel counts that also run leakyrelu, elu, mish
ROUTE_AT = {"f32": (12, 72, 136, 260), "bf16": (72, 136)}           # channel counts that also run the alternative routes
ROUTES = [("finish0", 0, 0), ("finish1", 0, 1), ("finish2", 0, 2), ("tails", 1, -1)]      # (name, set_tails, set_finish)

# ---- floor constants of e_hip <= max(4 e_ref, floor), measured on the first run on the MI355X -----------------------------------
# All cases of this file (both storages, every route).  4 e_ref was the working bound in every case but eight (dgamma where
# torch's fp32 happened to round well, e_hip <= 3.9e-8 there); the largest e_hip / max(4 e_ref, floor) of a quantity was 0.33.
# The floors only catch such draws and the entries a reference computes exactly; each is below twice the largest e_hip seen.
#   scale, rstd: e_ref 4.2e-8 .. 5.3e-6, e_hip 2.5e-8 .. 1.74e-7 (worst: fp32 (65, 5, 16) in none, five values per statistic:
#     e_ref 1.61e-7, e_hip 1.74e-7 — the one-pass variance at 2^-24 (1 + mean^2 / var) and the rounding of the stored number);
#   shift: e_hip 5.2e-9 .. 7.4e-8 but for InstanceNorm without an activation, whose measure |mean rstd| itself cancels:
#     fp32 (9, 130, 260): e_ref 6.65e-5, e_hip 3.62e-5 (4 e_ref binds); running_mean / running_var: e_ref 3.0e-8 .. 1.7e-7,
#     e_hip 2.9e-8 .. 6.2e-8.
# 3e-7 = 5 u: the rounding of the stored fp32 number (1 u) on top of the statistics' own error.
TABLE_FLOOR = 3e-7
#   mean: e_ref 0 .. 1.4e-6, e_hip 0 .. 7.7e-8; dgamma: e_ref 0 .. 2.7e-7, e_hip 0 .. 5.7e-8 (worst: fp32 (3, 7, 8) bn none);
#   dbeta: e_ref 0 .. 2.4e-8, e_hip 0 .. 2.4e-8; dbias (fp32 storage): e_ref 0 .. 6.2e-7, e_hip 0 .. 1.17e-7 (worst: fp32
#   (2, 1023, 72) gn relu, e_ref 3.4e-7 there).  fp64 sums of fp32 trip sums: the kernels sit at 1 - 2 u of the terms' scale.
# 2e-7 = 3 u.
SUM_FLOOR = 2e-7
#   dz per plane: fp32 storage e_ref 0 .. 3.4e-6, e_hip 0 .. 6.33e-7 (worst: (2, 1023, 72) gn elu stored, e_ref 3.40e-6 there: the
#   plane of the single live pixel, where k1 gy + k2 a + k3 cancels to 1 / count of its terms); bf16 storage, beyond the 2^-8 |ref|
#   of the stored rounding: e_ref 0 .. 1.8e-7, e_hip 0 .. 8.6e-8 (worst: (65, 5, 16) in relu).
# 1e-6 = 17 u, 1.6 x the largest e_hip: three fp32 tables, two multiply-adds, act'(z) (expf and a division for mish) and a product.
DZ_FLOOR = 1e-6
ACT_FLOOR = 5e-7           # test_gpu_pointwise.test_activation_fp32: |got - ref| <= max(4 e_ref, 5e-7) max(|ref|, 2^-20)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from microbeseg_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan_buf(n, dtype=torch.float32):
    """n output elements + the guard band, all NaN"""
    return torch.full((n + GUARD,), NAN, dtype=dtype, device="cuda")


def _take(buf, n, what):
    """-> the n output elements on the CPU as fp64, after checking that the guard band still holds its NaNs and the payload none"""
    host = buf.cpu()
    assert torch.isnan(host[n:].float()).all(), f"{what}: the kernel wrote behind its output"
    out = host[:n].double()
    assert torch.isfinite(out).all(), f"{what}: {int((~torch.isfinite(out)).sum())} of {n} elements are not finite"
    return out


def _workspace(lib, N, HW, Cc):
    return torch.zeros(lib.mseg_norm_workspace_bytes(N, HW, Cc), dtype=torch.uint8, device="cuda")     # counters: zero once


# =================================================================================================================================
# the geometry the shapes were chosen for
# =================================================================================================================================
def norm_geom(N, HW, Cc, vec):
    """a copy of the arithmetic of norm_geom in csrc/norm.hip: a workgroup = 256 threads = rpi row slots x cw channel groups of
    `vec` channels (4: fp32 storage, 8: bf16), one per (chunk of rows, sample, slice of <= 16 channel groups)"""
    c4 = Cc // vec
    cw = (c4 if c4 > 0 else 1) if c4 < 16 else 16
    slices = (c4 + cw - 1) // cw
    rpi = 256 // cw
    want = (1024 + N * slices - 1) // (N * slices)
    chunks = max(1, min(HW // (8 * rpi), want))
    rows = (HW + chunks - 1) // chunks
    chunks = (HW + rows - 1) // rows
    return {"cw": cw, "slices": slices, "rpi": rpi, "idle": 256 - rpi * cw, "chunks": chunks, "rows": rows,
            "last_slice": c4 - (slices - 1) * cw, "last_chunk": HW - (chunks - 1) * rows, "pow2": cw & (cw - 1) == 0}


def test_geometry_of_the_shapes():
    """what each shape is in the list for; if this fails, norm_geom was retuned: pick shapes that reach the same paths again"""
    g = lambda st, shape: norm_geom(*shape, 4 if st == "f32" else 8)
    sub = lambda d, **kw: all(d[k] == v for k, v in kw.items())
    # fp32 storage
    assert sub(g("f32", (1, 1, 4)), cw=1, chunks=1) and sub(g("f32", (3, 7, 8)), cw=2, chunks=1, rpi=128)         # HW < row slots
    assert sub(g("f32", (2, 4160, 4)), cw=1, slices=1, chunks=2)
    assert sub(g("f32", (2, 1400, 12)), cw=3, pow2=False, idle=1, chunks=2)
    assert sub(g("f32", (3, 255, 24)), cw=6, pow2=False, idle=4) and 24 // 8 == 3
    assert sub(g("f32", (2, 391, 40)), cw=10, pow2=False, idle=6) and 40 // 8 == 5
    assert sub(g("f32", (2, 1023, 64)), cw=16, slices=1, chunks=7, rows=147, last_chunk=141)
    assert sub(g("f32", (2, 1023, 72)), cw=16, slices=2, last_slice=2, chunks=7) and 72 // 8 == 9 and 63 < 64 < 71      # group 7
    assert sub(g("f32", (3, 300, 136)), cw=16, slices=3, last_slice=2, chunks=2) and 136 // 8 == 17
    assert sub(g("f32", (9, 130, 260)), slices=5, last_slice=1) and 9 > 8 and 260 > 256 and 260 > 128
    assert sub(g("f32", (2, 600, 132)), slices=3, last_slice=1) and 132 > 128 and 132 % 8
    assert sub(g("f32", (65, 5, 16)), cw=4, chunks=1) and 65 > 64
    # bf16 storage
    assert sub(g("bf16", (1, 1, 8)), cw=1, chunks=1)
    assert sub(g("bf16", (2, 2100, 24)), cw=3, pow2=False, idle=1, chunks=3)
    assert sub(g("bf16", (2, 1023, 72)), cw=9, pow2=False, idle=4, slices=1) and 72 // 8 == 9
    assert sub(g("bf16", (3, 513, 128)), cw=16, slices=1, chunks=4, rows=129, last_chunk=126)
    assert sub(g("bf16", (2, 300, 136)), cw=16, slices=2, last_slice=1)
    assert sub(g("bf16", (9, 130, 264)), slices=3, last_slice=1) and 264 > 256
    assert sub(g("bf16", (65, 5, 16)), cw=2, chunks=1)
    for st in SHAPES:
        for shape in SHAPES[st]:
            assert shape[0] * shape[1] * shape[2] < 350000


# =================================================================================================================================
# inputs and references
# =================================================================================================================================
Case = collections.namedtuple("Case", "st shape z gy gamma beta rm rv dead single")


@functools.lru_cache(maxsize=None)
def _case(st, shape):
    """z ~ 1.5 N(0, 1) + 0.3 and gy ~ N(0, 1) [N][HW][C] (bf16 numbers for bf16 storage), with planted cases: channel 1 is <= 0
    everywhere (a dead ReLU channel), channel 2 has ONE non-zero pixel, exact zeros all over (the derivative conventions at
    z == 0), 19.5 and 20.5 (the two sides of Mish's softplus threshold); gamma with a negative first and an exactly zero last
    entry; non-trivial running statistics"""
    N, HW, Cc = shape
    rng = np.random.Generator(np.random.PCG64(7 + N + 10 * HW + 100000 * Cc + (st == "bf16")))
    z = (rng.standard_normal((N, HW, Cc)) * 1.5 + 0.3).astype(np.float32)
    z.reshape(-1)[::7] = 0.0
    dead, single = 1, 2
    z[:, :, dead] = -np.abs(z[:, :, dead])
    z[:, :, single] = 0.0
    # (HW == 1: a value whose fp32 square rounds UP, by 1.8e-7 against eps = 1e-5: E[a^2] - mean^2 of ONE value is that rounding,
    # and rstd comes out 0.9 % low unless a statistic over one value is given the variance 0)
    z[N - 1, HW // 2, single] = 2.5 if HW > 1 else 2.7
    z[0, 0, 0], z[0, HW - 1, Cc - 1] = 19.5, 20.5
    gy = rng.standard_normal((N, HW, Cc)).astype(np.float32)
    zt, gt = torch.from_numpy(z), torch.from_numpy(gy)
    if st == "bf16":
        zt, gt = zt.to(torch.bfloat16).float(), gt.to(torch.bfloat16).float()
    assert (zt[:, :, dead] <= 0).all() and int((zt[:, :, single] != 0).sum()) == 1 and ((zt == 0).sum() > N * HW or HW == 1)
    gamma = (rng.standard_normal(Cc) * 0.3 + 1).astype(np.float32)
    gamma[0], gamma[Cc - 1] = -0.7, 0.0
    beta = (rng.standard_normal(Cc) * 0.1).astype(np.float32)
    rm = (rng.standard_normal(Cc) * 0.1).astype(np.float32)
    rv = (rng.random(Cc) + 0.5).astype(np.float32)
    return Case(st, shape, zt, gt, *(torch.from_numpy(v) for v in (gamma, beta, rm, rv)), dead, single)


def _reference(case, norm, act, mat, a=None, dtype=torch.float64):
    """(forward, backward) of tests/norm_ref.py; ``a``: the stored activation the statistics are to be taken over"""
    bf16 = case.st == "bf16"
    run = norm == "bn"
    fw = NR.forward(case.z, act, norm, case.gamma, case.beta, EPS, MOMENTUM, case.rm if run else None, case.rv if run else None,
                    bf16=bf16, materialised=mat, a=a, dtype=dtype)
    bw = NR.backward(case.gy, case.z, act, norm, case.gamma, EPS, bf16=bf16, materialised=mat, a=a, dtype=dtype)
    return fw, bw


@functools.lru_cache(maxsize=None)
def _reference_cached(st, shape, norm, act, mat):
    case = _case(st, shape)
    return _reference(case, norm, act, mat), _reference(case, norm, act, mat, dtype=torch.float32)


# =================================================================================================================================
# one forward + backward through the C ABI
# =================================================================================================================================
def _table_sizes(norm, N, Cc):
    return (Cc, Cc) if norm == "bn" else ((N * Cc, N * 8) if norm == "gn" else (N * Cc, N * Cc))


def _forward(lib, case, norm, act, mat, ws, z=None):
    """-> dict of CPU fp64 tensors (scale, shift, mean, rstd, running_mean, running_var, act_out) + the device buffers the
    backward reads"""
    from microbeseg_amd._lib import ACT, NORM
    N, HW, Cc = case.shape
    dt = torch.bfloat16 if case.st == "bf16" else torch.float32
    zd = (case.z if z is None else z).to(dt).cuda()
    aff = norm != "in"
    gd, bd = (case.gamma.cuda(), case.beta.cuda()) if aff else (None, None)
    rm, rv = (_nan_buf(Cc), _nan_buf(Cc)) if norm == "bn" else (None, None)
    if rm is not None:
        rm[:Cc], rv[:Cc] = case.rm.cuda(), case.rv.cuda()
    nt, ns = _table_sizes(norm, N, Cc)
    bufs = {"scale": _nan_buf(nt), "shift": _nan_buf(nt), "mean": _nan_buf(ns), "rstd": _nan_buf(ns)}
    aout = _nan_buf(N * HW * Cc, dt) if mat else None
    code = lib.mseg_norm_stats(zd.data_ptr(), N, HW, Cc, int(case.st == "bf16"), ACT[act], NORM[norm], _ptr(gd), _ptr(bd), EPS,
                               bufs["scale"].data_ptr(), bufs["shift"].data_ptr(), bufs["mean"].data_ptr(),
                               bufs["rstd"].data_ptr(), _ptr(rm), _ptr(rv), MOMENTUM, _ptr(aout), ws.data_ptr(), _stream())
    assert code == 0, f"mseg_norm_stats returned {code}"
    torch.cuda.synchronize()
    out = {k: _take(v, nt if k in ("scale", "shift") else ns, k) for k, v in bufs.items()}
    if norm != "bn":
        out = {k: v.reshape(N, -1) for k, v in out.items()}
    if rm is not None:
        out["running_mean"], out["running_var"] = _take(rm, Cc, "running_mean"), _take(rv, Cc, "running_var")
    if mat:
        out["act_out"] = _take(aout, N * HW * Cc, "act_out").reshape(N, HW, Cc)
    dev = {"z": zd, "gamma": gd, "mean": bufs["mean"], "rstd": bufs["rstd"], "act": aout}
    return out, dev


def _backward(lib, case, norm, act, dev, ws, alias):
    """-> dict of CPU tensors: dz (fp64, [N][HW][C]) and its raw bits, dgamma, dbeta (affine norms), dbias"""
    from microbeseg_amd._lib import ACT, NORM
    N, HW, Cc = case.shape
    n = N * HW * Cc
    dt = torch.bfloat16 if case.st == "bf16" else torch.float32
    aff = norm != "in"
    dg, db = (_nan_buf(Cc), _nan_buf(Cc)) if aff else (None, None)
    dbias = _nan_buf(Cc)
    dz = _nan_buf(n, dt)
    if alias:                                           # dz aliases gy, as engine.norm_bwd runs it
        dz[:n] = case.gy.to(dt).reshape(-1).cuda()
        gyd = dz
    else:
        gyd = case.gy.to(dt).cuda()
    code = lib.mseg_norm_bwd(gyd.data_ptr(), dev["z"].data_ptr(), N, HW, Cc, int(case.st == "bf16"), ACT[act], NORM[norm],
                             _ptr(dev["gamma"]), dev["mean"].data_ptr(), dev["rstd"].data_ptr(), dz.data_ptr(), _ptr(dg), _ptr(db),
                             dbias.data_ptr(), _ptr(dev["act"]), ws.data_ptr(), _stream())
    assert code == 0, f"mseg_norm_bwd returned {code}"
    torch.cuda.synchronize()
    out = {"dz": _take(dz, n, "dz").reshape(N, HW, Cc), "dbias": _take(dbias, Cc, "dbias"),
           "dz_bits": dz[:n].cpu().view(torch.int16 if case.st == "bf16" else torch.int32)}
    if aff:
        out["dgamma"], out["dbeta"] = _take(dg, Cc, "dgamma"), _take(db, Cc, "dbeta")
    return out


# =================================================================================================================================
# measures
# =================================================================================================================================
def _entry_err(x, ref, den):
    """max |x - ref| / den over the entries with den > 0; where den == 0 the value must equal the reference exactly"""
    x, ref, den = (torch.as_tensor(v, dtype=torch.float64) for v in (x, ref, den))
    den = (den if den.numel() == ref.numel() else den.expand_as(ref)).reshape(-1)
    x, ref = x.reshape(-1), ref.reshape(-1)
    err = (x - ref).abs()
    assert (err[den == 0] == 0).all(), "an entry that is exactly determined differs"
    pos = den > 0
    return (err[pos] / den[pos]).max().item() if pos.any() else 0.0


def _sum_err(x, ref, terms):
    """max |x - ref| / (the sum of the absolute values of the terms); a sum without terms must be 0"""
    return _entry_err(x, ref, torch.as_tensor(terms, dtype=torch.float64).reshape(-1))


def _plane_err(x, ref, k1, gy, slack=None):
    """dz per (sample, channel) plane: max over the planes of max|x - ref| / max(max|ref|, |k1| max|gy|); a plane without scale
    must be 0.  ``slack`` [N][HW][C]: an allowance taken off every element's error first (the bf16 rounding of dz)"""
    err = (x - ref).abs()
    if slack is not None:
        err = torch.clamp(err - slack, min=0.0)
    err = err.amax(dim=1)
    top = torch.maximum(ref.abs().amax(dim=1), (k1 if k1.dim() == 2 else k1[None]).abs() * gy.abs().amax(dim=1))
    return _entry_err(err, torch.zeros_like(err), top)


class Report:
    """collects (quantity, e_ref, e_hip, bound) lines, prints them and fails at the end with every miss, not the first"""

    def __init__(self, label):
        self.label, self.lines, self.bad = label, [], []

    def rule(self, name, e_ref, e_hip, floor):
        """e_hip <= max(4 e_ref, floor)"""
        bound = max(4 * e_ref, floor)
        self.lines.append(f"  {name}: e_ref {e_ref:.3e} e_hip {e_hip:.3e} ratio {e_hip / bound:.3f}")
        if not e_hip <= bound:
            self.bad.append(f"{name}: e_hip {e_hip:.3e} > max(4 x e_ref {e_ref:.3e}, {floor:.1e})")

    def within(self, name, value, bound):
        self.lines.append(f"  {name}: {value:.3e} of {bound:.3e} ratio {value / bound if bound > 0 else float(value > 0):.3f}")
        if not value <= bound:
            self.bad.append(f"{name}: {value:.3e} > {bound:.3e}")

    def exact(self, name, ok):
        if not ok:
            self.bad.append(f"{name}: not exact")

    def finish(self):
        print(self.label + "\n" + "\n".join(self.lines))
        assert not self.bad, self.label + ": " + "; ".join(self.bad)


def _check(rep, case, norm, act, mat, fwd, bwd, ref64, ref32):
    """every output of one forward + backward against the fp64 reference under the measures and bounds of the module docstring"""
    (f64, b64), (f32, b32) = ref64, ref32
    N, HW, Cc = case.shape
    bf16 = case.st == "bf16"
    one = torch.ones(())
    # ---- forward tables
    rep.rule("scale", _entry_err(f32["scale"], f64["scale"], f64["scale"].abs()), _entry_err(fwd["scale"], f64["scale"], f64["scale"].abs()),
             TABLE_FLOOR)
    rep.rule("shift", _entry_err(f32["shift"], f64["shift"], f64["shift_terms"]), _entry_err(fwd["shift"], f64["shift"], f64["shift_terms"]),
             TABLE_FLOOR)
    rep.rule("rstd", _entry_err(f32["rstd"], f64["rstd"], f64["rstd"]), _entry_err(fwd["rstd"], f64["rstd"], f64["rstd"]), TABLE_FLOOR)
    rep.rule("mean", _sum_err(f32["mean"], f64["mean"], f64["abs_mean"]), _sum_err(fwd["mean"], f64["mean"], f64["abs_mean"]), SUM_FLOOR)
    if norm == "bn":
        for k, den in (("running_mean", f64["running_mean_terms"]), ("running_var", f64["running_var"])):
            rep.rule(k, _entry_err(f32[k], f64[k], den), _entry_err(fwd[k], f64[k], den), TABLE_FLOOR)
    # ---- the a-priori bound of the statistics' arithmetic
    mean_slack = (fwd["mean"] - f64["mean"]).abs() - (8 * U * f64["abs_mean"] + U * f64["mean"].abs())
    rep.within("mean a-priori", max(mean_slack.max().item(), 0.0), 0.0)
    var_hip = 1.0 / fwd["rstd"] ** 2 - EPS
    var_bound = 8 * U * (f64["var"] + f64["mean"] ** 2) + (2 * U + 4 * U * U) * (f64["var"] + EPS)
    rep.within("variance a-priori (error / bound)", ((var_hip - f64["var"]).abs() / var_bound).max().item(), 1.0)
    # ---- the stored activation
    if mat:
        ref_a = R.activation(case.z, act)
        if bf16:
            rep.within("act_out (error / bound)", ((fwd["act_out"] - ref_a).abs() / (2.0 ** -8 * ref_a.abs() + 2.0 ** -133)).max().item(), 1.0)
        else:
            a32 = R.activation(case.z, act, dtype=torch.float32).double()
            den = torch.clamp(ref_a.abs(), min=2.0 ** -20)
            rep.rule("act_out", ((a32 - ref_a).abs() / den).max().item(), ((fwd["act_out"] - ref_a).abs() / den).max().item(), ACT_FLOOR)
            if act in ("none", "relu"):
                rep.exact("act_out of an exact activation", torch.equal(fwd["act_out"], ref_a))
    # ---- backward
    slack = (2.0 ** -8 * b64["dz"].abs() + 2.0 ** -133) if bf16 else None
    rep.rule("dz", _plane_err(b32["dz_stored"].double(), b64["dz"], b64["k1"], case.gy.double(), slack),
             _plane_err(bwd["dz"], b64["dz"], b64["k1"], case.gy.double(), slack), DZ_FLOOR)
    if bf16:                                            # the sum of dz AS STORED: two bf16 numbers per fp32 trip, fp64 above
        want, terms = bwd["dz"].sum(dim=(0, 1)), bwd["dz"].abs().sum(dim=(0, 1))
        rep.within("dbias - sum of the returned dz (error / 2^-23 sum|dz|)",
                   _entry_err(bwd["dbias"], want, 2 * U * terms), 1.0)
    else:
        rep.rule("dbias", _sum_err(b32["dbias"], b64["dbias"], b64["dbias_terms"]), _sum_err(bwd["dbias"], b64["dbias"], b64["dbias_terms"]),
                 SUM_FLOOR)
    if norm != "in":
        for k in ("dgamma", "dbeta"):
            rep.rule(k, _sum_err(b32[k], b64[k], b64[k + "_terms"]), _sum_err(bwd[k], b64[k], b64[k + "_terms"]), SUM_FLOOR)
    # ---- exact results
    ga, be = case.gamma.double(), case.beta.double()
    if norm == "bn":
        rep.exact("gamma == 0: scale == 0", fwd["scale"][Cc - 1].item() == 0.0)
        rep.exact("gamma == 0: shift == beta", fwd["shift"][Cc - 1].item() == be[Cc - 1].item())
    elif norm == "gn":
        rep.exact("gamma == 0: scale == 0", bool((fwd["scale"][:, Cc - 1] == 0).all()))
        rep.exact("gamma == 0: shift == beta", bool((fwd["shift"][:, Cc - 1] == be[Cc - 1]).all()))
    if act == "relu" and norm in ("bn", "in"):
        d = case.dead
        sel = (lambda t: t[d:d + 1]) if norm == "bn" else (lambda t: t[:, d])
        g_d, b_d = (ga[d].item(), be[d].item()) if norm == "bn" else (1.0, 0.0)
        rep.exact("dead channel: mean == 0", bool((sel(fwd["mean"]) == 0).all()))
        rep.exact("dead channel: rstd == 1 / sqrt(eps)", bool((sel(fwd["rstd"]) == float(RSTD0)).all()))
        rep.exact("dead channel: scale == gamma / sqrt(eps)", bool((sel(fwd["scale"]) == float(np.float32(g_d * (1.0 / np.sqrt(EPS))))).all()))
        rep.exact("dead channel: shift == beta", bool((sel(fwd["shift"]) == b_d).all()))
        rep.exact("dead channel: dz == 0", bool((bwd["dz"][:, :, d] == 0).all()))
        if norm == "bn":
            s, t = case.gy[:, :, d].double().sum().item(), case.gy[:, :, d].double().abs().sum().item()
            rep.within("dead channel: dbeta - the exact sum of gy", abs(bwd["dbeta"][d].item() - s), U * t + U * abs(s))
    if norm == "in" and HW == 1:
        rep.exact("one pixel per statistic: rstd == 1 / sqrt(eps)", bool((fwd["rstd"] == float(RSTD0)).all()))
        rep.exact("one pixel per statistic: dz == 0", bool((bwd["dz"] == 0).all()))


def _run_and_check(lib, case, norm, act, mat, label, ws=None, both_ways=True):
    N, HW, Cc = case.shape
    ws = _workspace(lib, N, HW, Cc) if ws is None else ws
    fwd, dev = _forward(lib, case, norm, act, mat, ws)
    bwd = _backward(lib, case, norm, act, dev, ws, alias=True)
    rep = Report(label)
    if both_ways:
        apart = _backward(lib, case, norm, act, dev, ws, alias=False)
        for k in bwd:
            rep.exact(f"{k} with dz aliasing gy == {k} with separate buffers", torch.equal(bwd[k], apart[k]))
    if case.st == "bf16" and mat:            # the statistics describe the activation AS STORED (see the module docstring)
        ref64 = _reference(case, norm, act, mat, a=fwd["act_out"])
        ref32 = _reference(case, norm, act, mat, a=fwd["act_out"], dtype=torch.float32)
    else:
        ref64, ref32 = _reference_cached(case.st, case.shape, norm, act, mat)
    _check(rep, case, norm, act, mat, fwd, bwd, ref64, ref32)
    rep.finish()


def _norms_of(st, shape):
    return [n for n in ONLY_NORMS.get((st, shape), NR.NORMS) if n != "gn" or shape[2] % 8 == 0]


def _default_cases():
    out = []
    for st in ("f32", "bf16"):
        for shape in SHAPES[st]:
            acts = [("none", False), ("relu", False), ("none", True), ("relu", True)]
            if shape[2] in EXPENSIVE_AT[st]:
                acts += [(a, m) for a in ("leakyrelu", "elu", "mish") for m in (False, True)]
            for norm, (act, mat) in itertools.product(_norms_of(st, shape), acts):
                out.append(pytest.param(st, shape, norm, act, mat,
                                        id=f"{st}-{'x'.join(map(str, shape))}-{norm}-{act}-{'stored' if mat else 'recomputed'}"))
    return out


@pytest.mark.parametrize("st,shape,norm,act,mat", _default_cases())
def test_norm_against_fp64(lib, st, shape, norm, act, mat):
    """the default route (one finishing launch per pass): forward tables, saved and running statistics, act_out, dz, dgamma,
    dbeta, dbias against the fp64 reference; `stored`: with act_out / act_in, `recomputed`: with both null"""
    _run_and_check(lib, _case(st, shape), norm, act, mat, f"norm {st} {shape} {norm} {act} {'stored' if mat else 'recomputed'}")


def _route_cases():
    out = []
    for st in ("f32", "bf16"):
        for shape in SHAPES[st]:
            if shape[2] in ROUTE_AT[st]:
                out += [pytest.param(st, shape, norm, id=f"{st}-{'x'.join(map(str, shape))}-{norm}") for norm in _norms_of(st, shape)]
    return out


@pytest.mark.parametrize("st,shape,norm", _route_cases())
def test_norm_alternative_routes_against_fp64(lib, st, shape, norm):
    """the separate reduction + finalize launches (set_finish(0)), the reduction launch whose last workgroup finalizes
    (set_finish(1); above 256 channels it falls back), the four-channels-per-workgroup launch set explicitly (set_finish(2)) and
    the in-kernel tails (set_tails(1)): each against the fp64 reference, not only against the other routes — an error they
    share would otherwise pass.  ReLU, activation recomputed; the tails' arrival counters are back at zero afterwards."""
    case = _case(st, shape)
    ws = _workspace(lib, *shape)
    try:
        for name, tails, finish in ROUTES:
            assert lib.mseg_norm_set_tails(tails) == 0 and lib.mseg_norm_set_finish(finish) == 0
            for _ in range(2 if tails else 1):           # the tails twice on one workspace: the counters were left at zero
                _run_and_check(lib, case, norm, "relu", False, f"norm route {name} {st} {shape} {norm}", ws=ws, both_ways=False)
            if tails:
                torch.cuda.synchronize()
                assert int(ws[:65536].view(torch.int32).abs().max().item()) == 0, "an arrival counter was left non-zero"
    finally:
        lib.mseg_norm_set_tails(0)
        lib.mseg_norm_set_finish(-1)


# =================================================================================================================================
# conditioning: mean / std of 10 and 100, a constant channel
# =================================================================================================================================
def test_statistics_at_large_mean_to_std_ratio(lib):
    """fp32 storage, no activation, (2, 1023, 64): channel 5 offset to mean / std = 10, channel 6 to 100, channel 7 constant 100.7.
    var = E[a^2] - mean^2 loses (mean / std)^2 of its relative accuracy; with fp32 sums of at most 8 values per trip and fp64 above
    the error stays below 8 * 2^-24 (var + mean^2) (+ the rounding of the stored rstd) — a longer fp32 trip or a dropped fp64
    stage does not.  scale and shift then agree with the reference within what that variance error implies: d rstd / rstd =
    d var / (2 (var + eps)).  The constant channel's variance comes out slightly negative and is clamped: everything finite,
    rstd <= 1 / sqrt(eps), and a * scale + shift within |mean| |scale| 2^-22 of beta."""
    case = _case("f32", (2, 1023, 64))
    N, HW, Cc = case.shape
    z = case.z.clone()
    z[:, :, 5] += 10 * 1.5
    z[:, :, 6] = z[:, :, 6] - z[:, :, 6].mean() + 100 * 1.5
    z[:, :, 7] = 100.7
    hard = case._replace(z=z)
    rep = Report("norm conditioning")
    for norm in ("bn", "in"):
        ws = _workspace(lib, N, HW, Cc)
        fwd, _ = _forward(lib, hard, norm, "none", False, ws)
        f64 = NR.forward(z, "none", norm, case.gamma, case.beta, EPS)
        ratio = (f64["mean"].abs() / torch.sqrt(f64["var"]))[..., 5:7]
        assert 8 < ratio[..., 0].min() and ratio[..., 0].max() < 13 and 80 < ratio[..., 1].min() and ratio[..., 1].max() < 130, ratio
        var_hip = 1.0 / fwd["rstd"] ** 2 - EPS
        dvar = 8 * U * (f64["var"] + f64["mean"] ** 2) + (2 * U + 4 * U * U) * (f64["var"] + EPS)
        err = (var_hip - f64["var"]).abs() / dvar
        rep.within(f"{norm}: variance a-priori, ratio 10 (error / bound)", err[..., 5].max().item(), 1.0)
        rep.within(f"{norm}: variance a-priori, ratio 100 (error / bound)", err[..., 6].max().item(), 1.0)
        rep.within(f"{norm}: variance a-priori, all channels (error / bound)", err.max().item(), 1.0)
        rel_var = (f64["var"] + f64["mean"] ** 2) / (f64["var"] + EPS)
        rep.lines.append(f"  {norm}: measured relative variance error at ratio 10: "
                         f"{((var_hip - f64['var']).abs() / f64['var'])[..., 5].max().item():.2e}, at 100: "
                         f"{((var_hip - f64['var']).abs() / f64['var'])[..., 6].max().item():.2e}")
        # implied: |d scale| <= |scale| (d var / (2 (var + eps)) + 2^-24); shift = beta - mean scale adds 8 * 2^-24 of mean's terms
        drel = 0.5 * dvar / (f64["var"] + EPS) * (1 + 1e-3) + U
        sc_err = (fwd["scale"] - f64["scale"]).abs() / (f64["scale"].abs() * drel)
        live = f64["scale"] != 0
        rep.within(f"{norm}: scale within the variance error (error / bound)", sc_err[live].max().item(), 1.0)
        dmean = 8 * U * f64["abs_mean"] + U * f64["mean"].abs()
        sh_bound = f64["mean"].abs() * f64["scale"].abs() * drel + dmean * f64["scale"].abs() + U * f64["shift_terms"]
        rep.within(f"{norm}: shift within the variance error (error / bound)", _entry_err(fwd["shift"], f64["shift"], sh_bound), 1.0)
        rep.exact(f"{norm}: gamma == 0", bool((fwd["scale"][~live] == 0).all()))
        assert rel_var[..., 6].min() > 5000
        # the constant channel
        rep.exact(f"{norm}: constant channel, rstd <= 1 / sqrt(eps)", bool((fwd["rstd"][..., 7] <= float(RSTD0)).all()))
        a = float(np.float32(100.7))
        sc, sh, mu = fwd["scale"][..., 7], fwd["shift"][..., 7], fwd["mean"][..., 7]
        be = case.beta[7].double() if norm == "bn" else torch.zeros(())
        rep.within(f"{norm}: constant channel, a * scale + shift - beta (error / bound)",
                   ((a * sc + sh - be).abs() / (mu.abs() * sc.abs() * 2.0 ** -22)).max().item(), 1.0)
    rep.finish()


# =================================================================================================================================
# mseg_norm_stats_from_conv on hand-made partial sums
# =================================================================================================================================
@pytest.mark.parametrize("Cc", [8, 40, 72])
@pytest.mark.parametrize("rows", [1, 15, 17, 100])
def test_stats_from_conv_partials(lib, rows, Cc):
    """part[rows][2][C] fp32 (row sums of 37 values ~ 1.5 N(0, 1) + 0.3 and of their squares), count = 37 rows: fewer rows than
    the 16 row slices, a ragged last slice, C no multiple of the 32 channels of a workgroup.  The kernel sums exact fp32 inputs
    in fp64: tables, saved and running statistics under the fp32 rule against the fp64 reference of the same sums."""
    k = 37
    rng = np.random.Generator(np.random.PCG64(3 + rows * 1000 + Cc))
    a = rng.standard_normal((rows, k, Cc)) * 1.5 + 0.3
    part = torch.from_numpy(np.stack([a.sum(axis=1), (a * a).sum(axis=1)], axis=1).astype(np.float32))
    g = torch.Generator().manual_seed(rows + Cc)
    gamma, beta = torch.randn(Cc, generator=g) * 0.3 + 1, torch.randn(Cc, generator=g) * 0.1
    gamma[0], gamma[Cc - 1] = -0.7, 0.0
    rm0, rv0 = torch.randn(Cc, generator=g) * 0.1, torch.rand(Cc, generator=g) + 0.5
    f64 = NR.forward_from_partials(part, rows * k, gamma, beta, EPS, MOMENTUM, rm0, rv0)
    f32 = NR.forward_from_partials(part, rows * k, gamma, beta, EPS, MOMENTUM, rm0, rv0, dtype=torch.float32)
    ws = _workspace(lib, 1, 1, Cc)
    bufs = {key: _nan_buf(Cc) for key in ("scale", "shift", "mean", "rstd", "running_mean", "running_var")}
    bufs["running_mean"][:Cc], bufs["running_var"][:Cc] = rm0.cuda(), rv0.cuda()
    pd, gd, bd = part.cuda(), gamma.cuda(), beta.cuda()
    code = lib.mseg_norm_stats_from_conv(pd.data_ptr(), rows, Cc, rows * k, gd.data_ptr(), bd.data_ptr(), EPS, bufs["scale"].data_ptr(),
                                         bufs["shift"].data_ptr(), bufs["mean"].data_ptr(), bufs["rstd"].data_ptr(),
                                         bufs["running_mean"].data_ptr(), bufs["running_var"].data_ptr(), MOMENTUM, ws.data_ptr(),
                                         _stream())
    assert code == 0
    torch.cuda.synchronize()
    got = {key: _take(v, Cc, key) for key, v in bufs.items()}
    rep = Report(f"stats from conv rows {rows} C {Cc}")
    for key, den in (("scale", f64["scale"].abs()), ("rstd", f64["rstd"]), ("running_mean", f64["running_mean_terms"]),
                     ("running_var", f64["running_var"])):
        rep.rule(key, _entry_err(f32[key], f64[key], den), _entry_err(got[key], f64[key], den), TABLE_FLOOR)
    rep.rule("shift", _entry_err(f32["shift"], f64["shift"], f64["shift_terms"]), _entry_err(got["shift"], f64["shift"], f64["shift_terms"]),
             TABLE_FLOOR)
    rep.rule("mean", _sum_err(f32["mean"], f64["mean"], f64["abs_mean"]), _sum_err(got["mean"], f64["mean"], f64["abs_mean"]), SUM_FLOOR)
    rep.exact("gamma == 0: scale == 0", got["scale"][Cc - 1].item() == 0.0)
    rep.exact("gamma == 0: shift == beta", got["shift"][Cc - 1].item() == beta[Cc - 1].double().item())
    rep.finish()


# =================================================================================================================================
# argument checks
# =================================================================================================================================
def test_norm_argument_checks(lib):
    """each invalid call returns MSEG_EINVAL and launches nothing (every output buffer keeps its NaNs); after each, a valid call
    on the same workspace gives the reference result"""
    from microbeseg_amd._lib import ACT, NORM
    shape = (3, 7, 8)
    N, HW, Cc = shape
    case = _case("f32", shape)
    ws = _workspace(lib, N, HW, 16)
    zd, gyd = case.z.cuda(), case.gy.cuda()
    z16 = torch.zeros(N * HW * 16, dtype=torch.bfloat16, device="cuda")
    gd, bd = case.gamma.cuda(), case.beta.cuda()
    outs = {k: _nan_buf(N * 16) for k in ("scale", "shift", "mean", "rstd", "rm", "rv", "dz", "dgamma", "dbeta", "dbias")}
    o = {k: v.data_ptr() for k, v in outs.items()}
    big = _nan_buf(N * HW * 16)
    ok = dict(z=zd.data_ptr(), N=N, HW=HW, C=Cc, st=0, act=ACT["relu"], norm=NORM["bn"], gamma=gd.data_ptr(), beta=bd.data_ptr(),
              scale=o["scale"], shift=o["shift"], mean=o["mean"], rstd=o["rstd"], rm=None, rv=None, ws=ws.data_ptr())

    def stats(**kw):
        a = dict(ok, **kw)
        return lib.mseg_norm_stats(a["z"], a["N"], a["HW"], a["C"], a["st"], a["act"], a["norm"], a["gamma"], a["beta"], EPS, a["scale"],
                                   a["shift"], a["mean"], a["rstd"], a["rm"], a["rv"], MOMENTUM, None, a["ws"], _stream())

    okb = dict(gy=gyd.data_ptr(), z=zd.data_ptr(), N=N, HW=HW, C=Cc, st=0, act=ACT["relu"], norm=NORM["bn"], gamma=gd.data_ptr(),
               mean=o["mean"], rstd=o["rstd"], dz=big.data_ptr(), ws=ws.data_ptr())

    def bwd(**kw):
        a = dict(okb, **kw)
        return lib.mseg_norm_bwd(a["gy"], a["z"], a["N"], a["HW"], a["C"], a["st"], a["act"], a["norm"], a["gamma"], a["mean"], a["rstd"],
                                 a["dz"], o["dgamma"], o["dbeta"], o["dbias"], None, a["ws"], _stream())

    def untouched():
        torch.cuda.synchronize()
        assert all(torch.isnan(v).all() for v in outs.values()) and torch.isnan(big).all(), "a rejected call wrote an output"

    def valid_call_still_right():
        _run_and_check(lib, case, "bn", "relu", False, "norm after a rejected call", ws=ws, both_ways=False)

    bad_stats = [dict(C=6), dict(C=10), dict(st=1, C=12, z=z16.data_ptr()), dict(norm=NORM["gn"], C=12), dict(norm=3), dict(norm=-1),
                 dict(st=2), dict(st=-1), dict(rm=o["rm"]), dict(rv=o["rv"]), dict(z=None), dict(scale=None), dict(shift=None),
                 dict(mean=None), dict(rstd=None), dict(ws=None), dict(N=0), dict(N=-1), dict(HW=0), dict(HW=-7), dict(C=0), dict(C=-8)]
    for kw in bad_stats:
        assert stats(**kw) == EINVAL, f"mseg_norm_stats accepted {kw}"
        untouched()
        valid_call_still_right()
    bad_bwd = [dict(C=6), dict(st=1, C=12, z=z16.data_ptr(), gy=z16.data_ptr()), dict(norm=NORM["gn"], C=12), dict(norm=3), dict(norm=-1),
               dict(st=2), dict(gy=None), dict(z=None), dict(mean=None), dict(rstd=None), dict(dz=None), dict(ws=None), dict(N=0),
               dict(HW=0), dict(C=0), dict(N=-2), dict(HW=-1), dict(C=-4)]
    for kw in bad_bwd:
        assert bwd(**kw) == EINVAL, f"mseg_norm_bwd accepted {kw}"
        untouched()
    valid_call_still_right()
    # from_conv: null pointers, non-positive sizes, one running statistic without the other
    part = torch.ones(4 * 2 * 8, device="cuda")
    okc = dict(part=part.data_ptr(), rows=4, C=8, count=40, scale=o["scale"], mean=o["mean"], rm=None, rv=None, ws=ws.data_ptr())
    for kw in (dict(part=None), dict(rows=0), dict(C=0), dict(count=0), dict(count=-3), dict(scale=None), dict(mean=None), dict(ws=None),
               dict(rm=o["rm"]), dict(rv=o["rv"])):
        a = dict(okc, **kw)
        assert lib.mseg_norm_stats_from_conv(a["part"], a["rows"], a["C"], a["count"], None, None, EPS, a["scale"], o["shift"], a["mean"],
                                             o["rstd"], a["rm"], a["rv"], MOMENTUM, a["ws"], _stream()) == EINVAL, kw
        untouched()
    valid_call_still_right()
