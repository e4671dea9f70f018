"""GPU (MI355X): the optimizer kernels of microbeseg_amd/csrc/loss.hip (mseg_adam_amsgrad_step, mseg_adam_amsgrad_step_dev,
mseg_ranger_step, mseg_ranger_step_multi) and mseg_bn_eval_coeffs through the C ABI, element by element against the fp64
references of tests/optim_ref.py.

Per-element assertion: |got - ref| <= bound for every element of every written array (Adam: p, m, v, vmax; Ranger: p, m, v,
slow), with the bounds of optim_ref exactly as derived there (no factor); tests/test_optim_ref_host.py shows on the same
inputs that independent fp32 evaluations stay inside them.  The gradient must come back bit-unchanged.  Every array sits
between sentinel words (a NaN pattern no kernel produces) that must come back untouched, and a refused call (MSEG_EINVAL)
must write nothing at all.

Inputs: magnitudes spread over 1e-6 .. 1e2 (g, m) and 1e-12 .. 1e6 (v) with the planted tuples of optim_ref on top, from
the first element to the last (vector body and scalar tail).

Adam sizes: 1, 3, 4, 5 (no vector / one vector / one vector and a tail), 1023 and 1027 (several workgroups, tails of 3) and
4 194 304 + 1027 — the launch is capped at 4096 workgroups x 256 threads x 4 elements, so this is the smallest size whose
grid stride runs, and it has a tail.  Its five arrays of 17 MB are the largest allocation of this file.

Ranger exact mode: beta1 = 0.5, beta2 = 0.75, step_lr = 2^-3, alpha = 0.5, not rectified, small-integer operands, rows whose
length is a power of two and whose sum is a multiple of it: every intermediate is exact in fp32 and the result must equal
the reference BIT FOR BIT — a wrong mean, row or tail shows exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as O
from conv_table import SENT, EINVAL, _sync, _stream, _eng

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 8e-4, 0.9, 0.999, 1e-8
RB1, RB2, REPS, RALPHA = 0.95, 0.999, 1e-5, 0.5
GUARD = 64                                          # words: keeps a 16-byte aligned body aligned
BIG = 4096 * 256 * 4 + 1027
ADAM_N = [1, 3, 4, 5, 1023, 1027, BIG]
ADAM_STEPS = [1, 2, 1000, 10 ** 6]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _eng()[2]


class Buf:
    """an fp32 array on the device between sentinels, `off` floats past a 16-byte boundary"""

    def __init__(self, init, off=0):
        init = np.ascontiguousarray(init, dtype=np.float32)
        self.n, self.lo = init.size, GUARD + off
        host = np.full(self.lo + self.n + GUARD, SENT, dtype=np.int32)
        host[self.lo:self.lo + self.n] = init.view(np.int32)
        self.before = host
        self.dev = torch.from_numpy(host).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + 4 * self.lo

    def take(self):
        _sync()
        after = self.dev.cpu().numpy()
        diff = after != self.before
        diff[self.lo:self.lo + self.n] = False
        bad = np.nonzero(diff)[0]
        assert bad.size == 0, f"{bad.size} sentinel words overwritten, first at element {int(bad[0]) - self.lo} of the array"
        return after[self.lo:self.lo + self.n].view(np.float32).copy()

    def untouched(self):
        _sync()
        return np.array_equal(self.dev.cpu().numpy(), self.before)


def _check(name, got, ref_bound, what):
    ref, bound = ref_bound
    err = np.abs(got.astype(np.float64) - ref)
    bad = np.nonzero(~(err <= bound))[0]                     # a NaN is wrong too
    share = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0))) if bad.size == 0 else np.inf
    assert bad.size == 0, (f"{what}: {name} misses its bound at {bad.size} of {got.size} elements, first at {int(bad[0])}: got "
                           f"{got[bad[0]]!r}, reference {ref[bad[0]]!r}, bound {bound[bad[0]]:.3e}, error {err[bad[0]]:.3e}")
    return share


def _check_all(got, ref, what):
    shares = {k: _check(k, got[k], ref[k], what) for k in ref}
    print(f"OPTIM {what} shares of the bounds:", {k: round(s, 3) for k, s in shares.items()})


# =================================================================================================================================
# Adam
# =================================================================================================================================
def _adam_bufs(arrs, offs=(0, 0, 0, 0, 0)):
    return [Buf(a, o) for a, o in zip(arrs, offs)]


def _adam_host(lib, arrs, step, offs=(0, 0, 0, 0, 0), what=""):
    bp, bg, bm, bv, bx = b = _adam_bufs(arrs, offs)
    rc = lib.mseg_adam_amsgrad_step(bp.ptr, bg.ptr, bm.ptr, bv.ptr, bx.ptr, arrs[0].size, LR, B1, B2, EPS, step, _stream())
    assert rc == 0, f"mseg_adam_amsgrad_step returned {rc} (hipError {lib.mseg_last_hip_error()})"
    got = dict(p=bp.take(), m=bm.take(), v=bv.take(), vmax=bx.take())
    assert bg.untouched(), "the gradient was written"
    _check_all(got, O.adam_step(*arrs, O.adam_scalars(LR, B1, B2, EPS, step)), what)
    return b


@pytest.mark.parametrize("step", ADAM_STEPS)
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_host_entry(lib, n, step):
    """mseg_adam_amsgrad_step, 16-byte aligned arrays: the vector body, its grid stride and the scalar tail"""
    _adam_host(lib, O.adam_inputs(n, 1000 + n % 9973 + step % 7), step, what=f"adam n={n} step={step}")
    if step == 1:                                            # a first step: all-zero state
        _adam_host(lib, O.adam_inputs(n, 2000 + n % 9973, zero_state=True), 1, what=f"adam n={n} first step")


@pytest.mark.parametrize("n", ADAM_N)
def test_adam_unaligned_takes_the_scalar_path(lib, n):
    """all five pointers one float past a 16-byte boundary: every element goes through the scalar loop"""
    _adam_host(lib, O.adam_inputs(n, 3000 + n % 9973), 1000, offs=(1, 1, 1, 1, 1), what=f"adam n={n} all pointers + 4 bytes")


@pytest.mark.parametrize("n", [5, 1027])
def test_adam_only_vmax_unaligned(lib, n):
    _adam_host(lib, O.adam_inputs(n, 4000 + n), 2, offs=(0, 0, 0, 0, 1), what=f"adam n={n} vmax + 4 bytes")


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("step", ADAM_STEPS)
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_device_entry(lib, n, step):
    """mseg_adam_amsgrad_step_dev, three calls from `step`: state[1] advances by exactly 1 per call, the two floats the call
    derives (it leaves them in the scratch slots state[2..3], lr / (1 - beta1^step) first) are within one fp32 ulp of the
    host's double evaluation (the device pow may differ in the last bit of a double), the update meets the bounds of the
    reference fed with the floats read back, and a learning rate written to state[0] between calls reaches the next step"""
    arrs = list(O.adam_inputs(n, 5000 + n % 9973 + step % 7, zero_state=step == 1))
    bp, bg, bm, bv, bx = _adam_bufs(arrs)
    state = torch.tensor([LR, float(step - 1), float("nan"), float("nan")], dtype=torch.float64, device="cuda")
    lr = LR
    for call in range(3):
        s = step + call
        if call == 2:
            lr = 0.25 * LR
            state[0] = lr
        rc = lib.mseg_adam_amsgrad_step_dev(bp.ptr, bg.ptr, bm.ptr, bv.ptr, bx.ptr, n, state.data_ptr(), B1, B2, EPS, _stream())
        assert rc == 0, f"mseg_adam_amsgrad_step_dev returned {rc} (hipError {lib.mseg_last_hip_error()})"
        _sync()
        st = state.cpu().numpy()
        assert st[0] == lr and st[1] == float(s), st
        d = st[2:4].view(np.float32)
        want = O.adam_scalars(lr, B1, B2, EPS, s)
        assert abs(float(d[0]) - want["step_size"]) <= _ulp32(want["step_size"]), (d[0], want["step_size"])
        assert abs(float(d[1]) - want["bc2_sqrt"]) <= _ulp32(want["bc2_sqrt"]), (d[1], want["bc2_sqrt"])
        sc = dict(want, step_size=float(d[0]), bc2_sqrt=float(d[1]))
        got = dict(p=bp.take(), m=bm.take(), v=bv.take(), vmax=bx.take())
        assert bg.untouched(), "the gradient was written"
        _check_all(got, O.adam_step(*arrs, sc), f"adam_dev n={n} step={s}")
        # the next call starts from what this one left (the buffers stay; their reference copy follows)
        arrs = [got["p"], arrs[1], got["m"], got["v"], got["vmax"]]
        for b, a in zip((bp, bm, bv, bx), (got["p"], got["m"], got["v"], got["vmax"])):
            b.before[b.lo:b.lo + b.n] = a.view(np.int32)


def test_adam_refusals_write_nothing(lib):
    arrs = O.adam_inputs(37, 6000)
    b = _adam_bufs(arrs)
    ptrs = [x.ptr for x in b]
    state = torch.tensor([LR, 3.0, -1.0, -2.0, 7.0], dtype=torch.float64, device="cuda")
    st0 = state.cpu().numpy().copy()
    host = lambda ps, n, step: lib.mseg_adam_amsgrad_step(*ps, n, LR, B1, B2, EPS, step, _stream())
    dev = lambda ps, n, sp: lib.mseg_adam_amsgrad_step_dev(*ps, n, sp, B1, B2, EPS, _stream())
    assert host(ptrs, 0, 5) == EINVAL and dev(ptrs, 0, state.data_ptr()) == EINVAL                 # n == 0
    assert host(ptrs, 37, 0) == EINVAL and host(ptrs, 37, -1) == EINVAL                            # step < 1
    for i in range(5):                                                                             # a NULL pointer
        ps = list(ptrs)
        ps[i] = None
        assert host(ps, 37, 5) == EINVAL and dev(ps, 37, state.data_ptr()) == EINVAL, i
    assert dev(ptrs, 37, None) == EINVAL
    assert dev(ptrs, 37, state.data_ptr() + 4) == EINVAL                                           # state not 8-byte aligned
    assert all(x.untouched() for x in b)
    _sync()
    assert np.array_equal(state.cpu().numpy(), st0)
    assert host(ptrs, 37, 5) == 0 and not b[0].untouched()                                         # the same call, accepted


# =================================================================================================================================
# Ranger, one tensor
# =================================================================================================================================
def _ranger_call(lib, arrs, rows, sc, rect, gc, look):
    """-> (rc, buffers); rows is passed as it is (without centralisation the entry only wants it positive)"""
    b = [Buf(a) for a in arrs]
    rc = lib.mseg_ranger_step(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr, arrs[0].size, rows, sc["beta1_in"],
                              sc["beta2_in"], sc["eps_in"], sc["step_lr_in"], rect, gc, look, sc["alpha"], _stream())
    return rc, b


def _ranger_scalars(beta1, beta2, eps, step_lr, alpha):
    sc = O.ranger_scalars(beta1, beta2, eps, step_lr, alpha)
    return dict(sc, beta1_in=beta1, beta2_in=beta2, eps_in=eps, step_lr_in=step_lr)          # the doubles the entry is given


def _ranger_take(b):
    got = dict(p=b[0].take(), m=b[2].take(), v=b[3].take(), slow=b[4].take())
    assert b[1].untouched(), "the gradient was written"
    return got


def _ranger_float(lib, arrs, rows, gc, rect, look, step_lr, what):
    sc = _ranger_scalars(RB1, RB2, REPS, step_lr, RALPHA)
    rc, b = _ranger_call(lib, arrs, rows if gc else 1, sc, rect, gc, look)
    assert rc == 0, f"mseg_ranger_step returned {rc} (hipError {lib.mseg_last_hip_error()})"
    got = _ranger_take(b)
    _check_all(got, O.ranger_step(*arrs, rows if gc else 0, sc, rect, look), what)
    return got


@pytest.mark.parametrize("look", [0, 1])
@pytest.mark.parametrize("rect", [0, 1])
@pytest.mark.parametrize("gc", [0, 1])
def test_ranger_float(lib, rect, gc, look):
    """all 8 combinations of (rectified, gc, lookahead); with centralisation over the row shapes, without over the sizes
    around the 4096 elements of a workgroup (planted tuples included)"""
    if gc:
        for rows, cols in O.GC_SHAPES:
            arrs = O.ranger_inputs(rows * cols, 200 + rows * cols + rows, plants=False)
            _ranger_float(lib, arrs, rows, 1, rect, look, 3.3e-4, f"ranger gc {rows}x{cols} rect={rect} look={look}")
    else:
        for n in O.NOGC_SIZES:
            arrs = O.ranger_inputs(n, 200 + n)
            _ranger_float(lib, arrs, 0, 0, rect, look, 3.3e-4, f"ranger n={n} rect={rect} look={look}")


@pytest.mark.parametrize("rect,look", [(1, 0), (0, 1)])
def test_ranger_float_gradient_offset(lib, rect, look):
    """every gradient + 1000: the centralised gradient is a cancellation against the row mean"""
    arrs = O.ranger_inputs(16 * 72, 777, plants=False, offset=1000.0)
    _ranger_float(lib, arrs, 16, 1, rect, look, 3.3e-4, f"ranger gc 16x72 +1000 rect={rect} look={look}")


EXACT_GC = [(1, 64), (5, 16), (16, 64), (3, 1), (2, 8192), (256, 256)]


@pytest.mark.parametrize("look", [0, 1])
@pytest.mark.parametrize("gc", [0, 1])
def test_ranger_exact(lib, gc, look):
    sc = _ranger_scalars(0.5, 0.75, 1e-5, 0.125, 0.5)
    cases = [(r * c, r) for r, c in EXACT_GC] if gc else [(n, 0) for n in O.NOGC_SIZES]
    for n, rows in cases:
        arrs = O.ranger_exact_inputs(n, rows, 300 + n + rows)
        rc, b = _ranger_call(lib, arrs, rows if gc else 1, sc, 0, gc, look)
        assert rc == 0
        got = _ranger_take(b)
        ref = O.ranger_step(*arrs, rows, sc, 0, look)
        for k in ref:
            assert np.array_equal(ref[k][0].astype(np.float32).astype(np.float64), ref[k][0]), "the exact mode is not exact"
            wrong = np.nonzero(~(got[k].astype(np.float64) == ref[k][0]))[0]
            assert wrong.size == 0, (f"ranger exact n={n} rows={rows} look={look}: {k} differs at {wrong.size} elements, first at "
                                     f"{int(wrong[0])}: got {got[k][wrong[0]]!r}, expected {ref[k][0][wrong[0]]!r}")


def test_ranger_refusals_write_nothing(lib):
    arrs = O.ranger_inputs(60, 8)
    sc = _ranger_scalars(RB1, RB2, REPS, 3.3e-4, RALPHA)
    rc, b = _ranger_call(lib, arrs, 7, sc, 1, 1, 1)                     # 60 % 7 != 0 with centralisation
    assert rc == EINVAL and all(x.untouched() for x in b)
    rc, b = _ranger_call(lib, arrs, 0, sc, 1, 0, 1)                     # rows <= 0
    assert rc == EINVAL and all(x.untouched() for x in b)
    ptrs = [x.ptr for x in b]
    for i in range(5):
        ps = list(ptrs)
        ps[i] = None
        assert lib.mseg_ranger_step(*ps, 60, 5, RB1, RB2, REPS, 3.3e-4, 1, 1, 1, RALPHA, _stream()) == EINVAL
    assert lib.mseg_ranger_step(*ptrs, 0, 5, RB1, RB2, REPS, 3.3e-4, 1, 1, 1, RALPHA, _stream()) == EINVAL      # n == 0
    assert all(x.untouched() for x in b)
    rc, b = _ranger_call(lib, arrs, 5, sc, 1, 1, 1)                     # 60 % 5 == 0: accepted
    assert rc == 0 and not b[0].untouched()


# =================================================================================================================================
# Ranger, many tensors
# =================================================================================================================================
# (rows, n): rows > 0 centralised.  One-block jobs beside many-block ones (256 rows; 9000 elements = 3 blocks without gc)
PALETTE = [(256, 256 * 300), (0, 1), (5, 60), (0, 9000), (3, 3), (0, 4097)]


def _multi_jobs(njobs):
    jobs = []
    for i in range(njobs):
        rows, n = PALETTE[i % len(PALETTE)]
        arrs = O.ranger_inputs(n, 900 + 7 * i, plants=rows == 0)
        jobs.append(dict(rows=rows, n=n, arrs=arrs, flags=(i // 2) % 4, step_lr=O.f32(3.3e-4 * (1 + i % 5))))
    return jobs


def _multi_launch(lib, jobs):
    from microbeseg_amd._lib import MsegRangerJob
    rec = (MsegRangerJob * len(jobs))()
    bufs = []
    for r, j in zip(rec, jobs):
        b = [Buf(a) for a in j["arrs"]]
        bufs.append(b)
        r.p, r.g, r.m, r.v, r.slow = (x.ptr for x in b)
        r.n, r.rows, r.step_lr, r.flags = j["n"], j["rows"], j["step_lr"], j["flags"]
    rc = lib.mseg_ranger_step_multi(C.addressof(rec), len(jobs), RB1, RB2, REPS, RALPHA, _stream())
    return rc, bufs


@pytest.mark.parametrize("njobs", [1, 48, 49, 96, 97])
def test_ranger_multi(lib, njobs):
    """48 job records travel per launch: one launch, a full one, a full one and one job, two full ones, two and one.  Every
    tensor must equal the per-tensor entry bit for bit and meet the fp64 bounds; per-job step_lr and flags."""
    jobs = _multi_jobs(njobs)
    assert {j["flags"] for j in jobs} == ({0, 1, 2, 3} if njobs > 1 else {0})
    rc, bufs = _multi_launch(lib, jobs)
    assert rc == 0, f"mseg_ranger_step_multi returned {rc} (hipError {lib.mseg_last_hip_error()})"
    for i, (j, b) in enumerate(zip(jobs, bufs)):
        got = _ranger_take(b)
        rect, look = j["flags"] & 1, (j["flags"] >> 1) & 1
        sc = _ranger_scalars(RB1, RB2, REPS, j["step_lr"], RALPHA)
        ref = O.ranger_step(*j["arrs"], j["rows"], sc, rect, look)
        for k in ref:
            _check(k, got[k], ref[k], f"ranger_multi job {i} of {njobs} (rows {j['rows']}, n {j['n']}, flags {j['flags']})")
        rc, b1 = _ranger_call(lib, j["arrs"], j["rows"] if j["rows"] else 1, sc, rect, int(j["rows"] > 0), look)
        assert rc == 0
        one = _ranger_take(b1)
        for k in one:
            assert np.array_equal(one[k].view(np.int32), got[k].view(np.int32)), f"job {i} of {njobs}: {k} differs from mseg_ranger_step"


def test_ranger_multi_refusals_write_nothing(lib):
    jobs = _multi_jobs(49)
    jobs[48] = dict(jobs[48], rows=7, n=60, arrs=O.ranger_inputs(60, 5))       # 60 % 7 != 0, in the second launch's share
    rc, bufs = _multi_launch(lib, jobs)
    assert rc == EINVAL and all(x.untouched() for b in bufs for x in b)
    from microbeseg_amd._lib import MsegRangerJob
    rec = (MsegRangerJob * 1)()
    b = [Buf(a) for a in jobs[1]["arrs"]]
    rec[0].p, rec[0].g, rec[0].m, rec[0].v, rec[0].slow = (x.ptr for x in b)
    rec[0].n, rec[0].rows, rec[0].step_lr, rec[0].flags = 1, 0, 1e-3, 3
    for nj in (0, -1):
        assert lib.mseg_ranger_step_multi(C.addressof(rec), nj, RB1, RB2, REPS, RALPHA, _stream()) == EINVAL
    assert lib.mseg_ranger_step_multi(None, 1, RB1, RB2, REPS, RALPHA, _stream()) == EINVAL
    assert all(x.untouched() for x in b)


# =================================================================================================================================
# eval-mode BatchNorm coefficients
# =================================================================================================================================
@pytest.mark.parametrize("C_", [1, 255, 256, 257])
def test_bn_eval_coeffs(lib, C_):
    """one workgroup, its last thread idle, exactly full, a second workgroup; gamma / beta present and NULL; running_var 0,
    2^-30, 1 and 1e6 planted among random values; per-channel bound"""
    for seed, (use_g, use_b) in enumerate(((1, 1), (0, 1), (1, 0), (0, 0))):
        gamma, beta, rm, rv = O.bn_inputs(C_, seed)
        ins = [Buf(a) for a in (gamma, beta, rm, rv)]
        nan = np.full(C_, np.nan, dtype=np.float32)
        sc, sh = Buf(nan), Buf(nan)
        rc = lib.mseg_bn_eval_coeffs(ins[0].ptr if use_g else None, ins[1].ptr if use_b else None, ins[2].ptr, ins[3].ptr,
                                     1e-5, C_, sc.ptr, sh.ptr, _stream())
        assert rc == 0
        ref = O.bn_eval_coeffs(gamma if use_g else None, beta if use_b else None, rm, rv, 1e-5)
        _check_all(dict(scale=sc.take(), shift=sh.take()), ref, f"bn_eval_coeffs C={C_} gamma={use_g} beta={use_b}")
        assert all(x.untouched() for x in ins)
    for args in ((None, ins[3].ptr, C_, sc.ptr, sh.ptr), (ins[2].ptr, None, C_, sc.ptr, sh.ptr), (ins[2].ptr, ins[3].ptr, 0, sc.ptr, sh.ptr),
                 (ins[2].ptr, ins[3].ptr, C_, None, sh.ptr), (ins[2].ptr, ins[3].ptr, C_, sc.ptr, None)):
        sc2, sh2 = Buf(nan), Buf(nan)
        a = list(args)
        a[3] = sc2.ptr if a[3] is not None else None
        a[4] = sh2.ptr if a[4] is not None else None
        assert lib.mseg_bn_eval_coeffs(ins[0].ptr, ins[1].ptr, a[0], a[1], 1e-5, a[2], a[3], a[4], _stream()) == EINVAL
        assert sc2.untouched() and sh2.untouched()
