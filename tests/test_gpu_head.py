"""GPU (MI355X): mseg_head_fwd / mseg_head_bwd (csrc/head.hip) through the C ABI against the fp64 reference of
tests/head_ref.py (which tests/test_head_ref_host.py pins to F.conv2d and autograd on the CPU).

A covering set over channel count and storage (fp32 4 .. 1028, bf16 8 .. 136), Co 1 .. 4, the five activations, no / per-channel
/ per-sample tables, fp32 and bf16 gy, and (N, HW) pairs that give the backward one chunk, several even chunks, an uneven last
chunk, the 1024 / N chunk cap (maxc = 1 at N = 700; N = 1100 > 1024) — plus one case past the forward's 8192-block cap.
Outputs are pre-filled with NaN and carry a NaN guard band that must come back untouched.

Bound for every smooth quantity q (out, fp32 gy, dW, db), under max|got - ref| against fp64:
    e_hip <= max(4 e_ref, 4 ulp_fp32(max|ref|)),   e_ref = the same statements in torch CPU fp32 on the same inputs.
bf16 gy: within one bf16 ulp of the fp64 result rounded to bf16; those cases draw W and gout from binary grids, so that the
fp32 sum in front of the rounding is exact and the one ulp is not spent on it.

Measured on the MI355X (first run), worst e_hip as a share of its bound over all cases: out 0.30, fp32 gy 0.25, dW 0.12,
db 0.12; the large case e_ref / e_hip: out 1.9e-6 / 1.6e-6, dW 5.3e-2 / 1.5e-4, db 1.2e-4 / 5.8e-6, gy 3.4e-7 / 3.4e-7; bf16 gy
equal to the rounded fp64 result in all 25 cases.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import head_ref as R
import pointwise_ref as P

pytestmark = pytest.mark.gpu

GUARD = 64
EINVAL = -1
NAN = float("nan")
F32, BF16 = 0, 1

SHAPES = [(1, 1), (2, 63), (2, 240), (1, 1024), (1, 1100), (3, 1536), (3, 2000), (700, 1024), (1100, 4)]
SOURCES = [(F32, 4), (F32, 8), (F32, 24), (F32, 64), (F32, 128), (BF16, 8), (BF16, 64), (BF16, 136)]
TABLES = ("none", "channel", "sample")
BIG = (F32, 64, 3, "mish", "channel", F32, 2, 262400)         # 524 800 pixels: 8200 forward blocks of 64 pixels, 512 chunks


def _cases():
    """(src dtype, C, Co, act, tables, gy dtype, N, HW).  Every shape meets six of the eight sources (the 700 x 1024 shape only
    C <= 8: its tensors stay below the large case); Co, activation, tables and gy type cycle with co-prime periods.  C = 1028
    (the cbase loop) runs at HW = 64 only."""
    cases, k = [], 0
    for si, (N, HW) in enumerate(SHAPES):
        for ci, (dt, Cc) in enumerate(SOURCES):
            if (N, HW) == (700, 1024):
                if Cc > 8:
                    continue
            elif (si + ci) % 4 == 0 or (si + 2 * ci) % 7 == 0:
                continue
            tables = TABLES[k % 3] if N > 1 else TABLES[k % 2]
            cases.append((dt, Cc, 1 + (k % 4), R.ACTS[k % 5], tables, (k // 2) % 2, N, HW))
            k += 1
    for j, (Co, tables, gyd) in enumerate([(1, "sample", F32), (3, "channel", BF16), (4, "sample", F32), (2, "none", F32)]):
        cases.append((F32, 1028, Co, R.ACTS[(j + 2) % 5], tables, gyd, 3, 64))
    # per-sample tables with N = 3 for every storage and both gy types, whatever the cycles gave
    cases += [(BF16, 136, 4, "mish", "sample", BF16, 3, 2000), (F32, 24, 3, "elu", "sample", BF16, 3, 1536),
              (BF16, 8, 2, "leakyrelu", "sample", F32, 3, 1536), (F32, 4, 4, "relu", "sample", F32, 3, 2000)]
    return cases


CASES = _cases()


def test_the_case_list_covers_every_axis():
    assert 50 <= len(CASES) <= 70, len(CASES)
    col = lambda i: {c[i] for c in CASES}                                               # noqa: E731
    assert {(c[0], c[1]) for c in CASES} == set(SOURCES) | {(F32, 1028)}
    assert col(2) == {1, 2, 3, 4} and col(3) == set(R.ACTS) and col(4) == set(TABLES) and col(5) == {F32, BF16}
    assert {(c[6], c[7]) for c in CASES} == set(SHAPES) | {(3, 64)}
    for dt in (F32, BF16):                                                              # pairs that select another kernel
        assert {c[2] for c in CASES if c[0] == dt} == {1, 2, 3, 4}
        assert {c[5] for c in CASES if c[0] == dt} == {F32, BF16}
        assert {c[4] for c in CASES if c[0] == dt} == set(TABLES)
    assert all(c[6] == 3 for c in CASES if c[1] == 1028) and {c[7] for c in CASES if c[1] == 1028} == {64}
    assert sum(c[4] == "sample" and c[6] == 3 for c in CASES) >= 6
    for N, HW in ((700, 1024), (1100, 4)):                                               # the chunk cap, both storages
        assert {c[0] for c in CASES if (c[6], c[7]) == (N, HW)} == {F32, BF16}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from microbeseg_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_buf(n, dtype=torch.float32):
    return torch.full((n + GUARD,), NAN, dtype=dtype, device="cuda")


def _take(buf, n):
    torch.cuda.synchronize()
    host = buf.cpu()
    assert torch.isnan(host[n:].float()).all(), "the kernel wrote behind its output"
    assert not torch.isnan(host[:n].float()).any(), "an output element was left unwritten"
    return host[:n]


@functools.lru_cache(maxsize=2)
def _inputs(dt, Cc, Co, act, tables, gyd, N, HW):
    """z N(0, 2) (bf16 sources: rounded to bf16 first, the reference reads the same values), tables with different rows per
    sample, W, b, gout; for bf16 gy W lies on the grid k / 64 and gout on k / 16 (products and their sum exact in fp32)"""
    g = torch.Generator().manual_seed(1000003 * N + 1009 * HW + 31 * Cc + 7 * Co + 3 * dt + gyd + len(act) + len(tables))
    z = torch.randn(N, HW, Cc, generator=g) * 2
    if dt == BF16:
        z = z.to(torch.bfloat16)
    shape = {"none": None, "channel": (Cc,), "sample": (N, Cc)}[tables]
    scale = None if shape is None else torch.randn(shape, generator=g) * 0.3 + 1
    shift = None if shape is None else torch.randn(shape, generator=g) * 0.2
    if tables == "sample" and N > 1:
        assert not torch.equal(scale[0], scale[1]) and not torch.equal(shift[0], shift[N - 1])
    if gyd == BF16:
        w = torch.randint(-64, 65, (Co, Cc), generator=g).float() / 64
        gout = torch.randint(-64, 65, (N, Co, HW), generator=g).float() / 16
    else:
        w = torch.randn(Co, Cc, generator=g) * 0.2
        gout = torch.randn(N, Co, HW, generator=g)
    b = torch.randn(Co, generator=g)
    return z, scale, shift, w, b, gout


def _src(z_dev, Cc, act, scale_dev, shift_dev, tables, dt):
    from microbeseg_amd import _lib
    s = _lib.MsegSrc()
    s.ptr, s.C, s.act, s.dtype = z_dev.data_ptr(), Cc, R.ACTS.index(act), dt
    s.scale = None if scale_dev is None else scale_dev.data_ptr()
    s.shift = None if shift_dev is None else shift_dev.data_ptr()
    s.ss = Cc if tables == "sample" else 0
    return s


def _bound(ref32, ref64, got, what):
    """e_hip <= max(4 e_ref, 4 ulp of max|ref|), all under max|. - ref64|"""
    ref64 = ref64.double()
    e_ref = (ref32.double() - ref64).abs().max().item()
    e_hip = (got.double() - ref64).abs().max().item()
    ulp = float(np.spacing(np.float32(ref64.abs().max().item())))
    print(f"    {what}: e_ref {e_ref:.3e} e_hip {e_hip:.3e} (4 ulp {4 * ulp:.3e}, max|ref| {ref64.abs().max().item():.3e})")
    assert e_hip <= max(4 * e_ref, 4 * ulp), f"{what}: e_hip {e_hip:.3e}, e_ref {e_ref:.3e}, 4 ulp {4 * ulp:.3e}"


def _run(lib, dt, Cc, Co, act, tables, gyd, N, HW, with_bias=True):
    z, scale, shift, w, b, gout = _inputs(dt, Cc, Co, act, tables, gyd, N, HW)
    print(f"head src {'bf16' if dt else 'fp32'} C {Cc} Co {Co} {act} tables {tables} gy {'bf16' if gyd else 'fp32'} "
          f"N {N} HW {HW}")
    zd, wd, bd, gd = z.cuda(), w.cuda(), b.cuda(), gout.cuda()
    scd = None if scale is None else scale.cuda()
    shd = None if shift is None else shift.cuda()
    s = _src(zd, Cc, act, scd, shd, tables, dt)
    # forward
    out = _nan_buf(N * Co * HW)
    code = lib.mseg_head_fwd(C.byref(s), N, HW, wd.data_ptr(), bd.data_ptr() if with_bias else None, Co, out.data_ptr(),
                             _stream())
    assert code == 0, code
    got_out = _take(out, N * Co * HW).reshape(N, Co, HW)
    # backward
    gy = _nan_buf(N * HW * Cc, torch.bfloat16 if gyd == BF16 else torch.float32)
    dW, db = _nan_buf(Co * Cc), _nan_buf(Co)
    ws = torch.empty(lib.mseg_head_bwd_workspace_bytes(N, HW, Cc, Co), dtype=torch.uint8, device="cuda")
    code = lib.mseg_head_bwd(C.byref(s), N, HW, wd.data_ptr(), Co, gd.data_ptr(), gy.data_ptr(), gyd, dW.data_ptr(),
                             db.data_ptr(), ws.data_ptr(), _stream())
    assert code == 0, code
    got_gy = _take(gy, N * HW * Cc).reshape(N, HW, Cc)
    got_dW, got_db = _take(dW, Co * Cc).reshape(Co, Cc), _take(db, Co)
    del zd, gd, out, gy, ws
    # references
    bb = b if with_bias else None
    x64, x32 = R.operand(z, act, scale, shift), R.operand(z, act, scale, shift, dtype=torch.float32)
    _bound(R.head_fwd(x32, w, bb), R.head_fwd(x64, w, bb), got_out, "out")
    gy64, dW64, db64 = R.head_bwd(x64, w, gout)
    gy32, dW32, db32 = R.head_bwd(x32, w, gout)
    del x64, x32
    _bound(dW32, dW64, got_dW, "dW")
    _bound(db32, db64, got_db, "db")
    if gyd == BF16:
        assert torch.equal(gy32.double(), gy64), "the grids do not make the fp32 sum exact"
        want = P.bf16_round(gy64.numpy())
        got_bits = got_gy.view(torch.int16).numpy().view(np.uint16)
        ref = P.bf16_bits_to_f64(want)
        ulp = np.exp2(np.maximum(np.frexp(ref)[1] - 8, -133).astype(np.float64))
        err = np.abs(P.bf16_bits_to_f64(got_bits) - ref)
        print(f"    gy bf16: {int((got_bits != want).sum())} of {want.size} differ from the rounded fp64 result, "
              f"max {float((err / ulp).max()):.2f} ulp")
        assert (err <= ulp).all(), f"gy: {int((err > ulp).sum())} elements more than one bf16 ulp off"
    else:
        _bound(gy32, gy64, got_gy, "gy")


@pytest.mark.parametrize("dt,Cc,Co,act,tables,gyd,N,HW", CASES,
                         ids=[f"{'bf16' if c[0] else 'f32'}-C{c[1]}-Co{c[2]}-{c[3]}-{c[4]}-gy{'16' if c[5] else '32'}-{c[6]}x{c[7]}"
                              for c in CASES])
def test_head_forward_backward_fp64(lib, dt, Cc, Co, act, tables, gyd, N, HW):
    _run(lib, dt, Cc, Co, act, tables, gyd, N, HW)


def test_head_without_bias(lib):
    """b == NULL: the forward adds nothing (a bias-free head; the backward does not depend on b)"""
    _run(lib, F32, 8, 2, "relu", "channel", F32, 2, 63, with_bias=False)


def test_head_past_the_forward_block_cap(lib):
    """N HW = 524 800 pixels at C = 64: 8200 blocks of 64 pixels wanted, 8192 launched, so the forward's grid-stride loop takes
    a second trip; the backward runs 512 chunks of 513 rows per sample (the 1024 / N cap), the last one shorter"""
    dt, Cc, Co, act, tables, gyd, N, HW = BIG
    assert N * HW > 8192 * 64 and HW // 512 >= 1024 // N
    _run(lib, *BIG)
    _inputs.cache_clear()


def test_head_argument_checks(lib):
    """Co = 5, C = 6, a bf16 source with C = 12 and an unknown gy_dtype are MSEG_EINVAL; a rejected call launches nothing (the
    buffers are valid and large enough all the same, and come back untouched)"""
    N, HW = 2, 40
    z = torch.zeros(N * HW * 16, device="cuda")
    w, b = torch.ones(5 * 16, device="cuda"), torch.zeros(5, device="cuda")
    gout = torch.ones(N * 5 * HW, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for Cc, Co, dt, gyd in ((8, 5, F32, F32), (6, 2, F32, F32), (12, 2, BF16, F32), (8, 2, F32, 2), (8, 2, F32, -1)):
        s = _src(z, Cc, "relu", None, None, "none", dt)
        out, gy, dW, db = _nan_buf(N * 5 * HW), _nan_buf(N * HW * 16), _nan_buf(5 * 16), _nan_buf(5)
        if gyd in (F32, BF16):
            assert lib.mseg_head_fwd(C.byref(s), N, HW, w.data_ptr(), b.data_ptr(), Co, out.data_ptr(), _stream()) == EINVAL
        assert lib.mseg_head_bwd(C.byref(s), N, HW, w.data_ptr(), Co, gout.data_ptr(), gy.data_ptr(), gyd, dW.data_ptr(),
                                 db.data_ptr(), ws.data_ptr(), _stream()) == EINVAL
        torch.cuda.synchronize()
        for t in (out, gy, dW, db):
            assert torch.isnan(t).all()
    s = _src(z, 8, "relu", None, None, "none", F32)                # the same buffers, valid arguments: runs
    out = _nan_buf(N * 2 * HW)
    assert lib.mseg_head_fwd(C.byref(s), N, HW, w.data_ptr(), b.data_ptr(), 2, out.data_ptr(), _stream()) == 0
    assert (_take(out, N * 2 * HW) == 0).all()
