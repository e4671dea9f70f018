"""Host: the plain references of tests/conv_ref.py against torch.nn.functional in fp64 (values, and gradients through
autograd) on a few odd shapes — N > 1, H != W, stride 2 on odd and even sizes, channel counts off every tile size — so that
the GPU tests of the convolution kernels can use them as the yardstick; and the bf16 rounding, the bf16 operand with its
ambiguity field and the widening condition of the bf16 table (tests/test_gpu_conv_bf16.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
import pointwise_ref as R

TOL = 1e-12          # fp64 against fp64, sums of a few hundred terms of magnitude ~1


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.asarray(a, dtype=np.float64), 3, 1)))


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def _close(got, want, S=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    scale = np.maximum(np.abs(want), 1.0) if S is None else np.maximum(S, 1e-30)
    assert (np.abs(got - want) / scale).max() < TOL


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("per_sample", [False, True])
def test_operand(act, per_sample):
    g = _rng(1)
    z = g.normal(size=(3, 5, 7, 12)) * 3
    shape = (3, 12) if per_sample else (12,)
    sc, sh = g.normal(size=shape), g.normal(size=shape)
    zt = _nchw(z)
    a = {"none": lambda v: v, "relu": F.relu, "leakyrelu": lambda v: F.leaky_relu(v, 0.01), "elu": F.elu, "mish": F.mish}[act](zt)
    st, ht = torch.from_numpy(sc), torch.from_numpy(sh)
    want = a * (st[:, :, None, None] if per_sample else st[None, :, None, None]) + \
        (ht[:, :, None, None] if per_sample else ht[None, :, None, None])
    _close(CR.operand(z, act, sc, sh), _nhwc(want))
    _close(CR.operand(z, R.ACTS.index(act)), _nhwc(a))


CONV_SHAPES = [(2, [12], 20, 7, 10, 1), (3, [8, 20], 9, 5, 9, 1), (2, [12], 6, 9, 7, 2), (2, [4, 8], 10, 8, 12, 2),
               (1, [36], 68, 6, 5, 2)]


@pytest.mark.parametrize("N,cs,Cout,H,W,stride", CONV_SHAPES)
def test_conv_fwd_and_dgrad(N, cs, Cout, H, W, stride):
    g = _rng(N + Cout + H)
    xs = [g.normal(size=(N, H, W, c)) for c in cs]
    w, b = g.normal(size=(Cout, sum(cs), 3, 3)), g.normal(size=Cout)
    x = torch.cat([_nchw(v) for v in xs], 1).requires_grad_(True)
    y = F.conv2d(x, torch.from_numpy(w), torch.from_numpy(b), stride=stride, padding=1)
    Ho, Wo = y.shape[2:]
    base = g.normal(size=(N, Ho, Wo, Cout))
    out, S = CR.conv_fwd(xs, w, b, stride)
    _close(out, _nhwc(y), S)
    out2, S2 = CR.conv_fwd(xs, w, b, stride, base=base)
    _close(out2, _nhwc(y) + base, S2)
    Sref = F.conv2d(x.detach().abs(), torch.from_numpy(np.abs(w)), torch.from_numpy(np.abs(b)), stride=stride, padding=1)
    _close(S, _nhwc(Sref))
    _close(S2, _nhwc(Sref) + np.abs(base))
    gy = g.normal(size=(N, Ho, Wo, Cout))
    y.backward(_nchw(gy))
    dx, Sd = CR.conv_dgrad(gy, w, stride, H, W)
    _close(dx, _nhwc(x.grad), Sd)
    based = g.normal(size=dx.shape)
    dx2, Sd2 = CR.conv_dgrad(gy, w, stride, H, W, base=based)
    _close(dx2, _nhwc(x.grad) + based, Sd2)
    assert (Sd2 >= np.abs(dx2) - 1e-9).all() and (S >= np.abs(out) - 1e-9).all()


@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 12, 20, 5, 7), (3, 36, 6, 3, 4), (1, 8, 68, 6, 2)])
def test_convT_fwd_and_dgrad(N, Cin, Cout, H, W):
    g = _rng(N + Cin)
    xa = g.normal(size=(N, H, W, Cin))
    w, b = g.normal(size=(Cin, Cout, 2, 2)), g.normal(size=Cout)
    x = _nchw(xa).requires_grad_(True)
    y = F.conv_transpose2d(x, torch.from_numpy(w), torch.from_numpy(b), stride=2)
    out, S = CR.convT_fwd(xa, w, b)
    _close(out, _nhwc(y), S)
    Sref = F.conv_transpose2d(x.detach().abs(), torch.from_numpy(np.abs(w)), torch.from_numpy(np.abs(b)), stride=2)
    _close(S, _nhwc(Sref))
    gy = g.normal(size=out.shape)
    y.backward(_nchw(gy))
    base = g.normal(size=xa.shape)
    dx, Sd = CR.convT_dgrad(gy, w, base=base)
    _close(dx, _nhwc(x.grad) + base, Sd)
    _close(CR.convT_dgrad(gy, w)[0], _nhwc(x.grad))


@pytest.mark.parametrize("N,cs,Cout,H,W,stride", CONV_SHAPES)
def test_wgrad_3x3(N, cs, Cout, H, W, stride):
    g = _rng(7 + N + Cout + W)
    qs = [g.normal(size=(N, H, W, c)) for c in cs]
    w = torch.from_numpy(g.normal(size=(Cout, sum(cs), 3, 3))).requires_grad_(True)
    y = F.conv2d(torch.cat([_nchw(v) for v in qs], 1), w, None, stride=stride, padding=1)
    gy = g.normal(size=tuple(_nhwc(y).shape))
    y.backward(_nchw(gy))
    G, S = CR.wgrad(gy, qs, 3, stride)
    _close(G, w.grad.numpy(), S)
    keep = sum(cs) - 3
    G2, S2 = CR.wgrad(gy, qs, 3, stride, nch_store=keep)
    assert G2.shape == (Cout, keep, 3, 3) and S2.shape == G2.shape
    _close(G2, w.grad.numpy()[:, :keep], S2)
    assert (S >= np.abs(G) - 1e-9).all()


@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 12, 20, 5, 7), (3, 36, 6, 3, 4)])
def test_wgrad_2x2(N, Cin, Cout, H, W):
    g = _rng(11 + Cin)
    xa = g.normal(size=(N, H, W, Cin))
    w = torch.from_numpy(g.normal(size=(Cin, Cout, 2, 2))).requires_grad_(True)
    y = F.conv_transpose2d(_nchw(xa), w, None, stride=2)
    gy = g.normal(size=tuple(_nhwc(y).shape))
    y.backward(_nchw(gy))
    half = Cout // 2
    G, S = CR.wgrad(xa, [gy[..., :half], gy[..., half:]], 2, 2)
    _close(G, w.grad.numpy(), S)


def test_exact_mode_is_integer_arithmetic():
    """int64 operands stay int64, S bounds every result, and the 2^24 premise is checked"""
    g = _rng(3)
    x = g.integers(-3, 4, size=(2, 5, 6, 8))
    w, b = g.integers(-3, 4, size=(4, 8, 3, 3)), g.integers(-3, 4, size=4)
    out, S = CR.conv_fwd([x], w, b, 2)
    assert out.dtype == np.int64 and S.dtype == np.int64 and (S >= np.abs(out)).all()
    CR.assert_exact(S)
    _close(out.astype(np.float64), CR.conv_fwd([x.astype(np.float64)], w, b, 2)[0])
    assert CR.as_exact(np.array([1.0, -2.0])).dtype == np.int64
    with pytest.raises(AssertionError):
        CR.as_exact(np.array([0.5]))
    with pytest.raises(AssertionError):
        CR.assert_exact(np.array([2 ** 24], dtype=np.int64))


# ---- bf16: rounding, the kernels' operand, and the widening condition of the bf16 table -------------------------------------------
def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _torch_bf16(a32):
    return torch.from_numpy(np.ascontiguousarray(a32)).to(torch.bfloat16).to(torch.float64).numpy()


def test_round_bf16_equals_torch_on_the_hard_values():
    """ties to even both ways, -0.0, bf16 subnormals, the largest finite value, one fp32 ulp either side of every tie, and a
    random sweep of bit patterns; bit for bit (the sign of zero included)"""
    ties = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x40FF8000, 0x00008000, 0x00018000, 0x80008000, 0x7F7E8000,
            0x007F8000, 0x00808000]                                   # ...8000: exactly half way; even / odd kept mantissa
    bits = []
    for t in ties:
        bits += [t - 1, t, t + 1]
    bits += [0x00000000, 0x80000000, 0x00000001, 0x00010000, 0x00004000, 0x007F0000, 0x7F7F0000, 0xFF7F0000, 0x7F7F7FFF,
             0x7F7F8000, 0x7F7FFFFF, 0x7F800000, 0xFF800000]          # zeros, subnormals, largest finite, overflow, infinities
    g = _rng(5)
    bits += [int(v) for v in g.integers(0, 2 ** 32, size=20000) if (int(v) >> 23) & 0xFF != 0xFF]
    a = _f32(bits)
    got, want = CR.round_bf16(a), _torch_bf16(a)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    # from fp64 there is no detour through fp32: a value just above a tie that fp32 would round ONTO the tie goes up
    x = 1.0 + 2.0 ** -8 + 2.0 ** -40
    assert CR.round_bf16(np.array([x]))[0] == 1.0 + 2.0 ** -7 and _torch_bf16(np.array([x], dtype=np.float32))[0] == 1.0
    assert CR.round_bf16(np.array([1.0 + 2.0 ** -8]))[0] == 1.0 and CR.round_bf16(np.array([1.0 + 3 * 2.0 ** -8]))[0] == 1.0 + 2.0 ** -6
    assert np.array_equal(CR.bf16_ulp(np.array([1.0, 1.99, 2.0, 0.0, 3e-39])), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133])


@pytest.mark.parametrize("act", R.ACTS)
def test_operand_bf16(act):
    """the operand is torch's bf16 rounding of torch's fp32 transform wherever it is not flagged ambiguous; a flagged one
    is at most one bf16 ulp away and A is exactly that ulp; a plain source is rounded directly and never flagged"""
    g = _rng(9)
    z = (g.normal(size=(2, 9, 11, 16)) * 2).astype(np.float32)
    z[0, 0, 0, :4] = [-0.0, 0.0, -1.0, 1.0 + 2.0 ** -8]
    sc, sh = (1 + 0.3 * g.normal(size=16)).astype(np.float32), g.normal(size=(16,)).astype(np.float32)
    zt = torch.from_numpy(z)
    t32 = R.activation(zt, act, dtype=torch.float32) * torch.from_numpy(sc) + torch.from_numpy(sh)
    want = t32.to(torch.bfloat16).to(torch.float64).numpy()
    op, A = CR.operand_bf16(z, act, sc, sh)
    clear = A == 0
    assert clear.mean() > 0.98
    assert np.array_equal(op[clear], want[clear])
    assert (np.abs(op - want)[~clear] <= A[~clear]).all() and np.array_equal(A[~clear], CR.bf16_ulp(op[~clear]))
    if act == "none":
        op0, A0 = CR.operand_bf16(z)
        assert not A0.any() and np.array_equal(op0, _torch_bf16(z))
    if act == "relu":                                                   # exact small integers, negative scale, -0.0: no rounding
        zi = g.integers(-3, 4, size=(1, 4, 4, 8)).astype(np.float32)
        zi[0, 0, 0, 0] = -0.0
        si, hi = np.array([-2, -1, 1, 2, 3, -2, 3, 1], np.float32), np.array([-2, -1, 1, 2, 2, 1, -1, -2], np.float32)
        opi, Ai = CR.operand_bf16(zi, "relu", si, hi)
        assert np.array_equal(opi, np.maximum(zi, 0) * si + hi) and np.abs(opi).max() <= 11
        assert not Ai.any()


def test_bf16_table_widening_condition():
    """every row of the bf16 table, every float variant and seed the GPU test uses: the widening of every output element
    stays within a quarter of the element's mean term, S / (4 K).  A row that breaks this gets another seed."""
    import conv_table as T
    import test_gpu_conv_bf16 as B
    worst = 0.0
    for r in B.ROWS:
        K = T.geom(r)["dot"]
        for i, (acts, pact) in enumerate(T.float_variants(r)):
            if not B.transformed(r, acts, pact):
                continue                                                # plain operands are rounded directly: nothing ambiguous
            d = T.make_data(r, "float", acts, pact, B._seed(r, 1 + i), want_ref=False)
            share = float((d["wid"] / (np.maximum(d["S"], T.TINY) / K)).max())
            worst = max(worst, share)
            assert share <= 0.25, (r.id, acts, pact, share)
    assert worst > 0.0                                                  # the condition is not vacuous: some operand is ambiguous
