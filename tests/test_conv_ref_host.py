"""Host: the plain references of tests/conv_ref.py against torch.nn.functional in fp64 (values, and gradients through
autograd) on a few odd shapes — N > 1, H != W, stride 2 on odd and even sizes, channel counts off every tile size — so that
the GPU tests of the convolution kernels can use them as the yardstick."""
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
