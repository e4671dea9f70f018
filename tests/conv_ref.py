"""Plain references of the convolution family of libmseg_hip (mseg_igemm / mseg_wgrad), written from the formulas in
include/mseg_hip.h alone (nothing is imported from the package under test).  numpy on the CPU, one loop over the taps.

All activation tensors are NHWC ([N][H][W][C]), weights are in torch's layouts:

  operand       act(z) * scale + shift, tables per channel [C] or per sample [N][C]          MsegSrc (norm-on-load)
  conv_fwd      Conv2d 3x3, stride 1 / 2, pad 1, of the concatenation of its sources         mseg_igemm MODE_CONV
  conv_dgrad    its data gradient                                                            mseg_igemm MODE_TCONV
  convT_fwd     ConvTranspose2d 2x2, stride 2                                                mseg_igemm EPI_SCATTER2X2
  convT_dgrad   its data gradient (a 2x2 stride-2 convolution of the output gradient)        mseg_igemm MODE_CONV, KH = 2
  wgrad         G[m][n][ky][kx] = sum_p P[p][m] * Q[gather(p, ky, kx)][n]                    mseg_wgrad
  round_bf16    round to nearest even onto the bf16 grid (values returned as float64)         MSEG_PREC_BF16 / MSEG_ST_BF16
  operand_bf16  the operand a bf16 matrix-core kernel forms: bf16(fma(act(z), scale, shift))  and where that is ambiguous

Every function works in the dtype of its arguments: float64 for the yardstick of the float tests, int64 for the exact
tests (small-integer operands; no rounding anywhere).  Every function returns ``(result, S)``: S is the same operation on
the absolute values, sum |a| |w| (+ |bias|, + |base| of an accumulating destination) — the natural scale of the rounding
error of each output element, and an upper bound of the magnitude of every partial sum whatever the summation order.
tests/test_conv_ref_host.py pins all of them to torch.nn.functional through autograd in fp64."""
import numpy as np
import torch

import pointwise_ref as R

EXACT_LIMIT = 2 ** 24        # integers below it are exact in fp32


def operand(z, act="none", scale=None, shift=None):
    """the norm-on-load value act(z) * scale + shift of an NHWC tensor in fp64 (numpy); ``act`` is a name or a MSEG_ACT_* id;
    scale / shift [C] (shared), [N][C] (per sample) or None.  The fp64 activation is pointwise_ref's."""
    v = R.activation(torch.as_tensor(np.asarray(z)), act).numpy()
    if scale is not None:
        sc, sh = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
        if sc.ndim == 1:
            sc, sh = sc[None], sh[None]
        v = v * sc[:, None, None, :] + sh[:, None, None, :]
    return v


def as_exact(x):
    """an integer-valued float array -> int64 (asserts that it holds integers)"""
    x = np.asarray(x)
    r = np.rint(x)
    assert np.array_equal(r, x), "the exact tests need integer operands"
    return r.astype(np.int64)


def assert_exact(S):
    """the exact tests' premise: every partial sum of every output element is an integer below 2^24, in any order"""
    assert S.dtype == np.int64 and int(S.max()) < EXACT_LIMIT, f"sum of magnitudes {int(S.max())} reaches 2^24"


MAGNITUDES_ONLY = False     # set by a caller that needs S alone (the widening condition of the bf16 table): result = S


def _both(fn, arrays, bias=None, base=None):
    """fn on the arrays and on their absolute values; bias (broadcast over the last axis) and base added likewise"""
    S = fn(*[np.abs(a) for a in arrays])
    out = S.copy() if MAGNITUDES_ONLY else fn(*arrays)
    if bias is not None:
        b = np.asarray(bias).astype(out.dtype)
        out, S = out + b, S + np.abs(b)
    if base is not None:
        b = np.asarray(base).astype(out.dtype)
        out, S = out + b, S + np.abs(b)
    return out, S


def _pad1(x):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))


# ---- Conv2d 3x3, pad 1 ------------------------------------------------------------------------------------------------------------
def out_size(n, stride):
    return (n + 2 - 3) // stride + 1


def _conv3x3(x, w, stride):
    N, H, W, _ = x.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    out = np.zeros((N, Ho, Wo, w.shape[0]), dtype=x.dtype)
    if stride == 1 and w.shape[0] < w.shape[1]:
        # fewer output than input channels: one matmul per tap on the tensor as it lies, then shift the (smaller) product
        for ky in range(3):
            for kx in range(3):
                y = np.tensordot(x, w[:, :, ky, kx], axes=([3], [1]))
                dy, dx = ky - 1, kx - 1
                out[:, max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] += \
                    y[:, max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
        return out
    xp = _pad1(x)
    for ky in range(3):
        for kx in range(3):
            patch = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out += np.tensordot(patch, w[:, :, ky, kx], axes=([3], [1]))
    return out


def conv_fwd(xs, w, bias=None, stride=1, base=None):
    """xs: list of one or two operands [N][H][W][Ci] (concatenated along C); w (Cout, sum Ci, 3, 3); bias [Cout] or None
    -> [N][Ho][Wo][Cout]"""
    x = np.concatenate(list(xs), axis=3)
    w = np.asarray(w).astype(x.dtype)
    assert w.shape[1:] == (x.shape[3], 3, 3)
    return _both(lambda a, b: _conv3x3(a, b, stride), (x, w), bias, base)


def _conv3x3_dgrad(gy, w, stride, H, W):
    N, Ho, Wo, _ = gy.shape
    dxp = np.zeros((N, H + 2, W + 2, w.shape[1]), dtype=gy.dtype)
    for ky in range(3):
        for kx in range(3):
            dxp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] += \
                np.tensordot(gy, w[:, :, ky, kx], axes=([3], [0]))
    return dxp[:, 1:H + 1, 1:W + 1]


def conv_dgrad(gy, w, stride, H, W, base=None):
    """gy [N][Ho][Wo][Cout] (an operand: the C ABI lets the gradient be transformed on load like any source); w (Cout, Cin,
    3, 3); H, W = size of the convolution's input -> dx [N][H][W][Cin]"""
    gy = np.asarray(gy)
    w = np.asarray(w).astype(gy.dtype)
    assert gy.shape[1:3] == (out_size(H, stride), out_size(W, stride)) and w.shape[0] == gy.shape[3]
    return _both(lambda a, b: _conv3x3_dgrad(a, b, stride, H, W), (gy, w), None, base)


# ---- ConvTranspose2d 2x2, stride 2 ---------------------------------------------------------------------------------------------
def _convT(x, w):
    N, H, W, _ = x.shape
    out = np.zeros((N, 2 * H, 2 * W, w.shape[1]), dtype=x.dtype)
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2] = np.tensordot(x, w[:, :, a, b], axes=([3], [0]))
    return out


def convT_fwd(x, w, bias=None, base=None):
    """x [N][H][W][Cin]; w (Cin, Cout, 2, 2) -> y [N][2H][2W][Cout], y[n, 2y+a, 2x+b, co] = bias[co] + sum_ci x w[ci, co, a, b]"""
    x = np.asarray(x)
    w = np.asarray(w).astype(x.dtype)
    assert w.shape[0] == x.shape[3] and w.shape[2:] == (2, 2)
    return _both(_convT, (x, w), bias, base)


def _convT_dgrad(gy, w):
    N, H2, W2, _ = gy.shape
    out = np.zeros((N, H2 // 2, W2 // 2, w.shape[0]), dtype=gy.dtype)
    for a in range(2):
        for b in range(2):
            out += np.tensordot(gy[:, a::2, b::2], w[:, :, a, b], axes=([3], [1]))
    return out


def convT_dgrad(gy, w, base=None):
    """gy [N][2H][2W][Cout]; w (Cin, Cout, 2, 2) -> dx [N][H][W][Cin]"""
    gy = np.asarray(gy)
    w = np.asarray(w).astype(gy.dtype)
    assert w.shape[1] == gy.shape[3] and gy.shape[1] % 2 == 0 and gy.shape[2] % 2 == 0
    return _both(_convT_dgrad, (gy, w), None, base)


# ---- weight gradients -----------------------------------------------------------------------------------------------------------
def _wgrad(P, Q, K, stride, pad):
    N, Hp, Wp, M = P.shape
    Qp = np.pad(Q, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    G = np.zeros((M, Q.shape[3], K, K), dtype=P.dtype)
    for ky in range(K):
        for kx in range(K):
            patch = Qp[:, ky:ky + stride * (Hp - 1) + 1:stride, kx:kx + stride * (Wp - 1) + 1:stride]
            G[:, :, ky, kx] = np.tensordot(P, patch, axes=([0, 1, 2], [0, 1, 2]))
    return G


def wgrad(P, Qs, K, stride, nch_store=None):
    """P [N][Hp][Wp][M]; Qs: one or two operands [N][Hq][Wq][Ci] (concatenated); K = 3: the 3x3 convolution (pad 1, stride 1 / 2;
    P = output gradient, Q = input) -> torch's Conv2d.weight gradient (M, Nch, 3, 3); K = 2: ConvTranspose2d 2x2 stride 2
    (pad 0; P = input, Q = output gradient) -> (M, Nch, 2, 2).  Only the first nch_store of the Nch columns are kept."""
    P = np.asarray(P)
    Q = np.concatenate([np.asarray(q) for q in Qs], axis=3).astype(P.dtype)
    pad = 1 if K == 3 else 0
    assert K in (2, 3) and (K == 3 or stride == 2)
    if K == 3:
        assert P.shape[1:3] == (out_size(Q.shape[1], stride), out_size(Q.shape[2], stride))
    else:
        assert Q.shape[1:3] == (2 * P.shape[1], 2 * P.shape[2])
    G, S = _both(lambda a, b: _wgrad(a, b, K, stride, pad), (P, Q))
    n = Q.shape[3] if nch_store is None else nch_store
    return np.ascontiguousarray(G[:, :n]), np.ascontiguousarray(S[:, :n])


# ---- bf16 (MSEG_PREC_BF16 operands, MSEG_ST_BF16 tensors) -----------------------------------------------------------------------
BF16_MIN_EXP = -133          # the smallest bf16 subnormal is 2^-133
TRANSFORM_BAND = 32 * 2.0 ** -24     # relative allowance of a transcendental operand transform (as in the fp32 table)


def _t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _ulp_t(t):
    """2^(exponent of |t| - 7), at least 2^-133, read off the exponent field of the fp64 value"""
    e = (t.contiguous().view(torch.int64) >> 52) & 0x7FF               # biased exponent; 0 for zero (and fp64 subnormals)
    return (torch.clamp(e - 7, min=1023 + BF16_MIN_EXP) << 52).view(torch.float64)


def _round32_t(t32):
    """fp32 -> bf16 values (still fp32), ties to even, on the bit pattern: add half an ulp less one, plus the kept part's
    last bit, and cut.  Finite input; beyond the largest finite bf16 value this gives infinity, as the hardware does."""
    b = t32.contiguous().view(torch.int32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & -65536).view(torch.float32)


def _round_t(t):
    if t.dtype == torch.float32:
        return _round32_t(t).to(torch.float64)
    q = _ulp_t(t)
    r = torch.round(t / q) * q                                         # t / q is exact (q a power of two); half to even
    r = torch.where(r.abs() >= 2.0 ** 128, torch.copysign(torch.full_like(t, float("inf")), t), r)
    return torch.where(torch.isfinite(t), r, t)


def bf16_ulp(a):
    """the spacing of the bf16 grid at |a| (float64); 2^-133 at zero and below the subnormals.  (torch elementwise
    arithmetic in fp64: the same IEEE operations as numpy's, on all cores — the tables hold tensors of 3e7 elements)"""
    return _ulp_t(_t64(a)).numpy()


def round_bf16(a):
    """fp32 or fp64 values -> the nearest bf16 value, ties to even, as float64 (no intermediate rounding to fp32); keeps the
    sign of zero, overflows to infinity beyond the largest finite bf16 value like the hardware conversion"""
    a = np.asarray(a)
    if a.dtype == np.float32 and np.isfinite(a).all():
        return _round_t(torch.from_numpy(np.ascontiguousarray(a))).numpy()
    return _round_t(_t64(a)).numpy()


def operand_bf16(z, act="none", scale=None, shift=None):
    """The operand of a bf16 matrix-core kernel and its ambiguity -> (op, A), both float64.

    A plain source (no activation, no table) is rounded directly: deterministic, A = 0.  A transformed one is
    bf16(fma(act(z), scale, shift)) with the fma in fp32.  For none / relu the fp32 fma is emulated (product and sum in
    fp64 — the product of two fp32 values is exact there — then one rounding to fp32) and the operand is AMBIGUOUS when the
    fp64 value lies within one fp32 ulp of a bf16 tie: an fma, a separate multiply and add, and this emulation may then
    land on different sides.  For leakyrelu / elu / mish the activation itself carries TRANSFORM_BAND relative error on the
    device, taken relative to |act * scale| + |shift| (the shift may cancel the product), plus the same fp32 ulp.
    A = one bf16 ulp of the operand where it is ambiguous, 0 elsewhere."""
    name = act if isinstance(act, str) else R.ACTS[act]
    z = np.asarray(z)
    if name == "none" and scale is None:
        return round_bf16(z), np.zeros(z.shape)
    a = R.activation(_t64(z), name)
    if scale is None:
        prod, sh = a, torch.zeros(1, dtype=torch.float64)
    else:
        sc, sh = _t64(scale), _t64(shift)
        if sc.dim() == 1:
            sc, sh = sc[None], sh[None]
        prod, sh = a * sc[:, None, None, :], sh[:, None, None, :]
    v = prod + sh
    q = _ulp_t(v)
    op = _round_t(v.to(torch.float32))
    band = q * 2.0 ** -16                                              # one fp32 ulp
    if name not in ("none", "relu"):
        band = band + TRANSFORM_BAND * (prod.abs() + sh.abs())
    t = v.abs() / q
    tie_distance = (t - torch.floor(t) - 0.5).abs() * q               # to the nearest midpoint between two bf16 values
    A = torch.where(tie_distance <= band, _ulp_t(op), torch.zeros((), dtype=torch.float64))
    return op.numpy(), A.numpy()
