"""Plain fp64 references of the small element-wise / reduction kernels of libmseg_hip, written from the formulas in
include/mseg_hip.h alone (nothing is imported from the package under test):

  regression losses (smooth-L1 beta 1 / L1 / MSE, mean) and their gradients        mseg_regression_loss / _bwd
  ce_dice: the six Dice sums + the cross-entropy sum, and the analytic gradient     mseg_ce_dice_fwd / _bwd
  MaxPool2d(2, 2) of act(z) * scale + shift with first-maximum routing              mseg_maxpool2x2_fwd / _bwd
  softmax over 3 classes + crop of the top / left pad + CHW -> HWC                  mseg_softmax3_hwc
  the five activations                                                              mseg_activation
  round-to-nearest-even fp32 -> bf16 on the bit pattern                             mseg_f32_to_bf16
  the zero-padded [T][Rpad][Cpad] weight repack                                     mseg_pack_weight(s_multi)

tests/test_pointwise_ref_host.py pins every one of them to torch on the CPU (fp64 values, autograd gradients); the GPU
tests then use them as the yardstick.  The functions that a test also evaluates in fp32 (to measure what the same formula
costs in the kernels' precision) take a ``dtype``.
"""
import numpy as np
import torch

KINDS = {"smooth_l1": 0, "l1": 1, "l2": 2}
ACTS = ("none", "relu", "leakyrelu", "elu", "mish")      # index = MSEG_ACT_*


def _t(x, dtype=torch.float64):
    return torch.as_tensor(x).to(dtype)


# ---- regression losses: kind 0 smooth-L1 (beta 1), 1 L1, 2 MSE; mean over all elements --------------------------------------
def reg_terms(pred, target, kind):
    d = _t(pred) - _t(target)
    ad = d.abs()
    if kind == 0:
        return torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)
    if kind == 1:
        return ad
    if kind == 2:
        return d * d
    raise ValueError(kind)


def reg_loss(pred, target, kind):
    """the mean loss, a python float (fp64)"""
    return reg_terms(pred, target, kind).mean().item()


def reg_grad(pred, target, kind, gscale=1.0):
    """d(gscale * mean loss) / d pred.  L1 has gradient 0 at d == 0; smooth-L1 has +-1 from |d| == 1 on."""
    d = _t(pred) - _t(target)
    if kind == 0:
        g = torch.where(d.abs() < 1.0, d, torch.sign(d))
    elif kind == 1:
        g = torch.sign(d)
    elif kind == 2:
        g = 2.0 * d
    else:
        raise ValueError(kind)
    return g * (float(gscale) / d.numel())


# ---- ce_dice: logits [N][3][HW], labels [N][HW] -------------------------------------------------------------------------------
def _softmax3(logits, dtype):
    l = _t(logits, dtype)
    m = l.max(dim=1, keepdim=True).values
    e = torch.exp(l - m)
    s = e.sum(dim=1, keepdim=True)
    return e / s, m + torch.log(s)


def ce_dice_fwd(logits, labels):
    """-> (sums6, ce_sum): sums6 = {sum g1 p1, sum p1^2, sum g1, sum g2 p2, sum p2^2, sum g2}, ce_sum = sum (lse - l_y)"""
    p, lse = _softmax3(logits, torch.float64)
    y = torch.as_tensor(labels).to(torch.int64)
    ly = torch.gather(_t(logits), 1, y[:, None, :])
    ce_sum = (lse - ly).sum().item()
    sums = []
    for c in (1, 2):
        g = (y == c).to(torch.float64)
        sums += [(g * p[:, c]).sum().item(), (p[:, c] * p[:, c]).sum().item(), g.sum().item()]
    return np.array(sums, dtype=np.float64), ce_sum


def ce_dice_loss(sums6, ce_sum, total_px, with_dice=True):
    """CE mean + 0.5 * sum_{c=1,2} c * (1 - (2 I_c + 1) / (G_c + P_c + 1))"""
    loss = ce_sum / total_px
    if with_dice:
        for c in (1, 2):
            i, p, g = sums6[(c - 1) * 3:(c - 1) * 3 + 3]
            loss += 0.5 * c * (1.0 - (2.0 * i + 1.0) / (g + p + 1.0))
    return loss


def ce_dice_grad(logits, labels, sums6, total_px, dice_weight=1.0, gscale=1.0, with_dice=True, dtype=torch.float64):
    """gscale * d/dlogit [ ce_sum / total_px + dice_weight * 0.5 * sum_c c * (1 - (2 I_c + 1) / (G_c + P_c + 1)) ] where the
    sums I, P, G are the ones PASSED IN (a data-parallel caller passes the all-reduced sums, of which this tensor's pixels
    are a part: dI_c/dp_c = g_c and dP_c/dp_c = 2 p_c at every pixel of this tensor whatever the other ranks hold).
      dDice_c/dp_c = -2 g_c / B_c + 2 A_c p_c / B_c^2,  A_c = 2 I_c + 1,  B_c = G_c + P_c + 1;  dp_c/dl_k = p_c (delta_ck - p_k)"""
    p, _ = _softmax3(logits, dtype)
    y = torch.as_tensor(labels).to(torch.int64)
    onehot = torch.stack([(y == k) for k in range(3)], dim=1).to(dtype)
    grad = (p - onehot) / torch.tensor(float(total_px), dtype=dtype)
    if with_dice:
        s = torch.as_tensor(np.asarray(sums6, dtype=np.float64)).to(dtype)
        for c in (1, 2):
            i, pp, g = s[(c - 1) * 3], s[(c - 1) * 3 + 1], s[(c - 1) * 3 + 2]
            a, b = 2.0 * i + 1.0, g + pp + 1.0
            dd = float(dice_weight) * 0.5 * c * (-2.0 * onehot[:, c] / b + 2.0 * a * p[:, c] / (b * b))    # [N][HW]
            delta = torch.zeros(3, dtype=dtype)
            delta[c] = 1.0
            grad = grad + (dd * p[:, c])[:, None, :] * (delta[None, :, None] - p)
    return grad * torch.tensor(float(gscale), dtype=dtype)


# ---- activations ---------------------------------------------------------------------------------------------------------------
def activation(z, act, dtype=torch.float64, slope=0.01):
    """MSEG_ACT_*: none, relu, leakyrelu (negative_slope 0.01), elu (alpha 1), mish = x tanh(softplus(x)) with softplus's
    threshold 20.  ``act`` is a name or an id."""
    name = ACTS[act] if isinstance(act, int) else act
    x = _t(z, dtype)
    if name == "none":
        return x
    if name == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    if name == "leakyrelu":
        return torch.where(x > 0, x, x * slope)
    if name == "elu":
        return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0.0)))
    if name == "mish":
        sp = torch.where(x > 20.0, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))
        return x * torch.tanh(sp)
    raise ValueError(act)


# ---- MaxPool2d(2, 2) of a norm-on-load operand, NHWC -------------------------------------------------------------------------
def transform(z, act, scale=None, shift=None):
    """act(z) * scale + shift on [N][H][W][C]; scale / shift [C] (shared) or [N][C] (per sample) or None"""
    v = activation(z, act)
    if scale is not None:
        sc, sh = _t(scale), _t(shift)
        if sc.dim() == 1:
            sc, sh = sc[None], sh[None]
        v = v * sc[:, None, None, :] + sh[:, None, None, :]
    return v


def _windows(v):
    """[N][H][W][C] -> [4][N][H/2][W/2][C], window elements in row-major order (k = 2 dy + dx)"""
    return torch.stack([v[:, 0::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 0::2], v[:, 1::2, 1::2]])


def maxpool_fwd(z, act, scale=None, shift=None):
    """-> (pooled [N][H/2][W/2][C], arg [N][H/2][W/2][C]): arg = the FIRST maximum of the window in row-major order"""
    w = _windows(transform(z, act, scale, shift))
    best, arg = w[0].clone(), torch.zeros(w[0].shape, dtype=torch.int64)
    for k in (1, 2, 3):
        take = w[k] > best                      # strictly greater: an equal later element does not take over
        best = torch.where(take, w[k], best)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    return best, arg


def maxpool_bwd(arg, gout, gin_old=None):
    """gin [N][H][W][C]: gout at the first maximum of its window, 0 elsewhere; added to ``gin_old`` when that is given"""
    g = _t(gout)
    N, Ho, Wo, Cc = g.shape
    gin = torch.zeros((N, 2 * Ho, 2 * Wo, Cc), dtype=torch.float64)
    for k in range(4):
        gin[:, (k >> 1)::2, (k & 1)::2] = torch.where(arg == k, g, torch.zeros_like(g))
    return gin if gin_old is None else gin + _t(gin_old)


# ---- softmax over 3 classes, crop, transpose ----------------------------------------------------------------------------------
def softmax_crop_hwc(logits_chw, pad_y, pad_x):
    """[3][Hp][Wp] logits -> [Hp - pad_y][Wp - pad_x][3] probabilities, the top / left pad cropped"""
    p, _ = _softmax3(_t(logits_chw)[None], torch.float64)
    return p[0, :, pad_y:, pad_x:].permute(1, 2, 0).contiguous()


# ---- fp32 -> bf16, round to nearest even, on the bit pattern ------------------------------------------------------------------
def bf16_rne_bits(x):
    """float32 array -> uint16 array of bf16 bit patterns.  u + 0x7fff + (bit 16 of u) carries into the kept half exactly when
    the dropped half is above 0x8000, or equal to it with an odd kept half; an overflowing mantissa carries into the
    exponent (FLT_MAX -> inf).  NaN keeps its sign and upper payload and gets the quiet bit."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_bits_to_f64(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_round(x64):
    """fp64 array -> bf16 bit patterns, rounded to nearest even in ONE step (no intermediate fp32 rounding): the quantum of
    a value with binary exponent e (|v| in [2^(e-1), 2^e)) is 2^(e-8), and 2^-133 throughout the subnormal range"""
    v = np.asarray(x64, dtype=np.float64)
    _, e = np.frexp(v)
    q = np.maximum(e - 8, -133).astype(np.float64)
    with np.errstate(over="ignore"):
        r = (np.rint(v / np.exp2(q)) * np.exp2(q)).astype(np.float32)      # exact in fp32, or +-inf from 2^128 on
    r = np.where(np.isfinite(v), r, v.astype(np.float32))
    return (np.ascontiguousarray(r).view(np.uint32) >> 16).astype(np.uint16)


# ---- weight repack --------------------------------------------------------------------------------------------------------------
def pack_weight(src, T, R, Rpad, Cc, Cpad, st, sr, sc):
    """dst[(t * Rpad + r) * Cpad + c] = (r < R && c < C) ? src[t * st + r * sr + c * sc] : +0"""
    flat = np.asarray(src, dtype=np.float32).reshape(-1)
    dst = np.zeros((T, Rpad, Cpad), dtype=np.float32)
    t, r, c = np.meshgrid(np.arange(T), np.arange(R), np.arange(Cc), indexing="ij")
    dst[:, :R, :Cc] = flat[t * st + r * sr + c * sc]
    return dst.reshape(-1)
