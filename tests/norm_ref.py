"""Plain fp64 reference of the normalisation kernels of libmseg_hip (csrc/norm.hip), written from the formulas of
BatchNorm2d / GroupNorm(8) / InstanceNorm2d applied AFTER the activation, y = norm(act(z)); nothing is imported from the
package under test and torch's own norm functions are not used (tests/test_norm_ref_host.py pins this file to them):

  forward tables scale / shift / mean / rstd + the BatchNorm running statistics          mseg_norm_stats
  the same tables from a convolution's partial sums part[rows][2][C] and a pixel count   mseg_norm_stats_from_conv
  backward dz, dgamma, dbeta, dbias (= the sum of dz over N and HW)                      mseg_norm_bwd
  the derivative of the five activations with torch's conventions

Tensors are NHWC with the pixels flattened: z, gy, dz [N][HW][C].  Statistics are taken per channel over (N, HW) for
BatchNorm, per (sample, group of C / 8 consecutive channels) over (HW, C / 8) for GroupNorm and per (sample, channel) over HW
for InstanceNorm, which has no affine parameters (gamma and beta are ignored, as the library ignores them).

bf16 storage (``bf16=True``), the contract of include/mseg_hip.h: z and gy ARE bf16 values (the caller passes the rounded
numbers); an activation that the forward materialises (``materialised=True``) is rounded to bf16 BEFORE the statistics are
taken and the backward uses that rounded tensor; dz is rounded to bf16 when stored and dbias is the sum of dz AS STORED.

The functions that a GPU test also evaluates in fp32 (to measure what the same formulas cost in the kernels' precision) take a
``dtype``, as in tests/pointwise_ref.py."""
import numpy as np
import torch

from pointwise_ref import ACTS, activation, bf16_bits_to_f64, bf16_round

NORMS = ("bn", "gn", "in")           # index = MSEG_NORM_*
GN_GROUPS = 8


def _t(x, dtype=torch.float64):
    return torch.as_tensor(x).to(dtype)


def _name(table, v):
    return table[v] if isinstance(v, int) else v


def bf16_store(x):
    """what a store + load of a bf16 tensor returns: the values rounded to nearest even in one step, as fp64"""
    x = _t(x)
    return torch.from_numpy(bf16_bits_to_f64(bf16_round(x.numpy()))).reshape(x.shape)


# ---- derivative of the activations ----------------------------------------------------------------------------------------------
def activation_grad(z, act, dtype=torch.float64, slope=0.01):
    """d act(z) / dz as torch's autograd gives it: ReLU and LeakyReLU take the value of the non-positive side at z == 0 (0 and
    the slope), ELU (alpha 1) is exp(z) for z <= 0 (1 at z == 0, from either side), Mish = z tanh(softplus(z)) differentiates
    softplus with its threshold 20: softplus'(z) = 1 above it, sigmoid(z) up to it."""
    name = _name(ACTS, act)
    x = _t(z, dtype)
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    if name == "none":
        return one
    if name == "relu":
        return torch.where(x > 0, one, zero)
    if name == "leakyrelu":
        return torch.where(x > 0, one, one * slope)
    if name == "elu":
        return torch.where(x > 0, one, torch.exp(torch.clamp(x, max=0.0)))
    if name == "mish":
        xc = torch.clamp(x, max=20.0)
        sp = torch.where(x > 20.0, x, torch.log1p(torch.exp(xc)))
        dsp = torch.where(x > 20.0, one, torch.sigmoid(xc))
        t = torch.tanh(sp)
        return t + x * (1.0 - t * t) * dsp
    raise ValueError(act)


# ---- the statistics' index sets ------------------------------------------------------------------------------------------------
def _fold(x, norm):
    """[N][HW][C] -> [B][M][G][K]: one statistic per (b, g), taken over (m, k)"""
    N, HW, Cc = x.shape
    if norm == "bn":
        return x.reshape(1, N * HW, Cc, 1)
    if norm == "gn":
        if Cc % GN_GROUPS:
            raise ValueError("GroupNorm(8) needs C % 8 == 0")
        return x.reshape(N, HW, GN_GROUPS, Cc // GN_GROUPS)
    if norm == "in":
        return x.reshape(N, HW, Cc, 1)
    raise ValueError(norm)


def _stat_shape(st, norm):
    """[B][G] -> [C] (BatchNorm), [N][8] (GroupNorm), [N][C] (InstanceNorm)"""
    return st.reshape(-1) if norm == "bn" else st


def _per_channel(st, norm, N, Cc):
    """a statistic [B][G] -> its value at every channel: [C] for BatchNorm, [N][C] otherwise"""
    if norm == "bn":
        return st.reshape(Cc)
    if norm == "gn":
        return st[:, :, None].expand(N, GN_GROUPS, Cc // GN_GROUPS).reshape(N, Cc)
    return st


def _affine(norm, Cc, gamma, beta, dtype):
    """gamma, beta [C]; 1 and 0 where absent, and always for InstanceNorm"""
    ga = torch.ones(Cc, dtype=dtype) if gamma is None or norm == "in" else _t(gamma, dtype)
    be = torch.zeros(Cc, dtype=dtype) if beta is None or norm == "in" else _t(beta, dtype)
    return ga, be


def _activated(z, act, bf16, materialised, a, dtype):
    """a = act(z) as the statistics see it: given (``a``: the stored tensor itself), or evaluated — and then rounded to bf16
    where bf16 storage materialises it"""
    if a is not None:
        return _t(a, dtype)
    v = activation(z, act, dtype)
    if bf16 and materialised:
        v = bf16_store(v.to(torch.float64)).to(dtype)
    return v


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def forward(z, act, norm, gamma=None, beta=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, *, bf16=False,
            materialised=False, a=None, dtype=torch.float64):
    """-> dict: a [N][HW][C]; scale, shift with y = a * scale + shift ([C] BatchNorm, [N][C] otherwise); mean, rstd, var (the
    biased variance) ([C] / [N][8] / [N][C]); abs_mean = the mean of |a| over the same sets (the scale of the mean's terms);
    for BatchNorm with running statistics given: running_mean, running_var after
        running = (1 - momentum) running + momentum (mean | var count / (count - 1)),  count = N HW,
    the correction left out when count == 1 (and running_mean_terms, the sum of the absolute values of the two terms).
    The variance is the two-pass mean of (a - mean)^2."""
    norm = _name(NORMS, norm)
    z = _t(z, dtype)
    N, HW, Cc = z.shape
    av = _activated(z, act, bf16, materialised, a, dtype)
    f = _fold(av, norm)
    count = f.shape[1] * f.shape[3]
    mean = f.sum(dim=(1, 3)) / count
    var = ((f - mean[:, None, :, None]) ** 2).sum(dim=(1, 3)) / count
    rstd = 1.0 / torch.sqrt(var + eps)
    ga, be = _affine(norm, Cc, gamma, beta, dtype)
    mean_c, rstd_c = _per_channel(mean, norm, N, Cc), _per_channel(rstd, norm, N, Cc)
    scale = ga * rstd_c
    shift = be - mean_c * ga * rstd_c
    out = {"a": av, "scale": scale, "shift": shift, "mean": _stat_shape(mean, norm), "rstd": _stat_shape(rstd, norm),
           "var": _stat_shape(var, norm), "abs_mean": _stat_shape(f.abs().sum(dim=(1, 3)) / count, norm), "count": count,
           "shift_terms": be.abs() + (mean_c * ga * rstd_c).abs()}
    if norm == "bn" and running_mean is not None:
        unbiased = var.reshape(Cc) * (count / (count - 1.0)) if count > 1 else var.reshape(Cc)
        out["running_mean"] = (1.0 - momentum) * _t(running_mean, dtype) + momentum * mean.reshape(Cc)
        out["running_mean_terms"] = ((1.0 - momentum) * _t(running_mean, dtype)).abs() + (momentum * mean.reshape(Cc)).abs()
        out["running_var"] = (1.0 - momentum) * _t(running_var, dtype) + momentum * unbiased
    return out


def forward_from_partials(part, count, gamma=None, beta=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None,
                          dtype=torch.float64):
    """BatchNorm tables from partial sums part[rows][2][C] (row r: sum of a, sum of a^2 over the pixels of row r) and the
    pixel count: mean = S / count, var = max(Q / count - mean^2, 0) — all the information the sums hold"""
    p = _t(part, dtype)
    Cc = p.shape[2]
    mean = p[:, 0].sum(dim=0) / count
    var = torch.clamp(p[:, 1].sum(dim=0) / count - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    ga, be = _affine("bn", Cc, gamma, beta, dtype)
    out = {"scale": ga * rstd, "shift": be - mean * ga * rstd, "mean": mean, "rstd": rstd, "var": var, "count": count,
           "abs_mean": p[:, 0].abs().sum(dim=0) / count, "shift_terms": be.abs() + (mean * ga * rstd).abs()}
    if running_mean is not None:
        unbiased = var * (count / (count - 1.0)) if count > 1 else var
        out["running_mean"] = (1.0 - momentum) * _t(running_mean, dtype) + momentum * mean
        out["running_mean_terms"] = ((1.0 - momentum) * _t(running_mean, dtype)).abs() + (momentum * mean).abs()
        out["running_var"] = (1.0 - momentum) * _t(running_var, dtype) + momentum * unbiased
    return out


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def backward(gy, z, act, norm, gamma=None, eps=1e-5, *, bf16=False, materialised=False, a=None, dtype=torch.float64):
    """gy = dL/dy [N][HW][C] -> dict: dz (exact), dz_stored (= dz, or its bf16 rounding under bf16 storage), dgamma, dbeta [C]
    (zero gradients of the absent parameters of InstanceNorm are returned all the same: sum of gy xhat and of gy), dbias [C] = the
    sum of dz_stored over N and HW, and the scales of these sums' terms for the tests' floors:
      k1 = gamma rstd ([C] / [N][C]);  dz_terms [N][HW][C] = (|k1 gy| + |k2 a| + |k3|) |act'(z)| with dz = (k1 gy + k2 a + k3) act'(z);
      dgamma_terms = sum rstd (|gy a| + |mean gy|),  dbeta_terms = sum |gy|,  dbias_terms = sum dz_terms.
    With xhat = (a - mean) rstd and the means m1, m2 of gamma gy and gamma gy xhat over the statistic's index set:
      da = rstd (gamma gy - m1 - xhat m2),   dz = da act'(z)."""
    norm = _name(NORMS, norm)
    z, g = _t(z, dtype), _t(gy, dtype)
    N, HW, Cc = z.shape
    fw = forward(z, act, norm, gamma, None, eps, bf16=bf16, materialised=materialised, a=a, dtype=dtype)
    av = fw["a"]
    ga, _ = _affine(norm, Cc, gamma, None, dtype)
    f = _fold(av, norm)
    B, M, G, K = f.shape
    mean = fw["mean"].reshape(B, G)[:, None, :, None]
    rstd = fw["rstd"].reshape(B, G)[:, None, :, None]
    xhat = (f - mean) * rstd
    gg = _fold(g * ga, norm)                                   # gamma gy
    count = M * K
    m1 = gg.sum(dim=(1, 3), keepdim=True) / count
    m2 = (gg * xhat).sum(dim=(1, 3), keepdim=True) / count
    da = (rstd * (gg - m1 - xhat * m2)).reshape(N, HW, Cc)
    d = activation_grad(z, act, dtype)
    dz = da * d
    stored = bf16_store(dz.to(torch.float64)).to(dtype) if bf16 else dz
    xh = xhat.reshape(N, HW, Cc)
    # the three tables of the library's form dz = (k1 gy + k2 a + k3) act'(z), for the scale of the terms only
    k1 = (rstd * _fold(ga.expand(N, HW, Cc), norm)).reshape(N, HW, Cc)
    k2 = (-rstd * rstd * m2).expand(B, M, G, K).reshape(N, HW, Cc)
    k3 = (-rstd * m1 + rstd * rstd * m2 * mean).expand(B, M, G, K).reshape(N, HW, Cc)
    dz_terms = ((k1 * g).abs() + (k2 * av).abs() + k3.abs()) * d.abs()
    rs, mu = rstd.expand(B, M, G, K).reshape(N, HW, Cc), mean.expand(B, M, G, K).reshape(N, HW, Cc)
    return {"dz": dz, "dz_stored": stored, "dgamma": (g * xh).sum(dim=(0, 1)), "dbeta": g.sum(dim=(0, 1)),
            "dbias": stored.sum(dim=(0, 1)), "k1": k1[:, 0, :] if norm != "bn" else k1[0, 0, :], "dz_terms": dz_terms,
            "dgamma_terms": (rs * ((g * av).abs() + (mu * g).abs())).sum(dim=(0, 1)), "dbeta_terms": g.abs().sum(dim=(0, 1)),
            "dbias_terms": dz_terms.sum(dim=(0, 1))}
