"""Plain torch reference of the 1x1 output heads of libmseg_hip (csrc/head.hip), written from include/mseg_hip.h:

  x[n][p][c]    = act(z[n][p][c]) * scale[n or -][c] + shift[n or -][c]      the norm-on-load operand (MsegSrc)
  out[n][co][p] = sum_c W[co][c] x[n][p][c] + b[co]                          mseg_head_fwd
  gy[n][p][c]   = sum_co gout[n][co][p] W[co][c]                             mseg_head_bwd (gradient w.r.t. x)
  dW[co][c]     = sum_{n,p} gout[n][co][p] x[n][p][c],  db[co] = sum_{n,p} gout[n][co][p]

fp64 is the reference; ``dtype=torch.float32`` evaluates the same statements with torch on the CPU in fp32 and exists only
to measure what they cost in the kernels' precision (e_ref).  tests/test_head_ref_host.py pins both directions to
F.conv2d and autograd in fp64.
"""
import numpy as np
import torch

import pointwise_ref as P

ACTS = P.ACTS
LEAKY_SLOPE = float(np.float32(0.01))       # the fp32 number the header's 0.01 denotes


def operand(z, act, scale=None, shift=None, dtype=torch.float64):
    """z [N][HW][C] (any float type; bf16 values are taken as they are) -> x; scale / shift None, [C] or [N][C]"""
    x = P.activation(torch.as_tensor(z).to(dtype), act, dtype=dtype, slope=LEAKY_SLOPE)
    if scale is not None:
        sc, sh = torch.as_tensor(scale).to(dtype), torch.as_tensor(shift).to(dtype)
        if sc.dim() == 1:
            sc, sh = sc[None], sh[None]
        x = x * sc[:, None, :] + sh[:, None, :]
    return x


def head_fwd(x, w, b=None):
    """-> out [N][Co][HW] in the type of x"""
    out = torch.einsum("npc,oc->nop", x, torch.as_tensor(w).to(x.dtype))
    return out if b is None else out + torch.as_tensor(b).to(x.dtype)[None, :, None]


def head_bwd(x, w, gout):
    """-> (gy [N][HW][C], dW [Co][C], db [Co]) in the type of x"""
    g = torch.as_tensor(gout).to(x.dtype)
    gy = torch.einsum("nop,oc->npc", g, torch.as_tensor(w).to(x.dtype))
    return gy, torch.einsum("nop,npc->oc", g, x), g.sum(dim=(0, 2))
