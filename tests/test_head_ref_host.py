"""CPU: the reference of tests/head_ref.py against F.conv2d and autograd in fp64, so that tests/test_gpu_head.py measures
the head kernels against something that is itself pinned."""
import pytest
import torch
import torch.nn.functional as F

import head_ref as R

TORCH_ACT = {"none": lambda v: v, "relu": F.relu, "leakyrelu": lambda v: F.leaky_relu(v, R.LEAKY_SLOPE), "elu": F.elu,
             "mish": F.mish}


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize("tables", ["none", "channel", "sample"])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("Co", [1, 4])
def test_head_reference_equals_conv2d_and_autograd(Co, act, tables):
    g = torch.Generator().manual_seed(29 + Co)
    N, H, W, Cc = 3, 5, 7, 12
    z = torch.randn(N, H * W, Cc, generator=g, dtype=torch.float64) * 2
    shape = {"none": None, "channel": (Cc,), "sample": (N, Cc)}[tables]
    scale = None if shape is None else torch.randn(shape, generator=g, dtype=torch.float64) * 0.3 + 1
    shift = None if shape is None else torch.randn(shape, generator=g, dtype=torch.float64) * 0.1
    w = torch.randn(Co, Cc, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(Co, generator=g, dtype=torch.float64).requires_grad_(True)
    gout = torch.randn(N, Co, H * W, generator=g, dtype=torch.float64)

    a = TORCH_ACT[act](z)                                          # [N][HW][C]
    if scale is not None:
        a = a * scale.reshape(-1, 1, Cc) + shift.reshape(-1, 1, Cc)
    xin = a.reshape(N, H, W, Cc).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xin, w.reshape(Co, Cc, 1, 1), b)
    y.backward(gout.reshape(N, Co, H, W))

    x = R.operand(z, act, scale, shift)
    assert _rel(x, a) <= 1e-15
    assert _rel(R.head_fwd(x, w.detach(), b.detach()), y.detach().reshape(N, Co, H * W)) <= 1e-14
    gy, dW, db = R.head_bwd(x, w.detach(), gout)
    assert _rel(gy, xin.grad.permute(0, 2, 3, 1).reshape(N, H * W, Cc)) <= 1e-14
    assert _rel(dW, w.grad) <= 1e-13
    assert _rel(db, b.grad) <= 1e-13


def test_head_reference_without_bias_and_in_fp32():
    g = torch.Generator().manual_seed(31)
    z = torch.randn(2, 9, 8, generator=g)
    w = torch.randn(3, 8, generator=g)
    x64, x32 = R.operand(z, "mish"), R.operand(z, "mish", dtype=torch.float32)
    assert x32.dtype == torch.float32 and x64.dtype == torch.float64
    assert torch.equal(R.head_fwd(x64, w), R.head_fwd(x64, w, torch.zeros(3)))
    assert 0 < _rel(R.head_fwd(x32, w).double(), R.head_fwd(x64, w)) < 1e-5
    z16 = z.to(torch.bfloat16)
    assert torch.equal(R.operand(z16, "none"), z16.double())       # a bf16 source is read as the values it holds
