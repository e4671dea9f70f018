"""CPU: the fp64 references of tests/pointwise_ref.py against torch on the CPU in fp64 (values and autograd gradients), so
that the GPU tests of tests/test_gpu_pointwise.py measure the kernels against something that is itself pinned."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R
from oracle import unet_ref

TORCH_LOSS = {0: F.smooth_l1_loss, 1: F.l1_loss, 2: F.mse_loss}


def _close(a, b, rel=1e-13, what=""):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    assert a.shape == b.shape, what
    err = (a - b).abs().max().item()
    assert err <= rel * max(b.abs().max().item(), 1e-300), f"{what}: {err:.3e}"


# ---- regression losses ----------------------------------------------------------------------------------------------------------
def _reg_inputs():
    g = torch.Generator().manual_seed(3)
    target = torch.randint(-4096, 4097, (600,), generator=g).to(torch.float64) / 64
    d = torch.randn(600, generator=g, dtype=torch.float64) * 1.5
    special = torch.tensor([0.0, 1.0, -1.0, 1 - 2.0 ** -10, -(1 - 2.0 ** -10), 1 + 2.0 ** -10, -(1 + 2.0 ** -10), 50.0, -50.0])
    d[:special.numel()] = special.to(torch.float64)
    return target + d, target, special.numel()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_regression_reference_equals_torch(kind):
    pred, target, _ = _reg_inputs()
    p = pred.clone().requires_grad_(True)
    loss = TORCH_LOSS[kind](p, target)
    (0.37 * loss).backward()
    assert abs(R.reg_loss(pred, target, kind) - loss.item()) <= 1e-14 * abs(loss.item())
    _close(R.reg_grad(pred, target, kind, 0.37), p.grad, what="gradient")


def test_regression_gradient_at_the_branch_points():
    """d = 0 exactly: L1 has gradient 0 (torch's sign(0)); |d| = 1 exactly: smooth-L1 is on its linear branch, +-1"""
    pred = torch.tensor([0.25, 1.25, -0.75, 0.25 + 1 - 2.0 ** -10], dtype=torch.float64)
    target = torch.full((4,), 0.25, dtype=torch.float64)
    for kind, want in ((1, [0.0, 1.0, -1.0, 1.0]), (0, [0.0, 1.0, -1.0, 1 - 2.0 ** -10])):
        p = pred.clone().requires_grad_(True)
        TORCH_LOSS[kind](p, target, reduction="sum").backward()
        assert p.grad.tolist() == want
        assert (R.reg_grad(pred, target, kind) * 4).tolist() == want


# ---- ce_dice ---------------------------------------------------------------------------------------------------------------------
def _ce_inputs(absent=False):
    g = torch.Generator().manual_seed(7)
    N, H, W = 3, 5, 7
    logits = torch.randn(N, 3, H, W, generator=g, dtype=torch.float64) * 3
    logits[0, :, 0, 0] = torch.tensor([80.0, 0.0, -80.0])
    logits[1, :, 2, 3] = torch.tensor([1.5, 1.5, 1.5])
    labels = torch.randint(0, 2 if absent else 3, (N, H, W), generator=g)
    return logits, labels


@pytest.mark.parametrize("absent", [False, True])
def test_ce_dice_reference_equals_oracle(absent):
    """own sums, dice_weight 1, total_px = N HW: the loss assembled from (sums6, ce_sum) and the analytic gradient against
    oracle/unet_ref.ce_dice and its autograd gradient in fp64"""
    logits, labels = _ce_inputs(absent)
    N, _, H, W = logits.shape
    l = logits.clone().requires_grad_(True)
    loss = unet_ref.ce_dice(l, labels)
    (0.37 * loss).backward()
    flat, lab = logits.reshape(N, 3, H * W), labels.reshape(N, H * W)
    sums6, ce_sum = R.ce_dice_fwd(flat, lab)
    if absent:
        assert sums6[3] == 0.0 and sums6[5] == 0.0 and sums6[4] > 0.0
    assert abs(R.ce_dice_loss(sums6, ce_sum, N * H * W) - loss.item()) <= 1e-13 * abs(loss.item())
    grad = R.ce_dice_grad(flat, lab, sums6, N * H * W, 1.0, 0.37, True)
    _close(grad.reshape(N, 3, H, W), l.grad, rel=1e-12, what="ce_dice gradient")


def test_plain_cross_entropy_reference_equals_torch():
    logits, labels = _ce_inputs()
    N, _, H, W = logits.shape
    l = logits.clone().requires_grad_(True)
    loss = F.cross_entropy(l, labels)
    loss.backward()
    flat, lab = logits.reshape(N, 3, H * W), labels.reshape(N, H * W)
    sums6, ce_sum = R.ce_dice_fwd(flat, lab)
    assert abs(R.ce_dice_loss(sums6, ce_sum, N * H * W, with_dice=False) - loss.item()) <= 1e-13 * abs(loss.item())
    _close(R.ce_dice_grad(flat, lab, sums6, N * H * W, with_dice=False).reshape(N, 3, H, W), l.grad, rel=1e-12)


def test_ce_dice_gradient_for_global_sums_is_the_two_rank_gradient():
    """data-parallel form: two ranks hold halves of a batch; each passes the all-reduced sums, dice_weight = world size 2
    and its own pixel count; averaging the two gradients as the gradient all-reduce does gives the gradient of the loss of
    the whole batch (which is what the reference computes on the gathered batch)"""
    logits, labels = _ce_inputs()
    logits, labels = logits[:2], labels[:2]
    _, _, H, W = logits.shape
    l = logits.clone().requires_grad_(True)
    unet_ref.ce_dice(l, labels).backward()
    flat, lab = logits.reshape(2, 3, H * W), labels.reshape(2, H * W)
    sums6, _ = R.ce_dice_fwd(flat, lab)
    for r in range(2):
        g = R.ce_dice_grad(flat[r:r + 1], lab[r:r + 1], sums6, H * W, dice_weight=2.0)
        _close(g.reshape(3, H, W) / 2, l.grad[r], rel=1e-12, what=f"rank {r}")


# ---- max-pool ----------------------------------------------------------------------------------------------------------------------
def test_maxpool_reference_equals_torch_forward_and_backward():
    g = torch.Generator().manual_seed(11)
    N, Cc, H, W = 2, 4, 6, 10
    z = torch.randint(-32, 33, (N, H, W, Cc), generator=g).to(torch.float64) / 8
    scale = torch.tensor([0.5, -1.0, 2.0, -2.0], dtype=torch.float64)
    shift = torch.tensor([0.0, 1.0, -1.0, 0.0], dtype=torch.float64)
    gout = torch.randint(-16, 17, (N, H // 2, W // 2, Cc), generator=g).to(torch.float64) / 16
    for act in ("relu", "none"):
        v = R.transform(z, act, scale, shift).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        want = F.max_pool2d(v, 2, 2)
        want.backward(gout.permute(0, 3, 1, 2))
        out, arg = R.maxpool_fwd(z, act, scale, shift)
        assert torch.equal(out, want.detach().permute(0, 2, 3, 1))
        assert torch.equal(R.maxpool_bwd(arg, gout), v.grad.permute(0, 2, 3, 1))
        old = torch.randint(-16, 17, (N, H, W, Cc), generator=g).to(torch.float64) / 16
        assert torch.equal(R.maxpool_bwd(arg, gout, old), v.grad.permute(0, 2, 3, 1) + old)


@pytest.mark.parametrize("window,first", [([[3.0, 3.0], [3.0, 3.0]], 0), ([[0.0, 1.0], [1.0, 0.0]], 1),
                                          ([[0.0, 0.0], [2.0, 2.0]], 2), ([[0.0, 0.0], [0.0, 2.0]], 3)])
def test_maxpool_tie_goes_to_the_first_maximum(window, first):
    v = torch.tensor(window, dtype=torch.float64).reshape(1, 1, 2, 2).requires_grad_(True)
    F.max_pool2d(v, 2, 2).sum().backward()
    assert int(v.grad.reshape(-1).argmax()) == first and v.grad.sum().item() == 1.0
    _, arg = R.maxpool_fwd(v.detach().reshape(1, 2, 2, 1), "none")
    assert int(arg) == first


# ---- softmax-crop, activations -------------------------------------------------------------------------------------------------
def test_softmax_crop_reference_equals_torch():
    g = torch.Generator().manual_seed(13)
    logits = torch.randn(3, 9, 14, generator=g, dtype=torch.float64) * 3
    logits[:, 4, 6] = torch.tensor([-80.0, 80.0, 0.0])
    want = F.softmax(logits[None], dim=1)[0, :, 3:, 5:].permute(1, 2, 0)
    got = R.softmax_crop_hwc(logits, 3, 5)
    assert got.shape == (6, 9, 3)
    _close(got, want, rel=1e-15)


def test_activation_references_equal_torch():
    g = torch.Generator().manual_seed(17)
    z = torch.cat([torch.randn(4000, generator=g, dtype=torch.float64) * 3,
                   torch.tensor([0.0, 2.0 ** -20, -2.0 ** -20, 20.0, -20.0, 20 + 2.0 ** -4, 20 - 2.0 ** -4, 60.0, -60.0, -100.0],
                                dtype=torch.float64)])
    want = {"none": z, "relu": F.relu(z), "leakyrelu": F.leaky_relu(z, 0.01), "elu": F.elu(z, 1.0),
            "mish": z * torch.tanh(F.softplus(z))}
    for i, name in enumerate(R.ACTS):
        _close(R.activation(z, name), want[name], rel=1e-15, what=name)
        assert torch.equal(R.activation(z, i), R.activation(z, name))
    _close(R.activation(z, "mish"), F.mish(z), rel=1e-15, what="F.mish")


# ---- fp32 -> bf16 ------------------------------------------------------------------------------------------------------------------
def _bits(v):
    return np.array(v, dtype=np.uint32).view(np.float32)


def test_bf16_rne_reference_equals_torch():
    assert R.bf16_rne_bits(_bits([0x3f808000, 0x3f818000, 0x3f808001, 0x7f7fffff, 0xff7fffff, 0x80000000])).tolist() == \
        [0x3f80, 0x3f82, 0x3f81, 0x7f80, 0xff80, 0x8000]
    rng = np.random.Generator(np.random.PCG64(19))
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)                  # every exponent, subnormals too
    u = np.concatenate([u, (u & 0xffff0000) | 0x8000, (u & 0xffff0000) | 0x7fff, (u & 0xffff0000) | 0x8001])
    x = u.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_rne_bits(x)
    fin = ~np.isnan(x)
    assert np.array_equal(got[fin], want[fin])
    assert np.isnan(R.bf16_bits_to_f64(got[~fin])).all()
    # the one-step rounding of an fp64 value agrees wherever the value is an fp32 number
    assert np.array_equal(R.bf16_round(x[fin].astype(np.float64)), want[fin])
    # ... and does not round twice: 1 + 2^-8 + 2^-30 lies above the tie, its fp32 rounding sits on it
    assert R.bf16_round(np.array([1 + 2.0 ** -8 + 2.0 ** -30])).tolist() == [0x3f81]


# ---- repack ------------------------------------------------------------------------------------------------------------------------
def test_pack_reference_is_the_transposed_zero_padded_weight():
    g = torch.Generator().manual_seed(23)
    w = torch.randn(5, 7, 3, 3, generator=g)                     # conv weight [co][ci][3][3]
    co, ci = 5, 7
    fwd = R.pack_weight(w.numpy(), 9, co, 8, ci, 12, 1, ci * 9, 9).reshape(9, 8, 12)
    assert np.array_equal(fwd[:, :co, :ci], w.reshape(co, ci, 9).permute(2, 0, 1).numpy())
    dg = R.pack_weight(w.numpy(), 9, ci, 8, co, 12, 1, 9, ci * 9).reshape(9, 8, 12)
    assert np.array_equal(dg[:, :ci, :co], w.reshape(co, ci, 9).permute(2, 1, 0).numpy())
    for p, r, c in ((fwd, co, ci), (dg, ci, co)):
        pad = p.copy()
        pad[:, :r, :c] = 0
        assert not pad.any() and not np.signbit(pad).any()
