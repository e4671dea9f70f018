"""GPU (MI355X): the full HIP U-Net / DU-Net (forward, fused losses, explicit backward, optimizer steps) against
  (a) golden vectors produced by the real reference modules (tests/golden/unet_*.npz, traj_*.npz), and
  (b) the CPU oracle (oracle/unet_ref.py) on larger seeded inputs.
Tolerance 1e-4 relative (BASELINE.json north_star)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from helpers import VARIANTS, NodeTrace, bf16_rule as _bf16_rule, grad_floor, load_npz, rel_err, state_from, variant

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _build(name, dev, sd):
    from microbeseg_amd.utils.unets import build_unet
    ut, act, norm, filters, ch_out, label_type, pool = variant(name)
    net = build_unet(ut, act, pool, norm, dev, 1, ch_out=ch_out, filters=filters)
    net.load_state_dict(sd)
    return net


def _loss(net, fx, label_type, dev, sfx=""):
    from microbeseg_amd.training.losses import get_loss
    x = torch.from_numpy(fx["x" + sfx[1:]] if sfx else fx["x"]).to(dev)
    l1 = torch.from_numpy(fx["label1" + sfx]).to(dev)
    if label_type == "distance":
        crit = get_loss("smooth_l1", "distance")
        l2 = torch.from_numpy(fx["label2" + sfx]).to(dev)
        border, cell = net(x)
        return crit["border"](border, l1) + crit["cell"](cell, l2), (border, cell)
    crit = get_loss("ce_dice", "boundary")
    out = net(x)
    return crit(out, l1), (out,)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_net_matches_reference_fixture(name, dev):
    label_type = variant(name)[5]
    fx = load_npz(f"unet_{name}.npz")
    net = _build(name, dev, state_from(fx))
    net.eval()
    with torch.no_grad():
        _, outs = _loss(net, fx, label_type, dev)
    for i, o in enumerate(outs):
        assert rel_err(o.cpu(), fx[f"eval_out{i}"]) < TOL, f"eval_out{i}"
    net.train()
    loss, outs = _loss(net, fx, label_type, dev)
    for i, o in enumerate(outs):
        assert rel_err(o.detach().cpu(), fx[f"train_out{i}"]) < TOL, f"train_out{i}"
    assert abs(loss.item() - float(fx["loss"])) < TOL * max(1.0, abs(float(fx["loss"])))
    loss.backward()
    floor = grad_floor(fx)
    params = dict(net.named_parameters())
    # Parameter gradients: 1e-4 against the fp64 evaluation of the same network where fp32 arithmetic itself gets that
    # close — per tensor max(1e-4, 4 e_ref), e_ref = the REFERENCE's own (torch CPU fp32, the fixture) distance from fp64 —
    # and never further than 5e-4 from the reference's values.  "Relative" = max |difference| / max |reference| over the
    # tensor (helpers.rel_err: a max-norm bound, not per element).
    g64 = _oracle_grads(fx, name, torch.float64)
    table = []
    for k, v in fx.items():
        if k.startswith("g/"):
            pk = k[2:]
            assert params[pk].grad is not None, k
            e_ref = rel_err(v, g64[pk], floor)
            e_hip = rel_err(params[pk].grad.cpu(), g64[pk], floor)
            table.append((e_hip / max(TOL, 4 * e_ref), pk, e_hip, e_ref))
            assert e_hip < max(TOL, 4 * e_ref), (k, e_hip, e_ref)
            assert rel_err(params[pk].grad.cpu(), v, floor) < 5 * TOL, k
    print("gradient error vs fp64 (ratio to bound, tensor, HIP, reference fp32):")
    for row in sorted(table, reverse=True)[:5]:
        print("   %.2f  %-40s %.2e  %.2e" % row)
    sd = net.state_dict()
    for k, v in fx.items():
        if k.startswith("after/"):
            assert np.allclose(sd[k[6:]].cpu().numpy(), v, rtol=1e-4, atol=1e-6), k


def _oracle_grads(fx, name, dtype):
    """parameter gradients of the fixture's training step through oracle/unet_ref.py on the CPU in `dtype`"""
    from oracle import unet_ref
    ut, act, norm, filters, ch_out, label_type, pool = variant(name)
    params = {k: ((v.clone().to(dtype) if v.is_floating_point() else v.clone())) for k, v in state_from(fx).items()}
    for k, v in params.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    outs = unet_ref.unet_forward(params, torch.from_numpy(fx["x"]).to(dtype), ut, act, norm, filters, pool_method=pool,
                                 training=True, update_running_stats=True)
    l1 = torch.from_numpy(fx["label1"])
    if label_type == "distance":
        l2 = torch.from_numpy(fx["label2"])
        loss = unet_ref.regression_loss(outs[0], l1.to(dtype)) + unet_ref.regression_loss(outs[1], l2.to(dtype))
    else:
        loss = unet_ref.ce_dice(outs, l1)
    loss.backward()
    return {k: v.grad.detach() for k, v in params.items() if getattr(v, "grad", None) is not None}


def _oracle_traj(fx, name, make_ref_opt, steps, dtype):
    """the same trajectory through oracle/unet_ref.py on the CPU in `dtype` (fp32 = the reference arithmetic,
    fp64 = ground truth): per-step losses and the final state"""
    from oracle import unet_ref
    ut, act, norm, filters, ch_out, label_type, pool = variant(name)
    params = {k: ((v.clone().to(dtype) if v.is_floating_point() else v.clone())) for k, v in state_from(fx).items()}
    for k, v in params.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    opt = make_ref_opt([v for v in params.values() if v.requires_grad])
    losses = []
    for s in range(steps):
        opt.zero_grad()
        b = s % 2
        outs = unet_ref.unet_forward(params, torch.from_numpy(fx[f"x{b}"]).to(dtype), ut, act, norm, filters,
                                     training=True, update_running_stats=True)
        l1 = torch.from_numpy(fx[f"label1_{b}"])
        if label_type == "distance":
            l2 = torch.from_numpy(fx[f"label2_{b}"])
            loss = unet_ref.regression_loss(outs[0], l1.to(dtype)) + unet_ref.regression_loss(outs[1], l2.to(dtype))
        else:
            loss = unet_ref.ce_dice(outs, l1)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return np.array(losses), {k: v.detach() for k, v in params.items()}


def _traj(fxname, name, make_opt, make_ref_opt, steps, dev):
    """N optimisation steps on the HIP path from the fixture's initial weights and batches.

    Two yardsticks.  (1) The reference's own trajectory (fixture, torch CPU fp32): losses within 1e-3.  (2) Tight, per
    tensor: Adam / RAdam updates are sign-like (m / sqrt(v)), so a parameter whose gradient is rounding noise (e.g. a conv
    bias in front of BatchNorm: analytically zero) moves by +-lr per step in an arbitrary direction in ANY fp32
    implementation, while well-conditioned parameters follow the exact trajectory closely.  The fp64 oracle trajectory
    is the ground truth and the fp32 oracle's distance from it (e_ref, per tensor) is what fp32 arithmetic can achieve:
    the HIP path must stay within max(2e-4, 4 e_ref) of the fp64 trajectory, for every tensor and for the losses."""
    label_type = variant(name)[5]
    fx = load_npz(fxname)
    net = _build(name, dev, state_from(fx))
    net.train()
    opt = make_opt(net.parameters())
    losses = []
    for s in range(steps):
        opt.zero_grad()
        loss, _ = _loss(net, fx, label_type, dev, sfx=f"_{s % 2}")
        loss.backward()
        opt.step()
        losses.append(loss.item())
    losses = np.array(losses)
    assert np.allclose(losses, fx["losses"], rtol=1e-3, atol=1e-5), (losses, fx["losses"])
    l32, sd32 = _oracle_traj(fx, name, make_ref_opt, steps, torch.float32)
    l64, sd64 = _oracle_traj(fx, name, make_ref_opt, steps, torch.float64)
    e_l = np.abs(l32 - l64) / np.abs(l64)
    assert (np.abs(losses - l64) / np.abs(l64) <= np.maximum(2e-5, 4 * e_l.max())).all(), (losses, l64, e_l)
    sd = net.state_dict()
    report = []
    for k, v64 in sd64.items():
        if k.endswith("num_batches_tracked"):
            continue
        e_ref = rel_err(sd32[k], v64)
        e_hip = rel_err(sd[k].cpu(), v64)
        report.append((e_hip / max(2e-4, 4 * e_ref), k, e_hip, e_ref))
        assert e_hip <= max(2e-4, 4 * e_ref), (k, e_hip, e_ref)
        assert rel_err(sd[k].cpu(), fx["final/" + k]) < 2e-2, k      # and never far from the reference's own end point
    print("worst tensors (ratio, name, e_hip, e_ref):", sorted(report, reverse=True)[:3])


def _adam(ps):
    return torch.optim.Adam(ps, lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True)


def _fused_adam(ps):
    from microbeseg_amd.training.optim import FusedAdam
    return FusedAdam(ps, lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True)


@pytest.mark.parametrize("mk", [_adam, _fused_adam], ids=["torch_adam", "fused_adam"])
def test_adam_trajectory(mk, dev):
    _traj("traj_adam_DU_bn_relu.npz", "DU_bn_relu_8_16", mk, _adam, 8, dev)


def test_ranger_trajectory(dev):
    from microbeseg_amd.training.ranger2020 import Ranger
    from oracle import unet_ref

    def mk(ps):
        with contextlib.redirect_stdout(io.StringIO()):
            return Ranger(ps, lr=6e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-6,
                          weight_decay=0, use_gc=True, gc_conv_only=False, gc_loc=True)
    _traj("traj_ranger_DU_bn_mish.npz", "DU_bn_mish_8_16", mk,
          lambda ps: unet_ref.RangerRef(ps, lr=6e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-6),
          14, dev)


@pytest.mark.parametrize("mk", [_adam, _fused_adam], ids=["torch_adam", "fused_adam"])
def test_adam_ce_dice_trajectory(mk, dev):
    _traj("traj_adam_U_gn_relu.npz", "U_gn_relu_8_16", mk, _adam, 6, dev)


def test_fused_adam_equals_torch_adam(dev):
    """training/optim.FusedAdam (one launch over the flat arenas) against torch.optim.Adam(amsgrad=True) on the same
    parameters and gradients, 12 steps with a learning-rate change in between: same update to fp32 rounding (the kernel
    contracts multiply-adds), identical step counters and state layout."""
    from microbeseg_amd.training.optim import FusedAdam
    g = torch.Generator().manual_seed(21)
    shapes = [(64, 32, 3, 3), (64,), (7,), (33, 5, 2, 2), (1, 64, 1, 1), (1,)]
    init = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    pa = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    oa = torch.optim.Adam(pa, lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True)
    ob = FusedAdam(pb, lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True)
    for step in range(12):
        if step == 6:
            for o in (oa, ob):
                o.param_groups[0]["lr"] = 2e-4            # what ReduceLROnPlateau does
        grads = [torch.randn(s, generator=g) * (10.0 ** (step % 3 - 2)) for s in shapes]
        ob.zero_grad()
        for a, b, gr in zip(pa, pb, grads):
            a.grad = gr.clone().to(dev)
            b.grad.copy_(gr.to(dev))
        oa.step()
        ob.step()
        for a, b in zip(pa, pb):
            assert rel_err(b.detach().cpu(), a.detach().cpu()) < 2e-6
    for a, b in zip(pa, pb):
        sa, sb = oa.state[a], ob.state[b]
        assert int(sa["step"]) == sb["step"] == 12
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert rel_err(sb[key].cpu(), sa[key].cpu()) < 2e-6, key


def test_fused_adam_load_state_dict(dev):
    """FusedAdam.load_state_dict: a state dict of torch.optim.Adam — and its own — is taken over INTO the flat
    arenas (the state tensors stay views of them), and the kernel reads the learning rate of the param_groups that
    load_state_dict installed: after a resume, a scheduler's change of param_groups[0]['lr'] reaches the next step."""
    from microbeseg_amd.training.optim import FusedAdam
    g = torch.Generator().manual_seed(22)
    shapes = [(32, 16, 3, 3), (32,), (5,), (9, 4, 2, 2)]
    init = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    pa = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    oa = torch.optim.Adam(pa, lr=8e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True)
    ob = FusedAdam(pb, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True)     # another lr on purpose

    def both_step():
        grads = [torch.randn(s, generator=g) * 0.05 for s in shapes]
        ob.zero_grad()
        for a, b, gr in zip(pa, pb, grads):
            a.grad = gr.clone().to(dev)
            b.grad.copy_(gr.to(dev))
        oa.step()
        ob.step()

    for _ in range(3):                                   # torch's Adam runs ahead; FusedAdam follows with a wrong lr
        grads = [torch.randn(s, generator=g) * 0.05 for s in shapes]
        for a, gr in zip(pa, grads):
            a.grad = gr.clone().to(dev)
        oa.step()
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    arena_ptrs = [ob.state[b]["exp_avg"].data_ptr() for b in pb]
    ob.load_state_dict(oa.state_dict())                  # moments, step counters AND lr = 8e-4 come from torch's optimizer
    assert [ob.state[b]["exp_avg"].data_ptr() for b in pb] == arena_ptrs, "the moments must stay views of the arenas"
    assert ob.param_groups[0]["lr"] == 8e-4
    both_step()
    for a, b in zip(pa, pb):
        assert rel_err(b.detach().cpu(), a.detach().cpu()) < 2e-6
    for o in (oa, ob):
        o.param_groups[0]["lr"] = 1e-4                   # a scheduler edits the groups load_state_dict installed
    both_step()
    ob.load_state_dict(ob.state_dict())                  # its own round trip
    both_step()
    for a, b in zip(pa, pb):
        assert rel_err(b.detach().cpu(), a.detach().cpu()) < 2e-6
        assert int(oa.state[a]["step"]) == ob.state[b]["step"] == 6


def test_ranger_multi_tensor_step(dev):
    """Ranger.step() updates all CUDA tensors of a group with mseg_ranger_step_multi (48 tensors per launch): bit-identical
    to mseg_ranger_step called per tensor, and the optimizer follows its own torch path (CPU parameters) over 14 steps
    (past the rectification threshold and two lookahead blends), with one parameter skipping a step."""
    import ctypes as C
    from microbeseg_amd import _lib
    from microbeseg_amd.training.ranger2020 import Ranger
    lib = _lib.load()
    g = torch.Generator().manual_seed(33)
    shapes = [(16, 8, 3, 3), (16,), (5, 3, 2, 2), (9000,), (1, 4, 1, 1), (3,)] * 10 + [(256, 300)]     # 61 tensors
    # (a) the kernel against the per-tensor entry point
    mk = lambda: [torch.randn(s, generator=g).to(dev) for s in shapes]
    p0, gr, m0, v0, s0 = mk(), mk(), mk(), [t.abs() for t in mk()], mk()
    one = [[t.clone() for t in ts] for ts in (p0, m0, v0, s0)]
    many = [[t.clone() for t in ts] for ts in (p0, m0, v0, s0)]
    jobs = (_lib.MsegRangerJob * len(shapes))()
    stream = torch.cuda.current_stream().cuda_stream
    for i, shp in enumerate(shapes):
        rows = shp[0] if len(shp) > 1 else 0
        rect, look, lr = i % 2, (i // 2) % 2, 1e-3 * (1 + i % 3)
        _lib.check(lib.mseg_ranger_step(one[0][i].data_ptr(), gr[i].data_ptr(), one[1][i].data_ptr(),
                                        one[2][i].data_ptr(), one[3][i].data_ptr(), gr[i].numel(), max(rows, 1), 0.95,
                                        0.999, 1e-5, lr, rect, int(rows > 0), look, 0.5, stream), "ranger_step")
        j = jobs[i]
        j.p, j.g, j.m, j.v, j.slow = (many[0][i].data_ptr(), gr[i].data_ptr(), many[1][i].data_ptr(),
                                      many[2][i].data_ptr(), many[3][i].data_ptr())
        j.n, j.rows, j.step_lr, j.flags = gr[i].numel(), rows, lr, rect | (look << 1)
    _lib.check(lib.mseg_ranger_step_multi(C.addressof(jobs), len(shapes), 0.95, 0.999, 1e-5, 0.5, stream), "multi")
    for a, b in zip(one, many):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert lib.mseg_ranger_step_multi(C.addressof(jobs), 0, 0.95, 0.999, 1e-5, 0.5, stream) != 0
    # (b) the optimizer on the device against its torch path on the CPU
    init = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    pc = [torch.nn.Parameter(t.clone()) for t in init]
    pd = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    with contextlib.redirect_stdout(io.StringIO()):
        oc, od = (Ranger(ps, lr=6e-3, eps=1e-6) for ps in (pc, pd))
    for step in range(14):
        for i, (a, b, shp) in enumerate(zip(pc, pd, shapes)):
            if step == 3 and i == 1:
                a.grad = b.grad = None                 # this tensor's step counter falls behind the others
                continue
            t = torch.randn(shp, generator=g) * (10.0 ** (step % 3 - 2))
            a.grad, b.grad = t.clone(), t.clone().to(dev)
        oc.step()
        od.step()
    for a, b in zip(pc, pd):
        assert rel_err(b.detach().cpu(), a.detach()) < 5e-6
        assert oc.state[a]["step"] == od.state[b]["step"]
        for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            assert rel_err(od.state[b][key].cpu(), oc.state[a][key]) < 5e-6, key
    assert od.state[pd[1]]["step"] == 13


def _l2_rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("ut,act,norm,filters,size,batch", [
    ("DU", "mish", "bn", (16, 128), 64, 3),      # 4 levels, odd batch
    ("U", "mish", "gn", (32, 64), 96, 2),
    ("DU", "elu", "bn", (64, 128), 48, 2),       # 64-channel level 0 like the default net
    ("DU", "relu", "bn", (64, 128), 48, 2),      # ReLU: see the note on mask flips below
    ("U", "relu", "gn", (32, 128), 64, 2),
])
def test_net_matches_oracle_on_larger_inputs(ut, act, norm, filters, size, batch, dev):
    """Same seeded weights / inputs through the HIP net and the CPU oracle, forward + parameter gradients.

    ReLU note: with ~3e5 activations per layer a few pre-activations land within fp32 rounding of 0, where the HIP
    and CPU summation orders disagree on the sign; each such flip switches one element of dz on/off (verified with
    tools/diag_dz.py: gy and z agree to 1e-6, dz differs only at those elements), and with N(0,1) upstream gradients a
    single flip moves max|dW| by ~1e-2.  The flipped elements are identified (HIP mask != oracle mask), required to
    sit at |z| <= 1e-4 max|z| and to be few (helpers.check_relu_flips), and exactly their contribution is removed by
    replaying the oracle's backward with the HIP path's masks (oracle/unet_ref.py RELU_MASKS); everything else is held
    to the same element-wise rule as the smooth activations."""
    from helpers import NodeTrace, check_relu_flips
    from microbeseg_amd.utils.unets import build_unet
    from oracle import unet_ref
    torch.manual_seed(1234)
    ch_out = 3 if ut == "U" else 1
    net = build_unet(ut, act, "conv", norm, dev, 1, ch_out=ch_out, filters=filters)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = torch.rand(batch, 1, size, size) * 2 - 1
    net.train()
    with NodeTrace() as tr:
        outs = net(x.to(dev))
        outs = outs if isinstance(outs, tuple) else (outs,)
        gos = [torch.randn(o.shape) for o in outs]
        torch.autograd.backward(outs, [g.to(dev) for g in gos])
        masks = tr.relu_masks() if act == "relu" else None

    def oracle(dtype, trace=None):
        params = {k: (v.clone().to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k
                      else (v.clone().to(dtype) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
        unet_ref.RELU_MASKS = iter(masks) if masks is not None else None
        unet_ref.RELU_TRACE = trace
        try:
            ref = unet_ref.unet_forward(params, x.to(dtype), ut, act, norm, filters, training=True,
                                        update_running_stats=True)
            ref = ref if isinstance(ref, tuple) else (ref,)
            torch.autograd.backward(ref, [g.to(dtype) for g in gos])
        finally:
            unet_ref.RELU_MASKS = unet_ref.RELU_TRACE = None
        return params, ref

    trace = [] if act == "relu" else None
    p32, r32 = oracle(torch.float32, trace)     # the reference arithmetic (torch CPU fp32)
    p64, r64 = oracle(torch.float64)            # ground truth
    for o, r in zip(outs, r32):
        assert rel_err(o.detach().cpu(), r.detach()) < TOL
    if act == "relu":
        flips, total = check_relu_flips(masks, trace)
        print(f"ReLU decisions flipped: {flips} of {total}")
    # Parameter gradients of a deep BatchNorm net are ill-conditioned: torch-CPU fp32 itself is ~1e-3 away from the
    # fp64 truth.  The HIP path must be as accurate as the reference arithmetic: per parameter within 4x of the
    # fp32 oracle's own error, or no worse than the fp32 oracle's worst parameter, or within 5*TOL.
    floor = 1e-3 * max(p.grad.abs().max().item() for p in p64.values() if getattr(p, "grad", None) is not None)
    e_ref_all = {k: rel_err(p32[k].grad, p64[k].grad, floor) for k, _ in net.named_parameters()}
    worst_ref = max(e_ref_all.values())
    for k, p in net.named_parameters():
        e_hip = rel_err(p.grad.cpu(), p64[k].grad, floor)
        assert e_hip < max(5 * TOL, 4 * e_ref_all[k], worst_ref), (k, e_hip, e_ref_all[k], worst_ref)
    for k, v in net.state_dict().items():
        if "running" in k:
            assert rel_err(v.cpu(), p32[k]) < 1e-4, k


@pytest.mark.parametrize("ut,act,norm,filters,size,batch", [("DU", "elu", "bn", (64, 128), 64, 2),
                                                            ("U", "mish", "bn", (64, 128), 48, 3),
                                                            ("DU", "mish", "gn", (64, 128), 64, 2),     # per-sample tables
                                                            ("U", "elu", "in", (64, 128), 64, 2)])
def test_bf16_mode_matches_bf16_oracle(ut, act, norm, filters, size, batch, dev):
    """BASELINE configs[2] (bf16 forward / backward, fp32 accumulate and norm statistics): engine.set_precision('bf16')
    against the oracle with the SAME rounding points (oracle/unet_ref.py BF16_RULE: operands of the 3x3 stride-1
    convolutions rounded to bf16, everything else fp32).  bf16 has its own tolerance: an operand whose fp32 value differs in
    the last bits between the two implementations can round to a different bf16 neighbour (2^-8 relative), so the
    agreement is ~1e-3 on the outputs — a quarter of the distance between bf16 and fp32 arithmetic itself, which is also
    checked (the bf16 path must stay within 3e-2 of the fp32 reference arithmetic)."""
    from microbeseg_amd import engine
    from microbeseg_amd.utils.unets import build_unet
    from oracle import unet_ref
    torch.manual_seed(1234)
    ch_out = 3 if ut == "U" else 1
    net = build_unet(ut, act, "conv", norm, dev, 1, ch_out=ch_out, filters=filters)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = torch.rand(batch, 1, size, size) * 2 - 1
    net.train()
    engine.set_precision("bf16")
    try:
        with NodeTrace() as tr:
            outs = net(x.to(dev))
            outs = outs if isinstance(outs, tuple) else (outs,)
            gos = [torch.randn(o.shape) for o in outs]
            torch.autograd.backward(outs, [g.to(dev) for g in gos])
            stored_bf16 = tr.nodes[0].z.dtype == torch.bfloat16
    finally:
        engine.set_precision("fp32")
    # 64 px inputs: every launch has a bf16 kernel -> activations / gradients are STORED as bf16; the 48 px case falls back
    # to fp32 tensors (operand rounding only).  The oracle models whichever the engine chose.
    assert stored_bf16 == (size == 64)

    def oracle(rule):
        unet_ref.BF16_RULE = rule
        unet_ref.BF16_STORAGE = stored_bf16
        try:
            params = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone())
                      for k, v in sd.items()}
            ref = unet_ref.unet_forward(params, x, ut, act, norm, filters, training=True, update_running_stats=True)
            ref = ref if isinstance(ref, tuple) else (ref,)
            torch.autograd.backward(ref, gos)
        finally:
            unet_ref.BF16_RULE = None
            unet_ref.BF16_STORAGE = False
        return params, ref

    p16, r16 = oracle(_bf16_rule)
    p32, r32 = oracle(None)
    # Own tolerance of the bf16 mode, stated relative to what bf16 itself does to this network: d_ref = distance of the
    # bf16 oracle (same operand AND storage rounding points, incl. the bf16-stored mish / elu activation) from the fp32
    # oracle, relative L2.  The HIP path must be as close to fp32 as its model (<= 1.25 d_ref), clearly closer to the model
    # than the model is to fp32 (<= 0.75 d_ref; measured 0.44-0.58: operands whose last fp32 bits differ between the two
    # implementations round to the other bf16 neighbour), and really bf16 (>= 0.4 d_ref).
    for o, a, b in zip(outs, r16, r32):
        d_ref = _l2_rel(a.detach(), b.detach())
        d_model, d_fp32 = _l2_rel(o.detach().cpu(), a.detach()), _l2_rel(o.detach().cpu(), b.detach())
        print(f"output: d_ref {d_ref:.2e}, HIP vs bf16 oracle {d_model:.2e}, HIP vs fp32 {d_fp32:.2e}")
        assert 1e-4 < d_ref < 5e-2
        assert 0.4 * d_ref < d_fp32 < 1.25 * d_ref and d_model < 0.75 * d_ref
    floor = 1e-3 * max(p.grad.abs().max().item() for p in p32.values() if getattr(p, "grad", None) is not None)
    for k, p in net.named_parameters():
        if p32[k].grad.abs().max().item() <= floor:
            continue
        noise = _l2_rel(p16[k].grad, p32[k].grad)                          # what bf16 rounding itself does to this gradient
        assert _l2_rel(p.grad.cpu(), p32[k].grad) < max(3e-2, 1.5 * noise), k      # floor: a few bf16 roundings (2^-9 each)
        assert _l2_rel(p.grad.cpu(), p16[k].grad) < max(3e-2, 1.5 * noise), k


@pytest.mark.parametrize("batch,size", [(2, 48), (3, 48), (2, 64)])
@pytest.mark.parametrize("name,ut,norm,filters,ch_in,pool", [("DU_64_128", "DU", "bn", (64, 128), 1, "conv"),
                                                             ("DU_64_128_in3", "DU", "bn", (64, 128), 3, "conv"),
                                                             ("DU_64_128_max", "DU", "bn", (64, 128), 1, "max"),
                                                             ("U_8_16", "U", "gn", (8, 16), 1, "conv")])
def test_bf16_storage_decision_is_what_the_passes_do(name, ut, norm, filters, ch_in, pool, batch, size, dev):
    """engine.bf16_storage_ok against the passes it decides for, on shapes that straddle the decision (DU (64, 128): bf16
    tensors when training at 2 x 48 x 48, fp32 at 3 x 48 x 48; ch_in = 3: bf16 for eval only): every tensor of a training
    forward + backward and of an eval forward is stored as the decision says, the decision is the recorded one
    (tests/golden/bf16_storage_grid.json), and the passes complete — the dispatch answers MSEG_EINVAL for a bf16 tensor on a
    launch without a bf16 kernel — with finite outputs and parameter gradients."""
    from helpers import storage_grid
    from microbeseg_amd import engine
    from microbeseg_amd.utils.unets import build_unet
    table = storage_grid()[1]
    torch.manual_seed(7)
    net = build_unet(ut, "relu", pool, norm, dev, 1, ch_in=ch_in, ch_out=3 if ut == "U" else 1, filters=filters)
    x = (torch.rand(batch, ch_in, size, size) * 2 - 1).to(dev)
    with engine.precision_scope("bf16"):
        for training in (True, False):
            want = engine.bf16_storage_ok(net._spec, batch, ch_in, size, size, training)
            assert want == table[(name, batch, size, training)], (name, batch, size, training)
            net.train(training)
            with NodeTrace() as tr, torch.set_grad_enabled(training):
                outs = net(x)
                outs = outs if isinstance(outs, tuple) else (outs,)
                if training:
                    torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
            assert tr.nodes and all((n.z.dtype == torch.bfloat16) == want for n in tr.nodes), (training, want)
            assert all(torch.isfinite(o).all() for o in outs)
            if training:
                assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


@pytest.mark.parametrize("optimizer", ["fused_adam", "torch_capturable"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_train_step_equals_eager(precision, optimizer, dev, request):
    """hipGraph replay of the training step (training/graph_step.py): same losses and bit-identical weights as the eager
    step on the same batches (the kernels and their order are the same; only the launches are pre-recorded) — with the
    default optimizer (FusedAdam: step counter and learning rate on the device, a learning-rate change does not re-record)
    and with torch's capturable Adam (re-recorded).  An eval forward after the replays must see the trained weights (the
    packed GEMM operands are refreshed inside the recorded step)."""
    from microbeseg_amd import engine
    from microbeseg_amd.training.graph_step import GraphedTrainStep
    from microbeseg_amd.training.losses import get_loss
    from microbeseg_amd.training.optim import FusedAdam
    from microbeseg_amd.utils.unets import build_unet
    request.addfinalizer(lambda: engine.set_precision("fp32"))
    engine.set_precision(precision)
    crit = get_loss("smooth_l1", "distance")
    g = torch.Generator().manual_seed(4)
    batches = [(torch.rand(4, 1, 64, 64, generator=g) * 2 - 1, torch.rand(4, 1, 64, 64, generator=g),
                torch.rand(4, 1, 64, 64, generator=g)) for _ in range(7)]
    batches = [tuple(t.to(dev) for t in b) for b in batches]
    odd = tuple(t[:3].contiguous() for t in batches[0])        # a smaller batch in between: falls back to eager

    def run(graphed):
        torch.manual_seed(11)
        net = build_unet("DU", "relu", "conv", "bn", dev, 1, ch_out=1, filters=(64, 128))
        if optimizer == "fused_adam":
            opt = FusedAdam(net.parameters(), lr=8e-4, betas=(0.9, 0.999), eps=1e-8, amsgrad=True)
        else:
            opt = torch.optim.Adam(net.parameters(), lr=8e-4, betas=(0.9, 0.999), eps=1e-8, amsgrad=True,
                                   capturable=True)
        net.train()

        def step(x, lb, lc):
            opt.zero_grad(set_to_none=True)
            border, cell = net(x)
            loss = crit["border"](border, lb) + crit["cell"](cell, lc)
            loss.backward()
            opt.step()
            return loss
        fn = GraphedTrainStep(step, opt, warmup=2) if graphed else step
        losses = []
        for i, b in enumerate(batches):
            losses.append(float(fn(*b).detach()))
            if i == 4:
                losses.append(float(fn(*odd).detach()))
            if i == 5:                                      # a learning-rate step (ReduceLROnPlateau); the very next batch is
                recorded = fn.graph if graphed else None    # the short one: it must NOT become the recorded shape
                if graphed:
                    fn.set_lr(2e-4)
                    assert (fn.graph is recorded) == (optimizer == "fused_adam"), "FusedAdam keeps the recorded step"
                else:
                    for group in opt.param_groups:
                        group["lr"] = 2e-4
                losses.append(float(fn(*odd).detach()))
        if graphed:
            assert fn.graph is not None and fn.shapes[0][0][0] == 4, "the full batch must be the recorded shape again"
        if optimizer == "fused_adam":
            assert all(opt.state[p]["step"] == len(batches) + 2 for p in net.parameters())
        net.eval()
        with torch.no_grad():
            out = [t.detach().clone() for t in net(batches[0][0])]
        return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, out

    l_e, sd_e, out_e = run(False)
    l_g, sd_g, out_g = run(True)
    assert l_e == l_g
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    for a, b in zip(out_e, out_g):
        assert torch.equal(a, b), "eval forward after the replays"


def test_conv_epilogue_statistics_in_the_training_step(dev, request):
    """engine.set_conv_stats(True): BatchNorm statistics of the layers whose convolution kernel can take them in its epilogue
    (MsegIgemm.stats) instead of a pass over the stored tensor.  The same sums in another order: outputs, running
    statistics and gradients of a bf16 training step agree with the pass to a few fp32 roundings amplified through bf16
    storage (a value that moves by one fp32 ulp may round to the neighbouring bf16)."""
    from microbeseg_amd import engine
    from microbeseg_amd.utils.unets import build_unet
    request.addfinalizer(lambda: (engine.set_precision("fp32"), engine.set_conv_stats(False)))
    engine.set_precision("bf16")
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(16, 1, 128, 128, generator=g) * 2 - 1).to(dev)
    gb, gc = torch.randn(16, 1, 128, 128, generator=g).to(dev), torch.randn(16, 1, 128, 128, generator=g).to(dev)
    res = []
    for fused in (False, True):
        engine.set_conv_stats(fused)
        torch.manual_seed(12)
        net = build_unet("DU", "relu", "conv", "bn", dev, 1, ch_out=1, filters=(64, 128))
        net.train()
        taken = []
        orig = engine.norm_stats

        def spy(node, *a, conv_part=None, **k):
            taken.append(conv_part is not None)
            return orig(node, *a, conv_part=conv_part, **k)
        engine.norm_stats = spy
        try:
            border, cell = net(x)
            ((border * gb).sum() + (cell * gc).sum()).backward()
        finally:
            engine.norm_stats = orig
        assert any(taken) == fused, "the 128-channel layers of this network take the statistics in the epilogue"
        res.append(([border.detach().cpu(), cell.detach().cpu()],
                    {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if "running" in k},
                    {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}))
    for a, b in zip(res[0][0], res[1][0]):
        assert rel_err(b, a) < 2e-2
    for k in res[0][1]:
        assert rel_err(res[1][1][k], res[0][1][k]) < 1e-5, k
    biggest = max(v.double().norm().item() for v in res[0][2].values())
    for k in res[0][2]:
        if res[0][2][k].double().norm().item() < 1e-2 * biggest:
            continue        # e.g. a convolution bias in front of BatchNorm: analytically zero, rounding noise in both runs
        assert _l2_rel(res[1][2][k], res[0][2][k]) < 2e-2, k


def test_eval_tables_follow_training_and_loading(dev):
    """Eval-mode BatchNorm tables are cached per layer: a training step (which updates the running statistics inside a
    kernel), a state-dict load and an in-place edit of a buffer must each be seen by the next eval forward, and repeated eval
    forwards must reuse the tables."""
    from microbeseg_amd import engine
    from microbeseg_amd.utils.unets import build_unet
    from oracle import unet_ref
    torch.manual_seed(3)
    net = build_unet("DU", "relu", "conv", "bn", dev, 1, ch_out=1, filters=(8, 16))
    x = torch.rand(2, 1, 32, 32, device=dev) * 2 - 1

    def eval_out():
        net.eval()
        with torch.no_grad():
            return [t.clone() for t in net(x)]

    def oracle_out():
        sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        with torch.no_grad():
            return unet_ref.unet_forward(sd, x.cpu(), "DU", "relu", "bn", (8, 16), training=False)

    a = eval_out()
    epoch0 = engine._stats_epoch
    b = eval_out()
    assert engine._stats_epoch == epoch0 and all(torch.equal(u, v) for u, v in zip(a, b))
    net.train()
    net(x)[0].sum().backward()                               # running statistics move
    c = eval_out()
    assert not torch.equal(a[0], c[0])
    for got, want in zip(c, oracle_out()):
        assert (got.cpu() - want).abs().max() < 1e-4 * max(1.0, want.abs().max())
    with torch.no_grad():                                    # in-place edit through torch
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.mul_(1.5)
    d = eval_out()
    assert not torch.equal(c[0], d[0])
    for got, want in zip(d, oracle_out()):
        assert (got.cpu() - want).abs().max() < 1e-4 * max(1.0, want.abs().max())
