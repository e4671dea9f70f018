"""GPU (MI355X): batched inference of stacks of small frames (InferWorker.frame_batch) — the group normalisation, the
batched distance post-processing (N frames in one chain of launches), the network forward at batch n and infer_stack end to
end.  Everything the batched path returns is compared with the frame-by-frame path and with the CPU oracles."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THS = ((0.10, 0.45), (0.02, 0.30))      # (th_cell, th_seed)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- normalisation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_group_normalisation_equals_host_formula_and_single_frame_kernels(dev, dtype):
    """5 frames of 100 x 130 (needs padding) with different ranges, one of them a single step wide: every value of the
    group call bit-equals 2 * (f32(x) - min) / (max - min) - 1 with the frame's own extrema and the one-frame kernels."""
    from microbeseg_amd import engine
    from microbeseg_amd.utils.utils import zero_pad_model_input
    rng = np.random.Generator(np.random.PCG64(11))
    top = 255 if dtype == np.uint8 else 65535
    ranges = [(0, top), (7, top // 3), (top // 2, top // 2 + 1), (top - 40, top), (3, 50)]
    frames = np.stack([rng.integers(lo, hi + 1, size=(100, 130)).astype(dtype) for lo, hi in ranges])
    assert int(frames[2].max()) - int(frames[2].min()) == 1
    store = torch.from_numpy(frames.view(np.int16) if dtype == np.uint16 else frames).to(dev)
    want, pads = [], None
    for f in frames:
        fmin, fmax = np.min(f), np.max(f)
        padded, pads = zero_pad_model_input(np.copy(f), pad_val=fmin)
        want.append((2 * (padded.astype(np.float32) - fmin) / (fmax - fmin) - 1).astype(np.float32))
    assert pads[0] > 0 and pads[1] > 0
    got = engine.normalize_frames(store, pads[0], pads[1])
    assert got.shape == (5, 1) + want[0].shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    for i in range(5):
        assert np.array_equal(got[i, 0].view(np.uint32), want[i].view(np.uint32)), f"frame {i}: host formula"
        single = engine.RawFrame(store[i], pads[0], pads[1]).normalized().cpu().numpy()[0, 0]
        assert np.array_equal(got[i, 0].view(np.uint32), single.view(np.uint32)), f"frame {i}: one-frame kernels"


# ---- post-processing -----------------------------------------------------------------------------------------------------
H_PP, W_PP = 160, 200
CELLS = [0, 3, 10, 25, 40, 60, 80, 100, 120, 150, 30, 60, 90, 45]     # frame 0: empty mask; 10..12 quantised; 13: no seed


def _group_maps():
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(2718))
    cells, borders = [], []
    for t, n in enumerate(CELLS):
        if n == 0:
            cell, border = np.zeros((H_PP, W_PP), np.float32), np.zeros((H_PP, W_PP), np.float32)
        else:
            cell, border = synth.synth_prediction_maps(rng, H_PP, W_PP, n, rmin=4.0, rmax=9.0)
        if t in (10, 11, 12):                       # maps in 1/16 steps: equal values inside components -> ties
            cell = (np.round(cell * 16) / 16).astype(np.float32)
        if t == 13:                                 # a mask, but nothing above either seed threshold
            cell = (np.clip(cell, 0, 1) * 0.25).astype(np.float32)
            border = np.zeros_like(border)
        cells.append(cell)
        borders.append(border)
    return np.stack(cells), np.stack(borders)


@pytest.fixture(scope="module")
def group(dev):
    """maps, and per (col_major, thresholds) the oracle labels and what the one-frame entry point returns"""
    from microbeseg_amd.inference import postprocessing as pp
    from oracle import postproc_ref as R
    cells, borders = _group_maps()
    c, b = torch.from_numpy(cells).to(dev), torch.from_numpy(borders).to(dev)
    want = {}
    for col_major in (True, False):
        for th_cell, th_seed in THS:
            oracle, single = [], []
            for i in range(len(CELLS)):
                if col_major:
                    oracle.append(R.distance_postprocessing(borders[i][..., None], cells[i][..., None], th_seed, th_cell))
                else:
                    oracle.append(R.distance_postprocessing(borders[i], cells[i], th_seed, th_cell))
                lab, n, s = pp.distance_postprocessing_device(b[i], c[i], th_seed, th_cell, col_major_ids=col_major)
                single.append((lab.cpu().numpy().view(np.uint16).copy(), int(n), int(s)))
            want[(col_major, th_cell, th_seed)] = (oracle, single)
    return c, b, want


def _check_group(pp, border, cell, want, pads=(0, 0)):
    for (col_major, th_cell, th_seed), (oracle, single) in want.items():
        labels, n_inst, status = pp.distance_postprocessing_batch_device(border, cell, th_seed, th_cell, pads=pads,
                                                                         col_major_ids=col_major)
        assert labels.shape == (len(CELLS), H_PP, W_PP) and labels.dtype == torch.int16
        got = labels.cpu().numpy().view(np.uint16)
        n_inst, status = n_inst.cpu().numpy(), status.cpu().numpy()
        print("col_major", col_major, "ths", (th_cell, th_seed), "instances", n_inst.tolist(), "status", status.tolist())
        for i in range(len(CELLS)):
            where = f"frame {i}, col_major {col_major}, ths {(th_cell, th_seed)}"
            assert np.array_equal(got[i], single[i][0]), f"{where}: {(got[i] != single[i][0]).sum()} px differ from the one-frame call"
            assert (int(n_inst[i]), int(status[i])) == single[i][1:], where
            assert np.array_equal(got[i], oracle[i]), f"{where}: {(got[i] != oracle[i]).sum()} px differ from the oracle"
        assert any(int(s) & 1 for s in status), "no frame took the exact serial redo"
        assert any(not int(s) & 1 for s in status), "no frame stayed on the per-component flood"
        assert not got[0].any() and int(n_inst[0]) == 0                 # the empty frame
        assert not got[13].any() and int(n_inst[13]) == 0               # a mask without a surviving seed
        assert int(n_inst.max()) >= 20


def test_postproc_group_equals_single_frames_and_oracle(group):
    from microbeseg_amd.inference import postprocessing as pp
    c, b, want = group
    _check_group(pp, b, c, want)
    _check_group(pp, b, c, want)                    # again on the same workspace


def test_postproc_group_of_one_equals_single_frame_and_oracle(group):
    """the group entry with N = 1 and the one-frame entry run the same kernels over two slab layouts (with and without
    the separator row, counters behind the workspace or inside it): same labels, instance count and status"""
    from microbeseg_amd.inference import postprocessing as pp
    c, b, want = group
    for (col_major, th_cell, th_seed), (oracle, single) in want.items():
        for i in range(len(CELLS)):
            labels, n_inst, status = pp.distance_postprocessing_batch_device(b[i:i + 1], c[i:i + 1], th_seed, th_cell,
                                                                             col_major_ids=col_major)
            assert labels.shape == (1, H_PP, W_PP) and n_inst.numel() == 1 and status.numel() == 1
            got = labels[0].cpu().numpy().view(np.uint16)
            where = f"frame {i}, col_major {col_major}, ths {(th_cell, th_seed)}"
            assert np.array_equal(got, single[i][0]), f"{where}: {(got != single[i][0]).sum()} px differ from the one-frame call"
            assert np.array_equal(got, oracle[i]), f"{where}: {(got != oracle[i]).sum()} px differ from the oracle"
            assert (int(n_inst[0]), int(status[0])) == single[i][1:], where


@pytest.mark.parametrize("rows,tile_s,tile_l", [(1, -1, -1), (16, 0, 0), (2, 400, 2000)])
def test_postproc_group_spill_and_global_probe_paths(group, rows, tile_s, tile_l):
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import postprocessing as pp
    c, b, want = group
    lib = _lib.load()
    assert lib.mseg_postproc_tuning(rows, tile_s, tile_l) == 0
    try:
        _check_group(pp, b, c, want)
    finally:
        assert lib.mseg_postproc_tuning(-1, -1, -1) == 0


def test_postproc_group_reads_padded_predictions_in_place(group):
    """the un-padded crop is read through the strides from (N, 1, Hp, Wp) network outputs; what lies in the padding must
    not matter"""
    from microbeseg_amd.inference import postprocessing as pp
    c, b, want = group
    pt, pl = 32, 56
    n = len(CELLS)
    cp = torch.full((n, 1, H_PP + pt, W_PP + pl), 5.0, device=c.device)
    bp = torch.full((n, 1, H_PP + pt, W_PP + pl), -3.0, device=c.device)
    cp[:, 0, pt:, pl:] = c
    bp[:, 0, pt:, pl:] = b
    _check_group(pp, bp[:, 0], cp[:, 0], want, pads=(pt, pl))


# ---- network ---------------------------------------------------------------------------------------------------------------
def _worker(tmp_path, unet_type, norm, seed=5):
    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.utils.unets import build_unet
    torch.manual_seed(seed)
    label_type = "distance" if unet_type == "DU" else "boundary"
    net = build_unet(unet_type, "relu", "conv", norm, torch.device("cuda:0"), 1, ch_out=1 if unet_type == "DU" else 3,
                     filters=(8, 16))
    if norm == "bn":                                # running statistics away from their initial values
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.uniform_(-0.2, 0.2)
                    m.running_var.uniform_(0.5, 1.5)
    base = tmp_path / f"{label_type}_model_00"
    torch.save(net.state_dict(), str(base) + ".pth")
    with open(str(base) + ".json", "w") as f:
        json.dump({"architecture": [unet_type, "conv", "relu", norm, [8, 16]], "label_type": label_type}, f)
    return InferWorker(model=str(base), device="cuda:0", ths=(0.10, 0.45))


@pytest.mark.parametrize("unet_type,norm", [("DU", "bn"), ("DU", "gn"), ("U", "bn")])
def test_forward_frames_matches_the_oracle_per_sample(tmp_path, dev, unet_type, norm):
    from microbeseg_amd.utils.utils import zero_pad_model_input
    from oracle import unet_ref
    worker = _worker(tmp_path, unet_type, norm)
    rng = np.random.Generator(np.random.PCG64(31))
    frames = np.stack([rng.integers(100 * t, 3000 + 8000 * t, size=(100, 130)).astype(np.uint16) for t in range(7)])
    pred = worker.forward_frames(frames)
    outs = pred if isinstance(pred, tuple) else (pred,)
    xs = []
    for f in frames:
        fmin, fmax = np.min(f), np.max(f)
        padded, _ = zero_pad_model_input(np.copy(f), pad_val=fmin)
        xs.append(2 * (padded.astype(np.float32) - fmin) / (fmax - fmin) - 1)
    x = torch.from_numpy(np.stack(xs)[:, None].astype(np.float32))
    sd = {k: v.detach().cpu() for k, v in worker.net.state_dict().items()}
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, x, unet_type, "relu", norm, (8, 16), training=False)
    ref = ref if isinstance(ref, tuple) else (ref,)
    assert len(outs) == len(ref)
    for o, r in zip(outs, ref):
        assert tuple(o.shape) == tuple(r.shape) and o.shape[0] == 7
        o = o.cpu()
        for i in range(7):
            err = (o[i] - r[i]).abs().max().item()
            bound = 1e-4 * max(1.0, r[i].abs().max().item())
            print(f"{unet_type}/{norm} sample {i}: max abs err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (i, err, bound)


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _count_net_calls(worker):
    calls = []
    worker.net.register_forward_pre_hook(lambda m, inp: calls.append(int(getattr(inp[0], "shape", (1,))[0])))
    return calls


def _distance_hook(T, H, W, dev, seed=99):
    """per-frame synthetic maps (some of them quantised), handed out in call order; pads the maps like the prediction"""
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    maps = []
    for t in range(T):
        cell, border = synth.synth_prediction_maps(rng, H, W, 5 + 4 * t, rmin=4.0, rmax=9.0)
        if t % 5 == 3:
            cell = (np.round(cell * 16) / 16).astype(np.float32)
        maps.append((torch.from_numpy(border).to(dev), torch.from_numpy(cell).to(dev)))
    calls = []

    def hook(pred):
        border, cell = pred
        assert border.shape[:2] == (1, 1) and cell.shape == border.shape
        t = len(calls)
        calls.append(t)
        ph, pw = border.shape[2] - H, border.shape[3] - W
        b, c = maps[t]
        pad = torch.nn.functional.pad
        return pad(b, (pw, 0, ph, 0))[None, None], pad(c, (pw, 0, ph, 0))[None, None]
    return hook, calls


def test_stack_in_groups_distance_model(tmp_path, dev):
    worker = _worker(tmp_path, "DU", "bn")
    T, H, W = 21, 128, 128
    rng = np.random.Generator(np.random.PCG64(8))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    net_calls = _count_net_calls(worker)
    hook, calls = _distance_hook(T, H, W, dev)
    worker.prediction_hook = hook
    want = worker.infer_stack(stack)                        # frame_batch = 1
    assert len(net_calls) == T and len(calls) == T
    assert int(want.max()) > 20
    del net_calls[:], calls[:]
    worker.frame_batch = 8
    got = worker.infer_stack(stack)
    assert net_calls == [8, 8, 5], net_calls
    assert calls == list(range(T))
    assert got.dtype == np.uint16 and got.shape == want.shape
    for t in range(T):
        assert np.array_equal(got[t], want[t]), f"frame {t}: {(got[t] != want[t]).sum()} px differ"
    # float stacks are normalised on the host and batched alike
    del net_calls[:], calls[:]
    got_f = worker.infer_stack(stack.astype(np.float32))
    assert net_calls == [8, 8, 5] and np.array_equal(got_f, want)


def test_stack_in_groups_survives_out_of_memory(tmp_path, dev):
    """a group's forward that does not fit is halved down to what fits, later groups start at that size, and the masks
    stay those of the frame-by-frame run; a frame that does not fit alone gets the zero mask"""
    worker = _worker(tmp_path, "DU", "bn")
    T, H, W = 10, 128, 128
    rng = np.random.Generator(np.random.PCG64(14))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    hook, calls = _distance_hook(T, H, W, dev, seed=7)
    worker.prediction_hook = hook
    want = worker.infer_stack(stack)
    assert int(want.max()) > 5
    forward, asked, limit = worker.net.forward, [], [3]

    def short_of_memory(x):
        asked.append(int(x.shape[0]))
        if x.shape[0] > limit[0]:
            raise RuntimeError("HIP out of memory. Tried to allocate 1.00 GiB")
        return forward(x)
    worker.net.forward = short_of_memory
    worker.frame_batch = 8
    del calls[:]
    got = worker.infer_stack(stack)
    assert asked == [8, 4, 2, 2, 2, 2, 2], asked
    assert calls == list(range(T)) and np.array_equal(got, want)
    limit[0] = 0
    del calls[:], asked[:]
    got = worker.infer_stack(stack[:3])
    assert asked == [3, 1, 1, 1] and not calls and not got.any()


def test_stack_in_groups_boundary_model(tmp_path, dev):
    from microbeseg_amd.utils import synth
    worker = _worker(tmp_path, "U", "bn")
    T, H, W = 21, 128, 128
    rng = np.random.Generator(np.random.PCG64(9))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    logits = []
    for t in range(T):
        cell, border = synth.synth_prediction_maps(rng, H, W, 4 + 2 * t, rmin=4.0, rmax=9.0)
        p1 = np.clip(cell * 2.0, 0, 1) * (1 - np.clip(border * 1.2, 0, 1))
        p2 = np.clip(border * 1.2, 0, 1) * (cell > 0.02)
        p0 = np.clip(1 - p1 - p2, 0.0, 1)
        probs = np.stack([p0, p1, p2], 0).astype(np.float32)
        probs = probs / probs.sum(0, keepdims=True)
        logits.append(torch.from_numpy(np.log(probs + 1e-6)[None]).to(dev))
    calls = []

    def hook(pred):
        assert pred.shape == (1, 3, H, W)
        calls.append(len(calls))
        return logits[calls[-1]]
    worker.prediction_hook = hook
    net_calls = _count_net_calls(worker)
    want = worker.infer_stack(stack)
    assert len(net_calls) == T and int(want.max()) > 5
    del net_calls[:], calls[:]
    worker.frame_batch = 8
    got = worker.infer_stack(stack)
    assert net_calls == [8, 8, 5] and calls == list(range(T))
    for t in range(T):
        assert np.array_equal(got[t], want[t]), f"frame {t}"


def test_stack_in_groups_without_hook_equals_oracle_of_own_predictions(tmp_path, dev):
    from oracle import postproc_ref
    from microbeseg_amd.utils import synth
    worker = _worker(tmp_path, "DU", "bn")
    T, H, W = 21, 128, 128
    rng = np.random.Generator(np.random.PCG64(10))
    frames = []
    for t in range(T):                                      # smooth frames: an untrained network maps blobs to blobs
        cell, _ = synth.synth_prediction_maps(rng, H, W, 6 + t, rmin=5.0, rmax=11.0)
        frames.append(np.clip(cell * 50000 + rng.normal(0, 800, cell.shape), 0, 65535).astype(np.uint16))
    stack = np.stack(frames)
    border, cell = worker.forward_frames(stack[:8])
    # an untrained network predicts no distance maps: thresholds from the distribution of its own output
    b = torch.tan(border[0, 0].clamp(0, 1) ** 2)
    b = torch.where(b < 0.05, torch.zeros_like(b), b).clamp(0, 1)
    worker.ths = [float(torch.quantile(cell[0, 0].flatten(), 0.85)), float(torch.quantile((cell[0, 0] - b).flatten(), 0.96))]
    worker.frame_batch = 8
    got = worker.infer_stack(stack)
    total = 0
    for g0 in range(0, T, 8):
        border, cell = worker.forward_frames(stack[g0:g0 + 8])
        for i in range(border.shape[0]):
            want = postproc_ref.distance_postprocessing(border[i, 0].cpu().numpy()[..., None],
                                                        cell[i, 0].cpu().numpy()[..., None], worker.ths[1], worker.ths[0])
            assert np.array_equal(got[g0 + i], want), f"frame {g0 + i}: {(got[g0 + i] != want).sum()} px differ"
            total += int(want.max())
    print("instances in the stack:", total, "thresholds (cell, seed):", worker.ths)
    assert total > 0


def test_padded_stack_matches_inference_frame_by_frame(tmp_path, dev):
    worker = _worker(tmp_path, "DU", "bn")
    T, H, W = 5, 100, 130
    rng = np.random.Generator(np.random.PCG64(12))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    hook, calls = _distance_hook(T, H, W, dev, seed=5)
    worker.prediction_hook = hook
    worker.frame_batch = 0                                  # auto
    got = worker.infer_stack(stack)
    assert calls == list(range(T))
    del calls[:]
    forward = worker._forward                               # inference() has no hook of its own: inject the same maps
    worker._forward = lambda x: hook(forward(x))
    for t in range(T):
        f = stack[t]
        padded, pads = worker.pad_frame(np.copy(f), np.min(f))
        assert pads[0] > 0 and pads[1] > 0
        one = worker.inference(padded, np.min(f), np.max(f), pads)
        assert one.shape == (H, W) and np.array_equal(got[t], one), f"frame {t}"
    assert int(got.max()) > 3


def test_frame_batch_1_never_reaches_the_group_entry_points(tmp_path, dev, monkeypatch):
    from microbeseg_amd import engine
    from microbeseg_amd.inference import postprocessing as pp
    worker = _worker(tmp_path, "DU", "bn")
    reached = []
    monkeypatch.setattr(pp, "distance_postprocessing_batch_device", lambda *a, **k: reached.append("pp"))
    monkeypatch.setattr(engine, "normalize_frames", lambda *a, **k: reached.append("norm"))
    monkeypatch.setattr(type(worker), "_infer_stack_batched", lambda *a, **k: reached.append("stack"))
    rng = np.random.Generator(np.random.PCG64(13))
    stack = rng.integers(0, 60000, size=(3, 128, 128)).astype(np.uint16)
    assert worker.frame_batch == 1
    worker.infer_stack(stack)
    assert not reached
    # sliding-window inference ignores the setting and says so
    said = []
    worker.text_output.connect(said.append)
    worker.sliding_window, worker.frame_batch = True, 8
    worker.infer_stack(stack)
    assert not reached and any("frame_batch" in s for s in said)
