"""GPU (MI355X): what the four stack routes of InferWorker.infer_stack — frame by frame (pipelined), frame_batch, tta,
scale — have in common whichever route a stack takes: the progress values, stop_inference, and float stacks with
apply_clahe.  Seeded small networks; what a route computes is tested in its own file."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# frame_batch = 2 on the three group routes: a stack of 3 frames goes through as a group of 2 and a group of 1
ROUTES = {"pipelined": {}, "frame_batch": {"frame_batch": 2}, "tta": {"tta": 2, "frame_batch": 2},
          "scale": {"scale": 0.5, "frame_batch": 2}}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _worker(tmp_path, unet_type, route, seed=5):
    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.utils.unets import build_unet
    torch.manual_seed(seed)
    label_type = "distance" if unet_type == "DU" else "boundary"
    net = build_unet(unet_type, "relu", "conv", "bn", torch.device("cuda:0"), 1, ch_out=1 if unet_type == "DU" else 3,
                     filters=(8, 16))
    with torch.no_grad():                            # running statistics away from their initial values
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    base = tmp_path / f"{label_type}_model_00"
    torch.save(net.state_dict(), str(base) + ".pth")
    with open(str(base) + ".json", "w") as f:
        json.dump({"architecture": [unet_type, "conv", "relu", "bn", [8, 16]], "label_type": label_type}, f)
    worker = InferWorker(model=str(base), device="cuda:0", ths=(0.10, 0.45))
    for attr, value in ROUTES[route].items():
        setattr(worker, attr, value)
    return worker


def _count_net_calls(worker):
    calls = []
    worker.net.register_forward_pre_hook(lambda m, inp: calls.append(int(getattr(inp[0], "shape", (1,))[0])))
    return calls


@pytest.mark.parametrize("unet_type", ["DU", "U"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_progress_and_stop(tmp_path, dev, route, unet_type):
    """T = 3: frame by frame on the pipelined route, a group of 2 and a ragged group of 1 on the others (the forwards
    asked of the network show it).  Every frame reports once, in frame order; a worker that was stopped before the call
    returns empty masks and leaves the network alone"""
    worker = _worker(tmp_path, unet_type, route)
    T, H, W = 3, 96, 80
    rng = np.random.Generator(np.random.PCG64(21))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    emitted = []
    worker.progress.connect(emitted.append)
    net_calls = _count_net_calls(worker)
    got = worker.infer_stack(stack)
    assert got.shape == (T, H, W) and got.dtype == np.uint16
    per_frame = {"pipelined": 1, "frame_batch": 1, "tta": 2, "scale": 1}[route]      # samples per frame in a forward
    assert net_calls == ([1] * T if route == "pipelined" else [2 * per_frame, per_frame]), net_calls
    assert emitted == [int(100 * (f + 1) / T) for f in range(T)], emitted
    del net_calls[:]
    worker.stop_inference = True
    got = worker.infer_stack(stack)
    assert got.shape == (T, H, W) and got.dtype == np.uint16 and not got.any()
    assert not net_calls, net_calls


def _smooth_stack(T, H, W, seed):
    """smooth frames: an untrained network maps blobs to blobs"""
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = []
    for t in range(T):
        cell, _ = synth.synth_prediction_maps(rng, H, W, 6 + t, rmin=5.0, rmax=11.0)
        frames.append(np.clip(cell * 50000 + rng.normal(0, 800, cell.shape), 0, 65535).astype(np.float32))
    return np.stack(frames)


@pytest.mark.parametrize("route", ["tta", "scale"])
def test_float_stacks_skip_clahe_with_one_message(tmp_path, dev, route):
    """a float stack has no fixed grey-level range: with apply_clahe it is segmented as it is, and infer_stack says so once
    per call, however many groups the stack has"""
    worker = _worker(tmp_path, "DU", route)
    T, H, W = 3, 100, 120
    stack = _smooth_stack(T, H, W, seed=10)
    predict = worker.predict_merged if route == "tta" else worker.predict_scaled
    border, cell = predict(stack[:1])
    # an untrained network predicts no distance maps: thresholds from the distribution of its own output
    b = torch.tan(border[0].clamp(0, 1) ** 2)
    b = torch.where(b < 0.05, torch.zeros_like(b), b).clamp(0, 1)
    worker.ths = [float(torch.quantile(cell[0].flatten(), 0.85)), float(torch.quantile((cell[0] - b).flatten(), 0.96))]
    said = []
    worker.text_output.connect(said.append)
    want = worker.infer_stack(stack)
    assert not said and want.any()
    worker.apply_clahe = True
    for call in (1, 2):
        del said[:]
        got = worker.infer_stack(stack)
        assert len(said) == 1 and "Skip CLAHE" in said[0] and "float32" in said[0], (call, said)
        assert np.array_equal(got, want)
