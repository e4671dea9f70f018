"""GPU (MI355X): inference at a chosen resolution (InferWorker.scale) — the two kernels of
csrc/resample.hip against the float64 restatement tests/resample_ref.py, their invariances, and the route: predict_scaled
against the same steps done by hand, the masks of infer_stack, the combinations and the defaults.

The bound 1e-5 of the kernel tests is derived, not measured: values lie in [-1, 1] and a result is two passes of at most
12 fp32 multiply-adds with weights rounded to fp32 (relative 2^-24 each).  Per pass the rounding of the weights
contributes at most 2^-24 * sum|w v| <= 6e-8 and the accumulation at most 12 * 2^-24 * sum|w v| <= 7.2e-7; two passes and
the second pass's amplification of the first (weights sum to 1) stay below 3e-6 < 1e-5."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import resample_ref

pytestmark = pytest.mark.gpu

EINVAL = -1
SHAPES = [(70, 131), (37, 53)]
FACTORS = [0.25, 0.73, 1.6, 4]
PADS = [(0, 0), (5, 11)]
BOUND = 1e-5
GUARD = 1024
SENTINEL = 0x5EAFD00D


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dev):
    """-> (whole buffer as int32, the fp32 view of `shape` in its middle): NaN inside, sentinel words around"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    view = buf[GUARD:GUARD + numel].view(torch.float32).view(*shape)
    view.fill_(float("nan"))
    return buf, view


def _guards_intact(buf):
    g = buf.cpu().numpy()
    return bool((g[:GUARD] == SENTINEL).all() and (g[-GUARD:] == SENTINEL).all())


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _frames(dtype, shape, seed):
    """3 frames with different content and different extrema"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if dtype == np.float32:
        return np.stack([rng.uniform(-1, 1, size=shape).astype(np.float32) * np.float32(s) for s in (1.0, 0.5, 0.03)])
    top = 255 if dtype == np.uint8 else 65535
    ranges = [(0, top), (7, top // 3), (top // 2, top // 2 + 1)]
    return np.stack([rng.integers(lo, hi + 1, size=shape).astype(dtype) for lo, hi in ranges])


def _upload(frames, dev):
    """-> (device tensor as resample.frames takes it, minmax or None)"""
    from microbeseg_amd import _lib, engine
    if frames.dtype == np.float32:
        return torch.from_numpy(frames).to(dev), None
    raw = torch.from_numpy(frames.view(np.int16) if frames.dtype == np.uint16 else frames).to(dev)
    minmax = torch.empty((len(frames), 2), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().mseg_frames_minmax(raw.data_ptr(), engine.RawFrame.PIX[raw.dtype], len(frames),
                                              frames.shape[1] * frames.shape[2], minmax.data_ptr(), _stream()), "minmax")
    return raw, minmax


def _frames_into(raw, minmax, ya, xa, pads, out, dtype=None):
    from microbeseg_amd import _lib
    pix = {torch.uint8: _lib.PIX_U8, torch.int16: _lib.PIX_U16, torch.float32: _lib.PIX_F32}[raw.dtype]
    return _lib.load().mseg_resample_frames(raw.data_ptr(), pix if dtype is None else dtype, raw.shape[0],
                                            None if minmax is None else minmax.data_ptr(), C.byref(ya), C.byref(xa),
                                            int(pads[0]), int(pads[1]), out.data_ptr(), _stream())


# ---- 1. frames -> network input ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_frames_equal_the_restatement(dev, dtype, shape):
    from microbeseg_amd.inference import resample as R
    H, W = shape
    frames = _frames(dtype, shape, seed=H * 100 + W)
    raw, minmax = _upload(frames, dev)
    worst = 0.0
    for s in FACTORS:
        hs, ws = R.out_size(H, s), R.out_size(W, s)
        ya, xa = R.axis(H, hs, dev), R.axis(W, ws, dev)
        for pads in PADS:
            want = resample_ref.network_input(frames, hs, ws, pads)
            buf, out = _guarded(want.shape, dev)
            assert _frames_into(raw, minmax, ya.desc, xa.desc, pads, out) == 0
            got = out.cpu().numpy()
            assert not np.isnan(got).any(), f"scale {s}, pads {pads}: {int(np.isnan(got).sum())} elements were not written"
            err = float(np.abs(got.astype(np.float64) - want).max())
            worst = max(worst, err)
            print(f"{np.dtype(dtype).name} {shape} x {s} pads {pads}: max |difference| {err:.3e}")
            assert err <= BOUND, f"scale {s}, pads {pads}: {err:.3e}"
            assert (got[:, :pads[0], :] == -1).all() and (got[:, :, :pads[1]] == -1).all()      # exactly -1
            assert _guards_intact(buf), f"scale {s}, pads {pads}: wrote outside the output"
            assert _bits_equal(R.frames(raw, ya, xa, pads, minmax).cpu().numpy(), got)          # the wrapper
    print(f"worst: {worst:.3e}")


# ---- 2. predictions -> the frame's grid ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_planes_chw_equal_the_restatement(dev, shape):
    """C = 1, CHW: the source sits behind non-zero top / left padding (NaN) of a larger buffer"""
    from microbeseg_amd.inference import resample as R
    H, W = shape
    n, pads = 3, (3, 5)
    rng = np.random.Generator(np.random.PCG64(H + W))
    for s in FACTORS:
        ho, wo = R.out_size(H, s), R.out_size(W, s)
        ya, xa = R.axis(H, ho, dev), R.axis(W, wo, dev)
        p = rng.uniform(-1, 1, size=(n, 1, H, W)).astype(np.float32)
        big = np.full((n, 1, H + pads[0], W + pads[1]), np.nan, np.float32)
        big[:, :, pads[0]:, pads[1]:] = p
        got = R.planes(torch.from_numpy(big).to(dev), ya, xa, pads=pads).cpu().numpy()
        want = resample_ref.resample(p, ho, wo)
        assert got.shape == want.shape == (n, 1, ho, wo)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"CHW {shape} x {s}: max |difference| {err:.3e}")
        assert err <= BOUND, f"scale {s}: {err:.3e}"


@pytest.mark.parametrize("shape", SHAPES)
def test_planes_hwc3_equal_the_restatement(dev, shape):
    """C = 3, HWC source and destination (pixel stride 3), into a guarded destination"""
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import resample as R
    H, W = shape
    n = 3
    rng = np.random.Generator(np.random.PCG64(7 * H + W))
    for s in FACTORS:
        ho, wo = R.out_size(H, s), R.out_size(W, s)
        ya, xa = R.axis(H, ho, dev), R.axis(W, wo, dev)
        p = rng.uniform(-1, 1, size=(n, H, W, 3)).astype(np.float32)
        src = torch.from_numpy(p).to(dev)
        want = resample_ref.resample(np.moveaxis(p, 3, 1), ho, wo)                        # (n, 3, ho, wo)
        buf, dst = _guarded((n, ho, wo, 3), dev)
        sfs, srs, sps, scs = src.stride()
        dfs, drs, dps, dcs = dst.stride()
        assert _lib.load().mseg_resample_planes(src.data_ptr(), sfs, scs, srs, sps, n, 3, C.byref(ya.desc), C.byref(xa.desc),
                                                dst.data_ptr(), dfs, dcs, drs, dps, _stream()) == 0
        got = dst.permute(0, 3, 1, 2).cpu().numpy()
        assert not np.isnan(got).any()
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"HWC-3 {shape} x {s}: max |difference| {err:.3e}")
        assert err <= BOUND, f"scale {s}: {err:.3e}"
        assert _guards_intact(buf)
        assert _bits_equal(R.planes(src.permute(0, 3, 1, 2), ya, xa, hwc=True).permute(0, 3, 1, 2).cpu().numpy(), got)


def test_large_ratios_take_the_halved_tiles(dev):
    """342 x 315 -> 60 x 60 (tables made directly: ratios 5.7 and 5.25) has the 12 and 11 taps the kernels go up to, and a
    64 x 16 output tile would need a window of about 315 x 97 (147 KB), so the tile is halved twice (32 x 8); 300 x 290 at
    0.25 is ratio 4 with 8 taps and one halving.  Several tiles, ragged last tiles, the same bound."""
    from microbeseg_amd.inference import resample as R
    for (H, W), (hs, ws), taps in (((342, 315), (60, 60), (12, 11)), ((300, 290), (75, 73), (8, 8))):
        ya, xa = R.axis(H, hs, dev), R.axis(W, ws, dev)
        assert (ya.taps, xa.taps) == taps
        frames = _frames(np.uint16, (H, W), seed=H)[:2]
        raw, minmax = _upload(frames, dev)
        for pads in PADS:
            want = resample_ref.network_input(frames, hs, ws, pads)
            buf, out = _guarded(want.shape, dev)
            assert _frames_into(raw, minmax, ya.desc, xa.desc, pads, out) == 0
            got = out.cpu().numpy()
            assert not np.isnan(got).any()
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"uint16 {(H, W)} -> {(hs, ws)} pads {pads}: max |difference| {err:.3e}")
            assert err <= BOUND and _guards_intact(buf)
        p = np.random.Generator(np.random.PCG64(W)).uniform(-1, 1, size=(2, H, W, 3)).astype(np.float32)
        got = R.planes(torch.from_numpy(p).to(dev).permute(0, 3, 1, 2), ya, xa, hwc=True).permute(0, 3, 1, 2).cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - resample_ref.resample(np.moveaxis(p, 3, 1), hs, ws)).max())
        print(f"HWC-3 {(H, W)} -> {(hs, ws)}: max |difference| {err:.3e}")
        assert err <= BOUND


def test_constant_planes_stay_constant(dev):
    from microbeseg_amd.inference import resample as R
    for H, W in SHAPES:
        for s in FACTORS:
            ya, xa = R.axis(H, R.out_size(H, s), dev), R.axis(W, R.out_size(W, s), dev)
            for value in (1.0, -0.37, 0.0):
                t = torch.full((2, 1, H, W), value, dtype=torch.float32, device=dev)
                got = R.planes(t, ya, xa).cpu().numpy()
                assert float(np.abs(got - np.float32(value)).max()) <= 1e-6, (H, W, s, value)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_batch_invariance_and_determinism(dev, dtype):
    """the n = 3 call equals three n = 1 calls bit for bit, and a second run gives the same bits"""
    from microbeseg_amd.inference import resample as R
    H, W = 70, 131
    frames = _frames(dtype, (H, W), seed=3)
    raw, minmax = _upload(frames, dev)
    planes = torch.from_numpy(_frames(np.float32, (H, W), seed=4))[:, None].to(dev)
    for s in FACTORS:
        ya, xa = R.axis(H, R.out_size(H, s), dev), R.axis(W, R.out_size(W, s), dev)
        whole = R.frames(raw, ya, xa, (5, 11), minmax).cpu().numpy()
        again = R.frames(raw, ya, xa, (5, 11), minmax).cpu().numpy()
        assert _bits_equal(whole, again)
        for k in range(3):
            one = R.frames(raw[k:k + 1], ya, xa, (5, 11), None if minmax is None else minmax[k:k + 1]).cpu().numpy()
            assert _bits_equal(one[0], whole[k]), f"scale {s}, frame {k}"
        whole = R.planes(planes, ya, xa).cpu().numpy()
        assert _bits_equal(whole, R.planes(planes, ya, xa).cpu().numpy())
        for k in range(3):
            assert _bits_equal(R.planes(planes[k:k + 1], ya, xa).cpu().numpy()[0], whole[k]), f"scale {s}, plane {k}"


def test_bad_arguments_are_refused_and_nothing_is_written(dev):
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import resample as R
    H, W = 37, 53
    frames = _frames(np.uint16, (H, W), seed=1)
    raw, minmax = _upload(frames, dev)
    ya, xa = R.axis(H, 19, dev), R.axis(W, 27, dev)
    buf, out = _guarded((3, 19, 27), dev)

    def with_taps(a, taps):
        d = a.desc
        return _lib.MsegResampleAxis(d.first, d.count, d.weight, d.host_first, d.host_count, d.n_in, d.n_out, taps, 0)
    assert _frames_into(raw, minmax, with_taps(ya, 13), xa.desc, (0, 0), out) == EINVAL
    assert _frames_into(raw, minmax, ya.desc, with_taps(xa, 13), (0, 0), out) == EINVAL
    assert _frames_into(raw, minmax, ya.desc, xa.desc, (0, 0), out, dtype=_lib.PIX_I32) == EINVAL
    assert _frames_into(raw, minmax, ya.desc, xa.desc, (0, 0), out, dtype=7) == EINVAL
    assert _frames_into(raw, None, ya.desc, xa.desc, (0, 0), out) == EINVAL                  # raw frames without extrema
    src = torch.zeros((3, 1, H, W), device=dev)
    lib = _lib.load()
    for y, x in ((with_taps(ya, 13), xa.desc), (ya.desc, with_taps(xa, 13))):
        assert lib.mseg_resample_planes(src.data_ptr(), H * W, H * W, W, 1, 3, 1, C.byref(y), C.byref(x), out.data_ptr(),
                                        19 * 27, 19 * 27, 27, 1, _stream()) == EINVAL
    short = _lib.MsegResampleAxis(ya.desc.first, ya.desc.count, ya.desc.weight, ya.desc.host_first, ya.desc.host_count,
                                  H - 1, 19, ya.taps, 0)                                     # the last window passes n_in
    assert lib.mseg_resample_planes(src.data_ptr(), H * W, H * W, W, 1, 3, 1, C.byref(short), C.byref(xa.desc),
                                    out.data_ptr(), 19 * 27, 19 * 27, 27, 1, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and _guards_intact(buf)
    with pytest.raises(RuntimeError, match="taps"):
        R.axis(100, 10, dev)


# ---- networks ----------------------------------------------------------------------------------------------------------------
def _worker(tmp_path, unet_type, norm="bn", seed=5):
    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.utils.unets import build_unet
    torch.manual_seed(seed)
    label_type = "distance" if unet_type == "DU" else "boundary"
    net = build_unet(unet_type, "relu", "conv", norm, torch.device("cuda:0"), 1, ch_out=1 if unet_type == "DU" else 3,
                     filters=(8, 16))
    with torch.no_grad():                            # running statistics away from their initial values
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    base = tmp_path / f"{label_type}_model_00"
    torch.save(net.state_dict(), str(base) + ".pth")
    with open(str(base) + ".json", "w") as f:
        json.dump({"architecture": [unet_type, "conv", "relu", norm, [8, 16]], "label_type": label_type}, f)
    return InferWorker(model=str(base), device="cuda:0", ths=(0.10, 0.45))


def _count_net_calls(worker):
    calls = []
    worker.net.register_forward_pre_hook(lambda m, inp: calls.append(int(getattr(inp[0], "shape", (1,))[0])))
    return calls


@pytest.mark.parametrize("unet_type", ["DU", "U"])
def test_predict_scaled_equals_the_steps_done_by_hand(tmp_path, dev, unet_type):
    from microbeseg_amd import engine
    from microbeseg_amd.inference import resample as R
    from microbeseg_amd.utils.utils import pad_amounts
    worker = _worker(tmp_path, unet_type)
    worker.scale = 0.5
    n, H, W = 3, 70, 131
    rng = np.random.Generator(np.random.PCG64(41))
    stack = np.stack([rng.integers(100 * t, 3000 + 20000 * t, size=(H, W)).astype(np.uint16) for t in range(n)])
    calls = _count_net_calls(worker)
    got = worker.predict_scaled(stack)
    assert calls == [n], calls                                  # one forward for the group
    hs, ws = R.out_size(H, 0.5), R.out_size(W, 0.5)
    assert (hs, ws) == (35, 66)
    pads = pad_amounts((hs, ws))
    assert pads[0] > 0 and pads[1] > 0
    raw, minmax = _upload(stack, dev)
    with torch.no_grad():
        x = R.frames(raw, R.axis(H, hs, dev), R.axis(W, ws, dev), pads, minmax)
        assert tuple(x.shape) == (n, hs + pads[0], ws + pads[1])
        with engine.precision_scope(worker.precision):
            pred = worker.net(x[:, None])
        yup, xup = R.axis(hs, H, dev), R.axis(ws, W, dev)
        if unet_type == "DU":
            want = [R.planes(t, yup, xup, pads=pads)[:, 0] for t in pred]
            assert isinstance(got, tuple) and len(got) == 2
            for g, w in zip(got, want):
                assert tuple(g.shape) == (n, H, W)
                assert _bits_equal(g.cpu().numpy(), w.cpu().numpy())
        else:
            probs = torch.stack([worker._softmax_hwc(pred[j:j + 1], pads) for j in range(n)])
            assert tuple(probs.shape) == (n, hs, ws, 3)
            want = R.planes(probs.permute(0, 3, 1, 2), yup, xup, hwc=True)
            assert tuple(got.shape) == (n, H, W, 3)
            assert _bits_equal(got.cpu().numpy(), want.cpu().numpy())
            total = got.cpu().numpy().astype(np.float64).sum(axis=3)
            assert float(np.abs(total - 1).max()) <= 1e-5


# ---- masks and plumbing --------------------------------------------------------------------------------------------------
def _synthetic_maps(T, H, W, seed=99):
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    return [synth.synth_prediction_maps(rng, H, W, 5 + 4 * t, rmin=4.0, rmax=9.0)[::-1] for t in range(T)]     # (border, cell)


def _distance_hook(T, H, W, dev, seed=99):
    """per-frame synthetic full-resolution maps handed out in call order; H x W needs no padding, so the prediction of
    the scale = 1 routes and the full-resolution prediction of the scaled route have the same shape"""
    maps = [(torch.from_numpy(b).to(dev), torch.from_numpy(c).to(dev)) for b, c in _synthetic_maps(T, H, W, seed)]
    calls = []

    def hook(pred):
        border, cell = pred
        assert tuple(border.shape) == (1, 1, H, W) and cell.shape == border.shape
        t = len(calls)
        calls.append(t)
        return maps[t][0][None, None], maps[t][1][None, None]
    return hook, calls


def test_masks_under_a_hook_equal_those_at_scale_1_distance_model(tmp_path, dev):
    worker = _worker(tmp_path, "DU")
    T, H, W = 5, 128, 128
    rng = np.random.Generator(np.random.PCG64(8))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    hook, calls = _distance_hook(T, H, W, dev)
    worker.prediction_hook = hook
    want = worker.infer_stack(stack)                            # scale = 1
    assert calls == list(range(T)) and int(sum(int(w.max()) for w in want)) > 20
    net_calls = _count_net_calls(worker)
    for s, fb, batches in ((0.5, 1, [1] * T), (2.0, 1, [1] * T), (0.5, 0, [T]), (0.5, 2, [2, 2, 1]), (2.0, 0, [T])):
        del calls[:], net_calls[:]
        worker.scale, worker.frame_batch = s, fb
        got = worker.infer_stack(stack)
        assert calls == list(range(T)), calls                   # once per frame, in frame order
        assert net_calls == batches, (s, fb, net_calls)         # the network did run, at the scaled size, in these groups
        assert got.dtype == np.uint16 and got.shape == (T, H, W)
        for t in range(T):
            assert np.array_equal(got[t], want[t]), f"scale {s}, frame_batch {fb}, frame {t}"


def test_masks_under_a_hook_equal_those_at_scale_1_boundary_model(tmp_path, dev):
    """the hook of the scale = 1 routes returns logits, which those routes send through mseg_softmax3_hwc; the scaled
    route's prediction is probabilities, so there the hook hands out the same kernel's probabilities of the same logits"""
    worker = _worker(tmp_path, "U")
    T, H, W = 3, 128, 128
    rng = np.random.Generator(np.random.PCG64(9))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    logits = []
    for border, cell in _synthetic_maps(T, H, W, seed=17):
        p1 = np.clip(cell * 2.0, 0, 1) * (1 - np.clip(border * 1.2, 0, 1))
        p2 = np.clip(border * 1.2, 0, 1) * (cell > 0.02)
        p0 = np.clip(1 - p1 - p2, 0.0, 1)
        probs = np.stack([p0, p1, p2], 0).astype(np.float32)
        probs = probs / probs.sum(0, keepdims=True)
        logits.append(torch.from_numpy(np.log(probs + 1e-6)[None]).to(dev))
    calls, as_probs = [], [False]

    def hook(pred):
        assert tuple(pred.shape) == (1, 3, H, W)
        calls.append(len(calls))
        lg = logits[calls[-1]]
        return worker._softmax_hwc(lg, (0, 0)).permute(2, 0, 1)[None] if as_probs[0] else lg
    worker.prediction_hook = hook
    want = worker.infer_stack(stack)
    assert calls == list(range(T)) and int(sum(int(w.max()) for w in want)) > 10
    as_probs[0] = True
    for s in (0.5, 2.0):
        del calls[:]
        worker.scale = s
        got = worker.infer_stack(stack)
        assert calls == list(range(T)) and got.dtype == np.uint16 and got.shape == (T, H, W)
        for t in range(T):
            assert np.array_equal(got[t], want[t]), f"scale {s}, frame {t}"


def _smooth_stack(T, H, W, seed):
    """smooth frames: an untrained network maps blobs to blobs"""
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = []
    for t in range(T):
        cell, _ = synth.synth_prediction_maps(rng, H, W, 6 + t, rmin=5.0, rmax=11.0)
        frames.append(np.clip(cell * 50000 + rng.normal(0, 800, cell.shape), 0, 65535).astype(np.uint16))
    return np.stack(frames)


def test_masks_without_a_hook_inference_and_clahe(tmp_path, dev):
    """no hook: the masks are the post-processing of predict_scaled at the frame's resolution; inference() on one padded
    frame is infer_stack on that frame; a float32 copy gives the same masks; apply_clahe runs"""
    from microbeseg_amd.inference import postprocessing as pp
    worker = _worker(tmp_path, "DU")
    worker.scale = 0.5
    T, H, W = 2, 100, 130
    stack = _smooth_stack(T, H, W, seed=10)
    border, cell = worker.predict_scaled(stack[:1])
    assert tuple(cell.shape) == (1, H, W)
    # an untrained network predicts no distance maps: thresholds from the distribution of its own output
    b = torch.tan(border[0].clamp(0, 1) ** 2)
    b = torch.where(b < 0.05, torch.zeros_like(b), b).clamp(0, 1)
    worker.ths = [float(torch.quantile(cell[0].flatten(), 0.85)), float(torch.quantile((cell[0] - b).flatten(), 0.96))]
    got = worker.infer_stack(stack)
    assert got.shape == (T, H, W) and got.dtype == np.uint16
    total = 0
    for t in range(T):
        border, cell = worker.predict_scaled(stack[t:t + 1])
        labels, _, _ = pp.distance_postprocessing_device(border[0].contiguous(), cell[0].contiguous(),
                                                         th_seed=worker.ths[1], th_cell=worker.ths[0], col_major_ids=True)
        want = labels.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[t], want), f"frame {t}: {(got[t] != want).sum()} px differ"
        total += int(want.max())
    assert total > 0
    assert np.array_equal(worker.infer_stack(stack.astype(np.float32)), got)
    f = stack[1]
    padded, pads = worker.pad_frame(np.copy(f), np.min(f))
    assert pads[0] > 0 and pads[1] > 0
    one = worker.inference(padded, np.min(f), np.max(f), pads)
    assert one.shape == (H, W) and one.dtype == np.uint16
    assert np.array_equal(one, got[1])
    worker.apply_clahe = True
    enhanced = worker.infer_stack(stack)
    assert enhanced.shape == (T, H, W) and enhanced.dtype == np.uint16


def _halving(n, limit):
    """batch sizes InferWorker._forward_group asks of the network for a group of n frames when more than ``limit`` samples
    do not fit: a forward that fails is retried at half its size (at least 1) from the same frame on, and that size is kept
    for the rest of the group; a single frame that does not fit is given up"""
    asked, i, size = [], 0, n
    while i < n:
        m = min(size, n - i)
        asked.append(m)
        if m > limit and m > 1:
            size = max(1, m // 2)
            continue
        i += m
    return asked


def test_groups_that_do_not_fit_in_memory(tmp_path, dev):
    """a group whose forward runs out of memory is halved down to what fits and the masks stay the same; a frame that does
    not fit alone gets the zero mask and no hook call, like the routes at scale 1"""
    worker = _worker(tmp_path, "DU")
    worker.scale, worker.frame_batch = 0.5, 2
    T, H, W = 4, 128, 128
    rng = np.random.Generator(np.random.PCG64(14))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    hook, calls = _distance_hook(T, H, W, dev, seed=7)
    worker.prediction_hook = hook
    want = worker.infer_stack(stack)
    assert calls == list(range(T)) and int(want.max()) > 5
    forward, asked, limit = worker.net.forward, [], [1]

    def short_of_memory(x):
        asked.append(int(x.shape[0]))
        if x.shape[0] > limit[0]:
            raise RuntimeError("HIP out of memory. Tried to allocate 1.00 GiB")
        return forward(x)
    worker.net.forward = short_of_memory
    del calls[:]
    got = worker.infer_stack(stack)
    assert asked == _halving(2, 1) * 2 == [2, 1, 1] * 2, asked          # every group starts at frame_batch again
    assert calls == list(range(T)) and np.array_equal(got, want)
    limit[0] = 0
    del calls[:], asked[:]
    got = worker.infer_stack(stack)
    assert asked == _halving(2, 0) * 2 == [2, 1, 1] * 2, asked
    assert not calls and got.shape == (T, H, W) and got.dtype == np.uint16 and not got.any()


def test_scale_1_is_untouched_and_combinations_are_refused_before_any_launch(tmp_path, dev, monkeypatch):
    from microbeseg_amd import _lib
    worker = _worker(tmp_path, "DU")
    rng = np.random.Generator(np.random.PCG64(13))
    stack = rng.integers(0, 60000, size=(3, 100, 130)).astype(np.uint16)
    untouched = worker.infer_stack(stack)
    lib = _lib.load()

    def boom(*a, **k):
        raise AssertionError("a resample entry point was reached")
    monkeypatch.setattr(lib, "mseg_resample_frames", boom, raising=False)
    monkeypatch.setattr(lib, "mseg_resample_planes", boom, raising=False)
    for one in (1, 1.0, np.float64(1.0)):
        worker.scale = one
        assert np.array_equal(worker.infer_stack(stack), untouched)
    worker.frame_batch = 8
    assert np.array_equal(worker.infer_stack(stack), untouched)
    f = stack[0]
    padded, pads = worker.pad_frame(np.copy(f), np.min(f))
    assert np.array_equal(worker.inference(padded, np.min(f), np.max(f), pads), untouched[0])
    # what the scaled route cannot take is refused before anything is launched: no resample call, no forward
    calls = _count_net_calls(worker)
    worker.frame_batch, worker.scale = 1, 0.5
    for attr, value, match in (("tta", 4, "tta"), ("sliding_window", True, "sliding_window")):
        setattr(worker, attr, value)
        for call in (lambda: worker.infer_stack(stack), lambda: worker.predict_scaled(stack),
                     lambda: worker.inference(padded, np.min(f), np.max(f), pads)):
            with pytest.raises(RuntimeError, match=match):
                call()
        setattr(worker, attr, {"tta": 1, "sliding_window": False}[attr])
    for bad in (0.2, 4.5, True, float("nan")):
        worker.scale = bad
        with pytest.raises(ValueError):
            worker.infer_stack(stack)
    assert not calls
