"""GPU (MI355X): test-time augmentation for inference (InferWorker.tta) — the two kernels of csrc/tta.hip
bit for bit against the numpy restatement tests/tta_ref.py, the round trip expand -> merge, the merged prediction of real
networks against the restatement built from the existing forward, the masks, the chunking, and the property the feature
is for: the merged prediction of a transformed frame is the transformed merged prediction, up to summation order."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import tta_ref

pytestmark = pytest.mark.gpu

EINVAL = -1
SHAPES = [(64, 64), (37, 53), (70, 45), (40, 72)]
CODE_LISTS = [(0, 1), (0, 1, 2, 4), (3, 5, 6, 7)]          # every list of the member sets 2 / 4 / 8, by shape class
GUARD = 1024                                               # words on either side of an output
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
    """-> (device tensor as tta.expand takes it, minmax or None)"""
    from microbeseg_amd import _lib, engine
    if frames.dtype == np.float32:
        return torch.from_numpy(frames).to(dev), None
    raw = torch.from_numpy(frames.view(np.int16) if frames.dtype == np.uint16 else frames).to(dev)
    minmax = torch.empty((len(frames), 2), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().mseg_frames_minmax(raw.data_ptr(), engine.RawFrame.PIX[raw.dtype], len(frames),
                                              frames.shape[1] * frames.shape[2], minmax.data_ptr(), _stream()), "minmax")
    return raw, minmax


def _expand_into(raw, minmax, codes, pads, out):
    from microbeseg_amd import _lib
    pix = {torch.uint8: _lib.PIX_U8, torch.int16: _lib.PIX_U16, torch.float32: _lib.PIX_F32}[raw.dtype]
    arr = (C.c_int32 * len(codes))(*codes)
    n, h0, w0 = raw.shape
    return _lib.load().mseg_tta_expand(raw.data_ptr(), pix, n, h0, w0, None if minmax is None else minmax.data_ptr(), arr,
                                       len(codes), int(pads[0]), int(pads[1]), out.data_ptr(), _stream())


# ---- 1. expand ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_expand_equals_the_host_formula_bit_for_bit(dev, dtype, shape):
    from microbeseg_amd.inference import tta
    frames = _frames(dtype, shape, seed=shape[0] * 100 + shape[1])
    if dtype != np.float32:
        assert int(frames[2].max()) - int(frames[2].min()) == 1
    raw, minmax = _upload(frames, dev)
    for codes in CODE_LISTS:
        (cs, (hm, wm), pads), = tta.shape_classes(codes, *shape)
        assert cs == codes
        want = np.stack([np.stack([tta_ref.member_input(f, c)[0] for f in frames]) for c in codes])
        assert want.shape == (len(codes), 3, hm + pads[0], wm + pads[1])
        buf, out = _guarded(want.shape, dev)
        assert _expand_into(raw, minmax, codes, pads, out) == 0
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), f"codes {codes}: {int(np.isnan(got).sum())} elements were not written"
        assert _bits_equal(got, want), f"codes {codes}: {(got != want).sum()} values differ"
        assert _guards_intact(buf), f"codes {codes}: wrote outside the output"
        assert _bits_equal(tta.expand(raw, codes, pads, minmax).cpu().numpy(), want)          # the wrapper
    if shape == (37, 53):
        assert want.shape[2:] == (64, 64)           # padded, transposed
    if shape == (70, 45):
        assert want.shape[2:] == (64, 128)
    # one call is one shape class: a mixed list is refused and nothing is written
    buf, out = _guarded((2, 3, 256, 256), dev)
    for mixed in ((0, 3), (6, 1), (0, 1, 2, 5)):
        assert _expand_into(raw, minmax, mixed, (0, 0), out) == EINVAL
    assert _expand_into(raw, minmax, (0, 8), (0, 0), out) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and _guards_intact(buf)


# ---- 2. merge ----------------------------------------------------------------------------------------------------------------
def _merge_into(members, n, ch, H, W, hwc, dev):
    """mseg_tta_merge into a guarded destination -> (buffer, destination view (n, C, H, W) or (n, H, W, C))"""
    from microbeseg_amd import _lib
    buf, dst = _guarded((n, H, W, ch) if hwc else (n, ch, H, W), dev)
    if hwc:
        fs, rs, ps, cs = dst.stride()
    else:
        fs, cs, rs, ps = dst.stride()
    arr = (_lib.MsegTtaMember * len(members))(*members)
    code = _lib.load().mseg_tta_merge(arr, len(members), n, ch, H, W, dst.data_ptr(), fs, cs, rs, ps, _stream())
    return code, buf, dst


def _mixed(rng, shape):
    """fp32 of mixed sign and magnitude (10^-3 .. 10^3): sums whose rounding depends on the order"""
    return (rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 3, size=shape)).astype(np.float32)


@pytest.mark.parametrize("shape", [(37, 53), (70, 45), (64, 64), (33, 130)])
@pytest.mark.parametrize("K", [2, 4, 8])
def test_merge_of_planes_equals_the_ordered_sum_bit_for_bit(dev, K, shape):
    """C = 1, CHW: every member sits inside a larger buffer — two leading frames that belong to other members, top / left
    padding filled with NaN — and is addressed through the descriptor's offset and strides"""
    from microbeseg_amd.inference import tta
    H, W = shape
    n, pt, pl = 3, 3, 5
    rng = np.random.Generator(np.random.PCG64(K * 1000 + H))
    codes = tta.member_codes(K)
    members, planes, keep = [], [], []
    for c in codes:
        hm, wm = (W, H) if c in tta.TRANSPOSING else (H, W)
        p = _mixed(rng, (n, 1, hm, wm))
        big = np.full((n + 2, 1, hm + pt, wm + pl), np.nan, np.float32)
        big[2:, :, pt:, pl:] = p
        t = torch.from_numpy(big).to(dev)
        keep.append(t)
        members.append(tta.member(t, c, first=2, pads=(pt, pl)))
        planes.append(p)
    want = tta_ref.merge(planes, codes, K)
    code, buf, dst = _merge_into(members, n, 1, H, W, False, dev)
    assert code == 0
    got = dst.cpu().numpy()
    assert _bits_equal(got, want), f"{(got != want).sum()} of {got.size} values differ"
    assert _guards_intact(buf)
    assert _bits_equal(tta.merge(members, n, 1, H, W).cpu().numpy(), want)                   # the wrapper


@pytest.mark.parametrize("shape", [(37, 53), (70, 45), (64, 64), (33, 130)])
@pytest.mark.parametrize("K", [2, 4, 8])
def test_merge_of_hwc_probabilities_equals_the_ordered_sum_bit_for_bit(dev, K, shape):
    """C = 3, HWC sources and destination (pixel stride 3): the sources are what mseg_softmax3_hwc writes for random
    logits, and the reference sums those same device outputs — the softmax's own rounding is not under test"""
    from microbeseg_amd.inference import tta
    from microbeseg_amd.inference.infer import InferWorker
    H, W = shape
    n, pt, pl = 3, 16, 32
    rng = np.random.Generator(np.random.PCG64(K * 2000 + W))
    codes = tta.member_codes(K)
    members, planes, keep = [], [], []
    for c in codes:
        hm, wm = (W, H) if c in tta.TRANSPOSING else (H, W)
        logits = torch.from_numpy((rng.normal(size=(n, 3, hm + pt, wm + pl)) * 4).astype(np.float32)).to(dev)
        probs = torch.stack([InferWorker._softmax_hwc(logits[i:i + 1], (pt, pl)) for i in range(n)])
        assert probs.shape == (n, hm, wm, 3) and probs.is_contiguous()
        keep.append(probs)
        members.append(tta.member(probs.permute(0, 3, 1, 2), c))
        planes.append(probs.permute(0, 3, 1, 2).cpu().numpy())
    want = tta_ref.merge(planes, codes, K)                       # (n, 3, H, W)
    code, buf, dst = _merge_into(members, n, 3, H, W, True, dev)
    assert code == 0
    got = dst.permute(0, 3, 1, 2).cpu().numpy()
    assert _bits_equal(got, want), f"{(got != want).sum()} of {got.size} values differ"
    assert _guards_intact(buf)
    assert _bits_equal(tta.merge(members, n, 3, H, W, hwc=True).permute(0, 3, 1, 2).cpu().numpy(), want)


def test_merge_refuses_bad_arguments(dev):
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import tta
    t = torch.zeros((1, 1, 8, 8), device=dev)
    m = tta.member(t, 0)
    out = torch.zeros((1, 1, 8, 8), device=dev)
    lib = _lib.load()
    for k in (3, 5, 6, 7, 9):                       # the scale 1 / K must be exact, and a launch carries 8 descriptors
        arr = (_lib.MsegTtaMember * k)(*([m] * k))
        assert lib.mseg_tta_merge(arr, k, 1, 1, 8, 8, out.data_ptr(), 64, 64, 8, 1, _stream()) == EINVAL
    arr = (_lib.MsegTtaMember * 2)(m, m)
    assert lib.mseg_tta_merge(arr, 0, 1, 1, 8, 8, out.data_ptr(), 64, 64, 8, 1, _stream()) == EINVAL
    assert lib.mseg_tta_merge(arr, 2, 1, 1, 8, 8, None, 64, 64, 8, 1, _stream()) == EINVAL
    assert lib.mseg_tta_merge(None, 2, 1, 1, 8, 8, out.data_ptr(), 64, 64, 8, 1, _stream()) == EINVAL
    assert lib.mseg_tta_merge(arr, 2, 0, 1, 8, 8, out.data_ptr(), 64, 64, 8, 1, _stream()) == EINVAL
    assert lib.mseg_tta_merge(arr, 2, 1, 1, 0, 8, out.data_ptr(), 64, 64, 8, 1, _stream()) == EINVAL
    null = _lib.MsegTtaMember(None, 64, 64, 8, 1, 0, 0)
    arr = (_lib.MsegTtaMember * 2)(m, null)
    assert lib.mseg_tta_merge(arr, 2, 1, 1, 8, 8, out.data_ptr(), 64, 64, 8, 1, _stream()) == EINVAL


# ---- 3. round trip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_expand_then_merge_returns_the_frame(dev, shape):
    """small integers (|v| <= 64): sums of at most 8 of them and the power-of-two scale are exact, so merging the
    cropped members must give back the frame — the inverse mapping, checked without tests/tta_ref.py"""
    from microbeseg_amd.inference import tta
    H, W = shape
    rng = np.random.Generator(np.random.PCG64(H + 7 * W))
    frames = rng.integers(-64, 65, size=(3, H, W)).astype(np.float32)
    raw = torch.from_numpy(frames).to(dev)
    for K in (1, 2, 4, 8):
        members, keep = {}, []
        for cs, _, pads in tta.shape_classes(tta.member_codes(K), H, W):
            x = tta.expand(raw, cs, pads)
            keep.append(x)
            for ci, c in enumerate(cs):
                members[c] = tta.member(x.view(len(cs) * 3, 1, x.shape[2], x.shape[3]), c, first=ci * 3, pads=pads)
        got = tta.merge([members[c] for c in sorted(members)], 3, 1, H, W)[:, 0].cpu().numpy()
        assert _bits_equal(got, frames), f"K = {K}: {(got != frames).sum()} values differ"


# ---- networks ----------------------------------------------------------------------------------------------------------------
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


def _count_net_calls(worker):
    calls = []
    worker.net.register_forward_pre_hook(lambda m, inp: calls.append(int(getattr(inp[0], "shape", (1,))[0])))
    return calls


def _heads(pred):
    """a prediction as a list of numpy arrays (n, C, ...)"""
    return [p.cpu().numpy() for p in (pred if isinstance(pred, tuple) else (pred,))]


def _restated_merge(worker, stack, K):
    """the merged prediction of ``stack`` built from the existing path: per shape class ONE forward_frames call on the
    transformed frames, code by code (the batch predict_merged forwards, in its member-major order), crop, softmax for
    the boundary model, then numpy: inverse transform and the ordered fp32 sum.  -> list of (n, C, H, W) per head"""
    from microbeseg_amd.inference import tta
    n = len(stack)
    per_code = {}
    for cs, _, pads in tta.shape_classes(tta.member_codes(K), *stack.shape[1:]):
        batch = np.concatenate([np.stack([tta_ref.transform(f, c) for f in stack]) for c in cs])
        pred = worker.forward_frames(batch)
        if isinstance(pred, tuple):
            heads = [p[:, :, pads[0]:, pads[1]:].cpu().numpy() for p in pred]
        else:
            probs = torch.stack([worker._softmax_hwc(pred[j:j + 1], pads) for j in range(pred.shape[0])])
            heads = [probs.permute(0, 3, 1, 2).cpu().numpy()]
        for ci, c in enumerate(cs):
            per_code[c] = [h[ci * n:(ci + 1) * n] for h in heads]
    codes = sorted(per_code)
    return [tta_ref.merge([per_code[c][h] for c in codes], codes, K) for h in range(len(per_code[codes[0]]))]


@pytest.mark.parametrize("unet_type,norm", [("DU", "bn"), ("DU", "gn"), ("U", "bn")])
def test_merged_prediction_equals_the_restatement_from_the_existing_forward(tmp_path, dev, unet_type, norm):
    """bit for bit: predict_merged forwards the same batches as forward_frames on the transformed frames (same launches,
    deterministic kernels), so only the expansion, the crop, the mapping back and the sum can differ"""
    from microbeseg_amd.inference import tta
    worker = _worker(tmp_path, unet_type, norm)
    worker.frame_batch = 3                          # 3 * K members per forward at most: the 3 frames are one group
    calls = _count_net_calls(worker)
    rng = np.random.Generator(np.random.PCG64(41))
    for shape in ((100, 130), (64, 64)):
        stack = np.stack([rng.integers(100 * t, 3000 + 20000 * t, size=shape).astype(np.uint16) for t in range(3)])
        for K in (2, 4, 8):
            worker.tta = K
            del calls[:]
            got = worker.predict_merged(stack)
            classes = tta.shape_classes(tta.member_codes(K), *shape)
            assert calls == [3 * len(cs) for cs, _, _ in classes], calls
            if unet_type == "DU":
                assert all(tuple(g.shape) == (3,) + shape for g in got)
                got = [g.cpu().numpy()[:, None] for g in got]
            else:
                assert tuple(got.shape) == (3,) + shape + (3,)
                got = [got.permute(0, 3, 1, 2).cpu().numpy()]
            want = _restated_merge(worker, stack, K)
            assert len(got) == len(want)
            for h, (g, w) in enumerate(zip(got, want)):
                assert _bits_equal(g, w), f"{shape}, tta {K}, head {h}: {(g != w).sum()} of {g.size} values differ"


# ---- 5. masks and plumbing -------------------------------------------------------------------------------------------------
def _synthetic_maps(T, H, W, dev, seed=99):
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    maps = []
    for t in range(T):
        cell, border = synth.synth_prediction_maps(rng, H, W, 5 + 4 * t, rmin=4.0, rmax=9.0)
        if t % 5 == 3:
            cell = (np.round(cell * 16) / 16).astype(np.float32)
        maps.append((border, cell))
    return maps


def _distance_hook(T, H, W, dev, seed=99):
    """per-frame synthetic maps handed out in call order, un-padded: H x W needs no padding, so the prediction of the
    tta = 1 routes and the merged prediction (which never has padding) have the same shape"""
    maps = [(torch.from_numpy(b).to(dev), torch.from_numpy(c).to(dev)) for b, c in _synthetic_maps(T, H, W, dev, seed)]
    calls = []

    def hook(pred):
        border, cell = pred
        assert tuple(border.shape) == (1, 1, H, W) and cell.shape == border.shape
        t = len(calls)
        calls.append(t)
        return maps[t][0][None, None], maps[t][1][None, None]
    return hook, calls


def test_masks_under_a_hook_equal_those_without_tta_distance_model(tmp_path, dev):
    worker = _worker(tmp_path, "DU", "bn")
    T, H, W = 6, 128, 128
    rng = np.random.Generator(np.random.PCG64(8))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    hook, calls = _distance_hook(T, H, W, dev)
    worker.prediction_hook = hook
    want = worker.infer_stack(stack)                            # tta = 1
    assert calls == list(range(T)) and int(sum(int(w.max()) for w in want)) > 20
    for fb in (1, 4):
        del calls[:]
        worker.tta, worker.frame_batch = 4, fb
        got = worker.infer_stack(stack)
        assert calls == list(range(T)), calls                   # once per frame, in frame order
        assert got.dtype == np.uint16 and got.shape == want.shape
        for t in range(T):
            assert np.array_equal(got[t], want[t]), f"frame_batch {fb}, frame {t}: {(got[t] != want[t]).sum()} px differ"


def test_masks_under_a_hook_equal_those_without_tta_boundary_model(tmp_path, dev):
    """the hook of the tta = 1 routes returns logits, which those routes send through mseg_softmax3_hwc; the merged
    prediction is probabilities, so under TTA the hook hands out the same kernel's probabilities of the same logits"""
    worker = _worker(tmp_path, "U", "bn")
    T, H, W = 6, 128, 128
    rng = np.random.Generator(np.random.PCG64(9))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    logits = []
    for border, cell in _synthetic_maps(T, H, W, dev, seed=17):
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
    assert calls == list(range(T)) and int(sum(int(w.max()) for w in want)) > 20
    del calls[:]
    worker.tta, as_probs[0] = 4, True
    got = worker.infer_stack(stack)
    assert calls == list(range(T))
    for t in range(T):
        assert np.array_equal(got[t], want[t]), f"frame {t}: {(got[t] != want[t]).sum()} px differ"


def _smooth_stack(T, H, W, seed):
    """smooth frames: an untrained network maps blobs to blobs"""
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = []
    for t in range(T):
        cell, _ = synth.synth_prediction_maps(rng, H, W, 6 + t, rmin=5.0, rmax=11.0)
        frames.append(np.clip(cell * 50000 + rng.normal(0, 800, cell.shape), 0, 65535).astype(np.uint16))
    return np.stack(frames)


def test_masks_without_a_hook_are_the_postprocessing_of_the_merged_prediction(tmp_path, dev):
    from microbeseg_amd.inference import postprocessing as pp
    worker = _worker(tmp_path, "DU", "bn")
    worker.tta = 4
    T, H, W = 3, 100, 130                                       # padded, and a group of one frame (frame_batch = 1)
    stack = _smooth_stack(T, H, W, seed=10)
    border, cell = worker.predict_merged(stack[:1])
    # an untrained network predicts no distance maps: thresholds from the distribution of its own output
    b = torch.tan(border[0].clamp(0, 1) ** 2)
    b = torch.where(b < 0.05, torch.zeros_like(b), b).clamp(0, 1)
    worker.ths = [float(torch.quantile(cell[0].flatten(), 0.85)), float(torch.quantile((cell[0] - b).flatten(), 0.96))]
    got = worker.infer_stack(stack)
    total = 0
    for t in range(T):
        border, cell = worker.predict_merged(stack[t:t + 1])
        labels, _, _ = pp.distance_postprocessing_device(border[0].contiguous(), cell[0].contiguous(),
                                                         th_seed=worker.ths[1], th_cell=worker.ths[0], col_major_ids=True)
        want = labels.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[t], want), f"frame {t}: {(got[t] != want).sum()} px differ"
        total += int(want.max())
    print("instances in the stack:", total, "thresholds (cell, seed):", worker.ths)
    assert total > 0
    # a float32 copy of the stack (normalised on the host) gives the same masks
    assert np.array_equal(worker.infer_stack(stack.astype(np.float32)), got)
    # inference() on one padded frame is infer_stack on that frame
    worker.tta = 2
    f = stack[1]
    padded, pads = worker.pad_frame(np.copy(f), np.min(f))
    assert pads[0] > 0 and pads[1] > 0
    one = worker.inference(padded, np.min(f), np.max(f), pads)
    assert one.shape == (H, W) and one.dtype == np.uint16
    assert np.array_equal(one, worker.infer_stack(stack[1:2])[0])


def test_masks_without_a_hook_boundary_model(tmp_path, dev):
    from microbeseg_amd.inference import postprocessing as pp
    worker = _worker(tmp_path, "U", "bn")
    worker.tta = 4
    stack = _smooth_stack(2, 100, 130, seed=11)
    got = worker.infer_stack(stack)
    for t in range(2):
        probs = worker.predict_merged(stack[t:t + 1])
        labels, _, _ = pp.boundary_postprocessing_device(probs[0].contiguous())
        assert np.array_equal(got[t], labels.cpu().numpy().view(np.uint16)), f"frame {t}"


# ---- 6. chunking -------------------------------------------------------------------------------------------------------------
def test_members_of_a_group_are_forwarded_in_chunks(tmp_path, dev, monkeypatch):
    from microbeseg_amd.inference import infer
    worker = _worker(tmp_path, "DU", "bn")
    worker.tta = 4
    T, H, W = 3, 128, 128
    stack = _smooth_stack(T, H, W, seed=12)
    calls = _count_net_calls(worker)
    ref = [h.copy() for h in _heads(worker.predict_merged(stack[:1]))]
    assert calls == [4]
    hook, hook_calls = _distance_hook(T, H, W, dev, seed=3)
    worker.prediction_hook = hook
    want = worker.infer_stack(stack)
    worker.prediction_hook = None
    monkeypatch.setattr(infer, "FRAME_BATCH_PIXELS", 3 * H * W)          # m = 3 members per forward
    del calls[:]
    got = _heads(worker.predict_merged(stack[:1]))
    assert calls == [3, 1], calls
    for g, r in zip(got, ref):
        err, bound = float(np.abs(g - r).max()), 1e-4 * max(1.0, float(np.abs(r).max()))
        print(f"chunked vs un-chunked: max abs difference {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    del hook_calls[:]
    worker.prediction_hook = hook
    assert np.array_equal(worker.infer_stack(stack), want) and hook_calls == list(range(T))
    assert int(want.max()) > 3


def test_members_that_do_not_fit_in_memory(tmp_path, dev):
    """a chunk whose forward runs out of memory is halved down to what fits and the masks stay the same; a frame with a
    member that does not fit alone gets the zero mask and no hook call, like the routes without TTA"""
    worker = _worker(tmp_path, "DU", "bn")
    worker.tta, worker.frame_batch = 4, 2                       # 8 members per forward, groups of 2 frames
    T, H, W = 4, 128, 128
    rng = np.random.Generator(np.random.PCG64(14))
    stack = rng.integers(0, 60000, size=(T, H, W)).astype(np.uint16)
    hook, calls = _distance_hook(T, H, W, dev, seed=7)
    worker.prediction_hook = hook
    want = worker.infer_stack(stack)
    assert calls == list(range(T)) and int(want.max()) > 5
    forward, asked, limit = worker.net.forward, [], [3]

    def short_of_memory(x):
        asked.append(int(x.shape[0]))
        if x.shape[0] > limit[0]:
            raise RuntimeError("HIP out of memory. Tried to allocate 1.00 GiB")
        return forward(x)
    worker.net.forward = short_of_memory
    del calls[:]
    got = worker.infer_stack(stack)
    assert asked == [8, 4, 2, 2, 2, 2] * 2, asked
    assert calls == list(range(T)) and np.array_equal(got, want)
    limit[0] = 0
    del calls[:], asked[:]
    got = worker.infer_stack(stack[:2])
    assert asked == [8, 4, 2, 1] + [1] * 7 and not calls and not got.any()


# ---- 7. equivariance ---------------------------------------------------------------------------------------------------------
def test_merged_prediction_commutes_with_the_transforms(tmp_path, dev):
    """predict_merged(T_g f) and T_g(predict_merged(f)) sum the same eight member predictions in different orders, so per
    element |difference| <= 2 gamma (sum_m |p_m|) / 8 + 4 e_pos with gamma = 7u / (1 - 7u), u = 2^-24 (the error of
    either ordered sum of eight against the exact one); e_pos, measured here on the existing forward alone, is the
    largest difference between predictions of the same eight images forwarded in two batch orders.  Control: with
    tta = 1 the same difference must be at least 100 x that bound — a seeded random network is far from equivariant."""
    worker = _worker(tmp_path, "DU", "bn")
    rng = np.random.Generator(np.random.PCG64(77))
    H = W = 64
    f = _smooth_stack(1, H, W, seed=13)[0] // 2 + rng.integers(0, 20000, size=(H, W)).astype(np.uint16)
    images = np.stack([tta_ref.transform(f, c) for c in range(8)])
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    p_a = _heads(worker.forward_frames(images))
    p_b = _heads(worker.forward_frames(images[order]))
    e_pos = max(float(np.abs(b - a[order]).max()) for a, b in zip(p_a, p_b))
    u = 2.0 ** -24
    gamma = 7 * u / (1 - 7 * u)
    # sum_m |p_m| per pixel of f: the members mapped back
    mag = [sum(np.abs(tta_ref.transform(a[c, 0], tta_ref.inverse(c))).astype(np.float64) for c in range(8)) for a in p_a]

    def both_sides(g):
        lhs = [h[0] for h in _heads(worker.predict_merged(tta_ref.transform(f, g)[None]))]
        rhs = [tta_ref.transform(h[0], g) for h in _heads(worker.predict_merged(f[None]))]
        return lhs, rhs

    worst, worst_bound, control = 0.0, 0.0, []
    for g in (1, 3, 6):
        worker.tta = 8
        lhs, rhs = both_sides(g)
        for h in range(2):
            diff = np.abs(lhs[h].astype(np.float64) - rhs[h].astype(np.float64))
            bound = 2 * gamma * tta_ref.transform(mag[h], g) / 8 + 4 * e_pos
            worst, worst_bound = max(worst, float(diff.max())), max(worst_bound, float(bound.max()))
            assert (diff <= bound).all(), f"code {g}, head {h}: {float((diff - bound).max()):.3e} over the bound"
        worker.tta = 1
        lhs, rhs = both_sides(g)
        control.append(max(float(np.abs(lhs[h] - rhs[h]).max()) for h in range(2)))
    print(f"equivariance: e_pos {e_pos:.3e}, tta = 8 max |difference| {worst:.3e} (largest bound {worst_bound:.3e}), "
          f"tta = 1 max |difference| per code {control}")
    assert min(control) >= 100 * worst_bound, (control, worst_bound)


# ---- 8. tta = 1 is untouched -------------------------------------------------------------------------------------------------
def test_tta_1_never_reaches_the_new_entry_points(tmp_path, dev, monkeypatch):
    from microbeseg_amd import _lib
    worker = _worker(tmp_path, "DU", "bn")
    lib = _lib.load()

    def boom(*a, **k):
        raise AssertionError("a tta entry point was reached")
    monkeypatch.setattr(lib, "mseg_tta_expand", boom, raising=False)
    monkeypatch.setattr(lib, "mseg_tta_merge", boom, raising=False)
    rng = np.random.Generator(np.random.PCG64(13))
    stack = rng.integers(0, 60000, size=(3, 100, 130)).astype(np.uint16)
    assert worker.tta == 1
    worker.infer_stack(stack)
    worker.frame_batch = 8
    worker.infer_stack(stack)
    worker.forward_frames(stack)
    f = stack[0]
    padded, pads = worker.pad_frame(np.copy(f), np.min(f))
    worker.inference(padded, np.min(f), np.max(f), pads)
    # tiled inference and TTA do not go together: refused before anything is launched
    worker.sliding_window, worker.tta, worker.frame_batch = True, 2, 1
    for call in (lambda: worker.infer_stack(stack), lambda: worker.predict_merged(stack),
                 lambda: worker.inference(padded, np.min(f), np.max(f), pads)):
        with pytest.raises(RuntimeError, match="sliding_window"):
            call()
    worker.sliding_window, worker.tta = False, 3
    with pytest.raises(ValueError):
        worker.infer_stack(stack)
