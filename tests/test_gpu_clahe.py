"""GPU (MI355X): the library-exact CLAHE (csrc/clahe.hip, utils/clahe.py) against scikit-image's own output
(tests/golden/clahe_library.npz) and the numpy restatement (tests/clahe_ref.py), through every surface that uses it: the
batched call, the data-set transform, the training augmentation and the inference worker.  Tolerance zero everywhere:
every step is integer arithmetic or a correctly rounded IEEE operation in a fixed order."""
import json
import pathlib

import numpy as np
import pytest
import torch

from clahe_ref import clahe_ref

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "clahe_library.npz"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _textured(rng, h, w, lo=200, hi=20000):
    """gradient + blobs + noise: different histograms in every tile"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = lo + (hi - lo) * (0.3 + 0.2 * np.sin(x / (0.2 * w + 1)) * np.cos(y / (0.15 * h + 1)))
    for _ in range(5):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1.5, 0.1 * min(h, w) + 2)
        img += 0.5 * (hi - lo) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    img += rng.normal(0, 0.02 * (hi - lo), (h, w))
    return np.clip(img, 0, 65535).astype(np.uint16)


# ---- 1: the library's own output ---------------------------------------------------------------------------------------------
def test_every_fixture_bit_for_bit(dev, golden):
    from microbeseg_amd.utils.clahe import equalize_adapthist_device
    names = golden["names"].tolist()
    assert len(names) == 8
    for name in names:
        img, want = golden["in_" + name], golden["out_" + name]
        got = equalize_adapthist_device(img)
        assert got.dtype == torch.uint16 and got.shape == img.shape and got.is_cuda
        got = _u16(got)
        diff = got != want
        print(f"{name}: {int(diff.sum())} px differ" + (f", max |d| {np.abs(got.astype(int) - want)[diff].max()}, first at "
                                                        f"{tuple(np.argwhere(diff)[0])}" if diff.any() else ""))
        assert np.array_equal(got, want), name
    # a device tensor (int16 storage of uint16 bits) and a stack go the same way
    img = golden["in_c2_40x56_u16"]
    t = torch.from_numpy(np.stack([img, img[::-1].copy()]).view(np.int16)).to(dev)
    got = _u16(equalize_adapthist_device(t))
    assert np.array_equal(got[0], golden["out_c2_40x56_u16"]) and np.array_equal(got[1], clahe_ref(img[::-1].copy()))


# ---- 2: batch and flags ------------------------------------------------------------------------------------------------------
def test_batch_with_apply_flags_f32_and_u16(dev):
    from microbeseg_amd.utils.clahe import clahe_device
    rng = np.random.default_rng(21)
    imgs = np.stack([_textured(rng, 40, 56, hi=3000 + 9000 * i) for i in range(5)])
    flags = [1, 0, 1, 1, 0]
    apply = torch.tensor(flags, dtype=torch.int32, device=dev)
    want = [clahe_ref(im) for im in imgs]
    src = torch.from_numpy(imgs.astype(np.float32)).to(dev)
    keep = src.clone()
    got = clahe_device(src, apply=apply, out_dtype=torch.float32)
    assert got.dtype == torch.float32 and torch.equal(src, keep)
    got = got.cpu().numpy()
    got16 = _u16(clahe_device(torch.from_numpy(imgs.view(np.int16)).to(dev), apply=apply))
    for i, on in enumerate(flags):
        expect = want[i] if on else imgs[i]
        assert np.array_equal(got[i], expect.astype(np.float32)), f"image {i} (fp32 route)"
        assert np.array_equal(got16[i], expect), f"image {i} (uint16 route)"
    # without flags every image is enhanced
    got_all = _u16(clahe_device(torch.from_numpy(imgs.view(np.int16)).to(dev)))
    for i in range(5):
        assert np.array_equal(got_all[i], want[i]), f"image {i} (no flags)"


# ---- 3: shapes without a fixture -------------------------------------------------------------------------------------------------
def _two_valued(rng):
    return np.where(rng.random((48, 48)) < 0.3, 40000, 1200).astype(np.uint16)


@pytest.mark.parametrize("name,make", [
    ("8x8 (tile 1x1)", lambda rng: rng.integers(0, 65536, (8, 8)).astype(np.uint16)),
    ("24x200", lambda rng: _textured(rng, 24, 200)),
    ("264x264 (clim 10)", lambda rng: _textured(rng, 264, 264, hi=50000)),
    ("267x270 (clim 10, s % k != 0)", lambda rng: _textured(rng, 267, 270, hi=50000)),
    ("two-valued 48x48", _two_valued),
])
def test_shapes_without_a_fixture(dev, name, make):
    """264 x 264 has tiles of 33 x 33 (clim = 10) but is a multiple of its tile (264 = 8 * 33); 267 x 270 keeps that tile
    and clim and adds the end padding up to the next tile multiple (267 % 33 = 3, 270 % 33 = 6), nine tiles per axis."""
    from microbeseg_amd.utils.clahe import equalize_adapthist_device
    img = make(np.random.default_rng(5))
    if name.startswith("26"):
        h, w = img.shape
        assert int(0.01 * (h // 8) * (w // 8)) == 10 and (h % (h // 8) != 0) == name.startswith("267")
    got, want = _u16(equalize_adapthist_device(img)), clahe_ref(img)
    print(f"{name}: {int((got != want).sum())} px differ")
    assert np.array_equal(got, want), name


# ---- 4: the data-set transform ---------------------------------------------------------------------------------------------------
def test_dataset_transform(dev, golden, tmp_path):
    from microbeseg_amd.inference.inference_dataset import InferenceDataset, pre_processing_transforms
    from microbeseg_amd.utils import tiffio
    img, enhanced = golden["in_c3_67x93_u16"], golden["out_c3_67x93_u16"]
    tiffio.imwrite(str(tmp_path / "img_000.tif"), img)
    data = InferenceDataset(tmp_path, transform=pre_processing_transforms(apply_clahe=True, scale_factor=1))
    assert len(data) == 1
    got, got_id, got_pads, got_size = data[0]
    want, _, want_pads, want_size = pre_processing_transforms(apply_clahe=False)({"image": enhanced, "id": "img_000"})
    assert got_id == "img_000" and list(got_pads) == list(want_pads) and tuple(got_size) == tuple(want_size) == (67, 93)
    assert got.dtype == torch.float32 and got.shape == want.shape and got.shape[0] == 1
    assert torch.equal(got, want)


# ---- 5: the augmentation ---------------------------------------------------------------------------------------------------------
def _aug_params(n):
    return dict(flip=np.zeros(n, np.int32), contrast=np.zeros((n, 4), np.float32), scale_apply=np.zeros(n, np.int32),
                scale_xy=np.ones((n, 2), np.float32), rot_apply=np.zeros(n, np.int32), rot_deg=np.zeros(n, np.float32),
                blur_sigma=np.zeros(n, np.float32), noise_frac=np.zeros(n, np.float32))


def _norm(v, lo=0.0, hi=65535.0):
    return 2 * (np.clip(v, lo, hi) - lo) / (hi - lo) - 1


def test_augmentation_library_mode_and_unchanged_default(dev):
    from microbeseg_amd import _lib
    from microbeseg_amd.training.device_augment import DeviceAugment
    rng = np.random.default_rng(9)
    imgs = np.stack([_textured(rng, 48, 48, hi=8000 + 20000 * i) for i in range(3)])
    p = _aug_params(3)
    p["contrast"][:, 0] = [3, 0, 3]
    t = torch.from_numpy(imgs.view(np.int16)).to(dev)
    out, _ = DeviceAugment("distance", 0, 65535, seed=7, clahe="library").apply(t, [], p)
    out = out.cpu().numpy()[:, 0]
    for i in (0, 2):
        want = _norm(clahe_ref(imgs[i]).astype(np.float32)).astype(np.float32)
        assert np.array_equal(out[i], want), f"image {i}: {(out[i] != want).sum()} px differ"
    assert np.array_equal(out[1], _norm(imgs[1].astype(np.float32)).astype(np.float32))
    # the default keyword is the operation the augmentation had so far: mseg_aug_clahe on the same planes
    old, _ = DeviceAugment("distance", 0, 65535, seed=7).apply(t, [], p)
    lib = _lib.load()
    src = torch.from_numpy(imgs.astype(np.float32)).to(dev)
    dst = torch.empty_like(src)
    ws = torch.empty(lib.mseg_aug_clahe_workspace_bytes(3), dtype=torch.uint8, device=dev)
    choice = torch.from_numpy(p["contrast"]).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mseg_aug_clahe(src.data_ptr(), dst.data_ptr(), 3, 48, 48, choice.data_ptr(), ws.data_ptr(), st) == 0
    want_old = _norm(dst.cpu().numpy()).astype(np.float32)
    assert np.array_equal(old.cpu().numpy()[:, 0], want_old)
    assert not np.array_equal(want_old[0], out[0])                # and it is a different computation


# ---- 6: the inference worker -----------------------------------------------------------------------------------------------------
def _worker(tmp_path):
    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.utils.unets import build_unet
    torch.manual_seed(5)
    net = build_unet("DU", "relu", "conv", "bn", torch.device("cuda:0"), 1, ch_out=1, filters=(8, 16))
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    base = tmp_path / "distance_model_00"
    torch.save(net.state_dict(), str(base) + ".pth")
    with open(str(base) + ".json", "w") as f:
        json.dump({"architecture": ["DU", "conv", "relu", "bn", [8, 16]], "label_type": "distance"}, f)
    return InferWorker(model=str(base), device="cuda:0", ths=(0.10, 0.45))


def _record_inputs(worker):
    """what the network is handed, per call: the raw uint16 frame (frame by frame) or the normalised group"""
    seen = []

    def hook(_module, inp):
        x = inp[0]
        raw = getattr(x, "raw", None)
        seen.append(_u16(raw).copy() if raw is not None else x.detach().cpu().numpy().copy())
    worker.net.register_forward_pre_hook(hook)
    return seen


def test_inference_worker(dev, tmp_path):
    worker = _worker(tmp_path)
    said = []
    worker.text_output.connect(said.append)
    rng = np.random.default_rng(33)
    stack = np.stack([_textured(rng, 96, 80, hi=6000 + 15000 * i) for i in range(3)])
    enhanced = np.stack([clahe_ref(f) for f in stack])
    seen = _record_inputs(worker)
    assert worker.apply_clahe is False and worker.frame_batch == 1
    plain = worker.infer_stack(stack)
    plain_in = [a for a in seen]
    assert len(plain_in) == 3 and all(np.array_equal(a, f) for a, f in zip(plain_in, stack))
    del seen[:]
    want = worker.infer_stack(enhanced)                       # the stack enhanced beforehand, no CLAHE in the worker
    want_in = [a for a in seen]
    assert all(np.array_equal(a, f) for a, f in zip(want_in, enhanced))
    for batch in (1, 3):
        worker.frame_batch = batch
        worker.apply_clahe = False
        del seen[:]
        want_b = worker.infer_stack(enhanced)
        want_b_in = [a for a in seen]
        assert np.array_equal(want_b, want)
        worker.apply_clahe = True
        del seen[:]
        got = worker.infer_stack(stack)
        assert len(seen) == len(want_b_in) == (3 if batch == 1 else 1)
        for a, b in zip(seen, want_b_in):                     # the network saw exactly the pre-enhanced frames
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"frame_batch {batch}"
        assert got.dtype == np.uint16 and np.array_equal(got, want), f"frame_batch {batch}"
        worker.apply_clahe = False
        assert np.array_equal(worker.infer_stack(stack), plain), f"frame_batch {batch}: the default changed"
    # sliding-window inference: the whole frame is enhanced before it is tiled
    worker.frame_batch = 1
    worker.sliding_window = True
    want_sw = worker.infer_stack(enhanced)
    worker.apply_clahe = True
    assert np.array_equal(worker.infer_stack(stack), want_sw)
    worker.sliding_window = False
    # float frames: segmented as they are, with a message
    assert not said
    got_f = worker.infer_stack(stack.astype(np.float32))
    assert len(said) == 1 and "Skip CLAHE" in said[0] and "float32" in said[0]
    assert np.array_equal(got_f, plain)


# ---- 7: bad arguments ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(dev):
    from microbeseg_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    src = torch.full((1, 16, 16), 7, dtype=torch.int16, device=dev)
    dst = torch.full((1, 16, 16), -5, dtype=torch.int16, device=dev)
    nbytes = lib.mseg_clahe_workspace_bytes(1, 16, 16)
    assert nbytes > 0 and lib.mseg_clahe_workspace_bytes(1, 7, 16) == 0 and lib.mseg_clahe_workspace_bytes(0, 16, 16) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(in_ptr, in_dt, h, w, out_ptr, out_dt, ws_bytes=nbytes):
        return lib.mseg_clahe_u16(in_ptr, in_dt, 1, h, w, None, out_ptr, out_dt, ws.data_ptr(), ws_bytes, st)
    einval, ews = -1, -3
    assert call(src.data_ptr(), _lib.PIX_U16, 7, 16, dst.data_ptr(), _lib.PIX_U16) == einval          # H = 7
    assert call(src.data_ptr(), _lib.PIX_U16, 16, 7, dst.data_ptr(), _lib.PIX_U16) == einval
    assert call(src.data_ptr(), _lib.PIX_U16, 16, 16, src.data_ptr(), _lib.PIX_U16) == einval         # in == out
    assert call(src.data_ptr(), _lib.PIX_I32, 16, 16, dst.data_ptr(), _lib.PIX_U16) == einval         # bad input dtype
    assert call(src.data_ptr(), _lib.PIX_U16, 16, 16, dst.data_ptr(), _lib.PIX_U8) == einval          # bad output dtype
    assert call(src.data_ptr(), _lib.PIX_U16, 16, 16, dst.data_ptr(), _lib.PIX_U16, nbytes - 1) == ews
    torch.cuda.synchronize()
    assert (dst == -5).all() and (src == 7).all()                                                     # nothing ran
    assert call(src.data_ptr(), _lib.PIX_U16, 16, 16, dst.data_ptr(), _lib.PIX_U16) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_u16(dst)[0], clahe_ref(np.full((16, 16), 7, np.uint16)))   # the same call, now legal, does run
