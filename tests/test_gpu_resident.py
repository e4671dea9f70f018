"""GPU: the device-resident training set — ``mseg_set_gather`` bit for bit against numpy (every conversion pair, aligned and
odd crop sizes, repeats, N > n, N == 0, offsets past 2^31), the host's index guard, ``ResidentSet.batch`` against the
collated ``TrainingDataset`` items, and seeded ``TrainWorker`` runs that must write the same model on either route."""
import json
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np_of(t):
    return t.cpu().numpy()


# ---- kernel ---------------------------------------------------------------------------------------------------------------
def _pairs():
    from microbeseg_amd import _lib
    from microbeseg_amd.utils.utils import min_max_normalization
    return {
        "u16_raw": (np.uint16, _lib.GATHER_RAW, torch.uint16, lambda a: a),
        "u16_norm": (np.uint16, _lib.GATHER_NORM, torch.float32, lambda a: min_max_normalization(a, 100, 50000)),
        "f32_raw": (np.float32, _lib.GATHER_RAW, torch.float32, lambda a: a),
        "u8_i64": (np.uint8, _lib.GATHER_I64, torch.int64, lambda a: a.astype(np.int64)),
        "u8_f32": (np.uint8, _lib.GATHER_F32, torch.float32, lambda a: a.astype(np.float32)),
    }


def _plane(rng, dtype, shape):
    if dtype == np.float32:
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)


def _index_lists(n):
    """N = 0, 1, 5 and 9 (repeats, N > n); the lists of 5 and 9 hold both 0 and n - 1, N = 1 takes each end once"""
    return [[], [0], [n - 1], [n - 1, 2, 0, 2, 1], [0, n - 1, 3, 3, 1, n - 1, 0, 2, 4]]


@pytest.mark.parametrize("pair", ["u16_raw", "u16_norm", "f32_raw", "u8_i64", "u8_f32"])
@pytest.mark.parametrize("n,h,w", [(7, 16, 16), (5, 17, 19)])
def test_gather_equals_numpy(pair, n, h, w):
    _need_gpu()
    from microbeseg_amd.training.resident_set import set_gather
    src_dtype, mode, out_dtype, ref = _pairs()[pair]
    rng = np.random.Generator(np.random.PCG64(n * 100 + h))
    plane = _plane(rng, src_dtype, (n, h, w))
    dev = torch.from_numpy(plane).to(DEV)
    for indices in _index_lists(n):
        idx = torch.tensor(indices, dtype=torch.int32, device=DEV)
        got = set_gather(dev, idx, mode, 100, 50000)
        torch.cuda.synchronize()
        assert got.dtype == out_dtype and tuple(got.shape) == (len(indices), h, w)
        want = ref(plane[np.asarray(indices, dtype=np.int64)])
        assert _np_of(got).tobytes() == np.ascontiguousarray(want).tobytes(), (pair, indices)
    assert np.array_equal(_np_of(dev), plane)                       # the plane itself is only read


@pytest.mark.parametrize("lo,hi", [(0, 65535), (1000, 60000)])
def test_gather_normalises_every_uint16_value_like_the_host(lo, hi):
    _need_gpu()
    from microbeseg_amd import _lib
    from microbeseg_amd.training.resident_set import set_gather
    from microbeseg_amd.utils.utils import min_max_normalization
    crop = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    got = set_gather(torch.from_numpy(crop).to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV), _lib.GATHER_NORM, lo, hi)
    want = min_max_normalization(crop, min_value=lo, max_value=hi)
    assert want.dtype == np.float32
    assert np.array_equal(_np_of(got).view(np.uint32), want.view(np.uint32))


def test_gather_refuses_other_pairs_and_accepts_an_empty_batch():
    _need_gpu()
    from microbeseg_amd import _lib
    lib = _lib.load()
    src = torch.zeros((2, 4, 4), dtype=torch.float32, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    dst = torch.zeros((1, 4, 4), dtype=torch.int64, device=DEV)

    def call(src_dtype, mode, N=1, lo=0.0, hi=1.0):
        return lib.mseg_set_gather(src.data_ptr(), src_dtype, 2, 16, idx.data_ptr(), N, dst.data_ptr(), mode, lo, hi, None)
    allowed = {(_lib.PIX_U16, _lib.GATHER_RAW), (_lib.PIX_U16, _lib.GATHER_NORM), (_lib.PIX_F32, _lib.GATHER_RAW),
               (_lib.PIX_U8, _lib.GATHER_I64), (_lib.PIX_U8, _lib.GATHER_F32)}
    for src_dtype in (_lib.PIX_U8, _lib.PIX_U16, _lib.PIX_I32, _lib.PIX_F32, 9):
        for mode in (_lib.GATHER_RAW, _lib.GATHER_F32, _lib.GATHER_NORM, _lib.GATHER_I64, 7):
            if (src_dtype, mode) not in allowed:
                assert call(src_dtype, mode) == -1, (src_dtype, mode)
    assert call(_lib.PIX_U16, _lib.GATHER_NORM, lo=5.0, hi=5.0) == -1
    assert call(_lib.PIX_F32, _lib.GATHER_RAW, N=-1) == -1
    assert call(_lib.PIX_F32, _lib.GATHER_RAW, N=0) == 0
    assert lib.mseg_set_gather(None, _lib.PIX_F32, 2, 16, None, 0, None, _lib.GATHER_RAW, 0.0, 1.0, None) == 0
    torch.cuda.synchronize()
    assert int(dst.abs().sum()) == 0


def test_gather_offsets_are_64_bit():
    """a uint8 plane of 2^23 + 3 crops of 16 x 16 = 2 GiB + 768 B: the last three crops start past 2^31 bytes"""
    _need_gpu()
    from microbeseg_amd import _lib
    from microbeseg_amd.training.resident_set import set_gather
    n = 2 ** 23 + 3
    plane = torch.empty((n, 16, 16), dtype=torch.uint8, device=DEV)
    rng = np.random.Generator(np.random.PCG64(8))
    rows = [0, n - 3, n - 2, n - 1]
    crops = rng.integers(0, 256, size=(4, 16, 16)).astype(np.uint8)
    for r, c in zip(rows, crops):
        plane[r] = torch.from_numpy(c).to(DEV)
    got = set_gather(plane, torch.tensor(rows, dtype=torch.int32, device=DEV), _lib.GATHER_I64)
    assert np.array_equal(_np_of(got), crops.astype(np.int64))
    del plane
    torch.cuda.empty_cache()


# ---- ResidentSet against the loader route's batches ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_set(tmp_path_factory):
    from microbeseg_amd.utils import synth
    return synth.write_training_set(tmp_path_factory.mktemp("resident") / "set", 10, 4, size=64, seed=31)


def _resident(data, label_type, raw_train=True, **kw):
    from microbeseg_amd.training import resident_set as R
    return R.ResidentSet(R.load_host(data, label_type), label_type, torch.device(DEV), 0, 65535, raw_train=raw_train, **kw)


def _datasets(data, label_type, augmentation=True):
    from microbeseg_amd.training.training_dataset import TrainingDataset, augmentors
    t = augmentors(label_type=label_type, min_value=0, max_value=65535, device_augmentation=augmentation)
    return {x: TrainingDataset(root_dir=data, label_type=label_type, mode=x, transform=t[x]) for x in ("train", "val")}


def test_index_guard_raises_before_any_launch(small_set):
    _need_gpu()
    from microbeseg_amd.training import resident_set as R
    launches = []

    def counting(*a):
        launches.append(a)
        return R.set_gather(*a)
    rset = _resident(small_set, "distance", gather=counting)
    for split, n in (("train", 10), ("val", 4)):
        with pytest.raises(IndexError):
            rset.batch(split, [0, n], split == "train")
        with pytest.raises(IndexError):
            rset.batch(split, [-1], split == "train")
    assert launches == []
    rset.batch("val", [3], False)
    assert len(launches) == 3


@pytest.mark.parametrize("label_type", ["distance", "boundary"])
def test_batch_equals_the_collated_dataset_items(small_set, label_type):
    _need_gpu()
    from torch.utils.data import default_collate
    from microbeseg_amd.training.train import _Feeder
    datasets = _datasets(small_set, label_type)
    rset = _resident(small_set, label_type)
    feeder = _Feeder(label_type, torch.device(DEV), datasets["train"].transform)
    assert feeder.augment is not None
    lists = {"train": [[0, 1, 2, 3], [9, 4, 4, 0], [8, 9], [5]], "val": [[0, 1, 2, 3], [3, 0], [2]]}
    for split, training in (("train", True), ("val", False)):
        for indices in lists[split]:
            want = default_collate([datasets[split][i] for i in indices])
            got = rset.batch(split, indices, training)
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                assert tuple(g.shape) == tuple(w.shape) and g.device.type == "cuda"
                raw_img = training and k == 0
                raw_label = training and label_type == "boundary" and k == 1
                if raw_img:                     # DeviceAugment takes the 16-bit image as it is
                    assert g.dtype == torch.uint16 and w.dtype == torch.int32
                    assert np.array_equal(_np_of(g).astype(np.int32), w.numpy())
                elif raw_label:                 # ... and an fp32 label plane (exact: values 0, 1, 2)
                    assert g.dtype == torch.float32 and w.dtype == torch.int64
                    assert np.array_equal(_np_of(g).astype(np.int64), w.numpy())
                else:
                    assert g.dtype == w.dtype
                    assert _np_of(g).tobytes() == w.numpy().tobytes()
            fed = []
            for samples in (want, got):
                random.seed(3)
                np.random.seed(3)
                feeder.augment._seed = 77
                fed.append(feeder(samples, training))
            (img_a, labels_a), (img_b, labels_b) = fed
            assert img_a.dtype == img_b.dtype == torch.float32 and torch.equal(img_a, img_b)
            assert len(labels_a) == len(labels_b)
            for a, b in zip(labels_a, labels_b):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_batch_without_augmentation_is_normalised_in_both_phases(small_set):
    _need_gpu()
    from torch.utils.data import default_collate
    datasets = _datasets(small_set, "boundary", augmentation=False)
    rset = _resident(small_set, "boundary", raw_train=False)
    want = default_collate([datasets["train"][i] for i in (7, 0, 7)])
    got = rset.batch("train", [7, 0, 7], True)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and _np_of(g).tobytes() == w.numpy().tobytes()


# ---- seeded runs: the same model on either route --------------------------------------------------------------------------------
def _run(data, models, label_type, optimizer, augment, max_epochs, resident, max_bytes=None):
    from microbeseg_amd.training.train import TrainWorker
    models.mkdir()
    torch.manual_seed(3)
    np.random.seed(3)
    random.seed(3)
    w = TrainWorker()
    w.num_workers = 0
    w.augment = augment
    w.resident = resident
    if max_bytes is not None:
        w.resident_max_bytes = max_bytes
    msgs = []
    w.text_output.connect(msgs.append)
    w.start_training(data, models, label_type, 1, optimizer, 4, torch.device(DEV), 1, False, filters=[8, 16],
                     max_epochs=max_epochs)
    assert w._resident_state is None
    run = f"{label_type}_model_01"
    return dict(msgs=msgs, loss=(models / f"{run}_loss.txt").read_text(), cfg=json.load(open(models / f"{run}.json")),
                sd=torch.load(models / f"{run}.pth", map_location="cpu"))


def _assert_same_model(a, b):
    print("loader route:\n" + a["loss"] + "\nother route:\n" + b["loss"])
    assert a["loss"] == b["loss"]
    assert list(a["sd"]) == list(b["sd"])
    for k in a["sd"]:
        assert torch.equal(a["sd"][k], b["sd"][k]), k


@pytest.mark.parametrize("label_type,optimizer,augment,max_epochs", [
    ("distance", "adam", True, 3), ("boundary", "adam", True, 3), ("distance", "ranger", False, 4)])
def test_resident_run_writes_the_loader_runs_model(small_set, tmp_path, label_type, optimizer, augment, max_epochs):
    """10 train crops at batch 4: the last train batch of every epoch is partial"""
    _need_gpu()
    loader = _run(small_set, tmp_path / "loader", label_type, optimizer, augment, max_epochs, resident=False)
    resident = _run(small_set, tmp_path / "resident", label_type, optimizer, augment, max_epochs, resident=True)
    assert "data_route" not in loader["cfg"] and resident["cfg"]["data_route"] == "resident"
    assert not any(m.startswith("Resident training set not used") for m in loader["msgs"] + resident["msgs"])
    assert len(loader["loss"].splitlines()) >= 1 + min(max_epochs, 3)
    _assert_same_model(loader, resident)


def test_over_budget_falls_back_to_the_loader_route(small_set, tmp_path):
    _need_gpu()
    loader = _run(small_set, tmp_path / "loader", "distance", "adam", True, 2, resident=False)
    fallback = _run(small_set, tmp_path / "fallback", "distance", "adam", True, 2, resident=True, max_bytes=1)
    said = [m for m in fallback["msgs"] if m.startswith("Resident training set not used")]
    assert len(said) == 1 and "budget" in said[0]
    assert "data_route" not in fallback["cfg"] and fallback["cfg"]["trained_epochs"] == 2
    _assert_same_model(loader, fallback)
