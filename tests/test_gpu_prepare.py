"""GPU (MI355X): training-set preparation on the device (csrc/prepare.hip, utils/data_cropping.py, utils/data_import.py,
prepare_script.py) — the four kernels against Python-int / numpy results and the fixtures of tools/gen_golden_prepare.py
(numpy restatement of the reference loops + scikit-image), the import and the crop route end to end, pre-labelling against
the CPU oracles, and the CLI."""
import json
import pathlib
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import prepare_ref as R
from helpers import load_npz

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
S = 64
DTYPES = [np.uint8, np.uint16]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def crops_fx():
    return load_npz("prepare_crops.npz")


@pytest.fixture(scope="module")
def import_fx():
    return load_npz("prepare_import.npz")


def _up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _frame(crops_fx, i, dtype):
    f = crops_fx[f"frame_{i}"]
    return f if dtype == np.uint16 else (f >> 8).astype(np.uint8)


# ---- 1. mseg_frame_stats ----------------------------------------------------------------------------------------------------
def _exact(a):
    v = a.astype(object)
    return int(v.min()), int(v.max()), int(v.sum()), int((v * v).sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_frame_stats_equal_python_int_sums(dev, dtype):
    from microbeseg_amd.utils.data_cropping import frame_stats_device, stats_from_sums
    rng = np.random.Generator(np.random.PCG64(21))
    top = np.iinfo(dtype).max
    frames = [rng.integers(0, top + 1, size=shape).astype(dtype) for shape in ((1, 1), (37, 53), (300, 517))]
    tail = rng.integers(top // 4, top // 2, size=(300, 517)).astype(dtype)      # 155100 = 605 * 256 + 220 pixels: the
    tail.reshape(-1)[-1], tail.reshape(-1)[-3] = top, 0                          # extrema sit in the last partial block
    frames.append(tail)
    for a in frames:
        got = frame_stats_device(_up(a, dev))
        want = _exact(a)
        print(a.shape, np.dtype(dtype).name, got, want)
        assert got == want
        mean, std = stats_from_sums(*got, a.size)
        if a.size > 1:
            em, es = abs(mean - np.mean(a)) / np.mean(a), abs(std - np.std(a)) / np.std(a)
            print("  relative distance to numpy: mean %.3e std %.3e" % (em, es))
            assert em <= 1e-12 and es <= 1e-12
        else:
            assert (mean, std) == (float(a[0, 0]), 0.0)


def test_frame_stats_beyond_2_pow_53_and_argument_checks(dev):
    from microbeseg_amd import _lib
    from microbeseg_amd.utils.data_cropping import frame_stats_device, stats_from_sums
    a = np.full((2048, 2048), 65535, np.uint16)
    got = frame_stats_device(_up(a, dev))
    n = a.size
    assert got == (65535, 65535, 65535 * n, 65535 * 65535 * n) and got[3] > 2 ** 53
    assert stats_from_sums(*got, n) == (65535.0, 0.0)
    lib = _lib.load()
    out = torch.zeros(4, dtype=torch.int64, device=dev)
    raw = _up(a[:2], dev)
    assert lib.mseg_frame_stats(raw.data_ptr(), 1, 2 ** 31, out.data_ptr(), None) == -1
    assert lib.mseg_frame_stats(raw.data_ptr(), 2, 10, out.data_ptr(), None) == -1
    assert lib.mseg_frame_stats(raw.data_ptr(), 1, 0, out.data_ptr(), None) == -1


# ---- 2. mseg_crops_extract --------------------------------------------------------------------------------------------------
def _check_extract(dev, frame, origins, lo, hi, pad):
    from microbeseg_amd.utils.data_cropping import extract_crops_device, _host
    out = extract_crops_device(_up(frame, dev), frame.dtype, origins, S, pad, lo, hi)
    padded = R.pad_to_crop(frame, S, pad)
    img, show, x, u16 = R.crop_views(padded, origins, S, lo, hi)
    assert _host(out["raw"]).dtype == frame.dtype and np.array_equal(_host(out["raw"]), img)
    assert np.array_equal(out["show"].cpu().numpy(), show)
    assert np.array_equal(out["x"].cpu().numpy()[:, 0].view(np.uint32), x.view(np.uint32))
    assert np.array_equal(_host(out["u16"]), u16)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_crops_extract_equals_fixture_and_numpy_formulas(dev, crops_fx, dtype):
    from microbeseg_amd.utils.data_cropping import propose_origins, _host
    tested_k = set()
    for i, shape in enumerate(R.SHAPES):
        frame = _frame(crops_fx, i, dtype)
        lo, hi = np.min(frame), np.max(frame)
        ph, pw = max(shape[0], S), max(shape[1], S)
        for seed in (1, 2, 3):
            origins = propose_origins(shape, S, random.Random(seed)) or [(0, 0)]
            origins = (origins + [(ph - S, pw - S), (0, pw - S)])[:3] if seed == 3 else origins   # last valid positions
            for k in range(1, len(origins) + 1):
                out = _check_extract(dev, frame, origins[:k], lo, hi, lo)
                tested_k.add(k)
            if seed == 1 and dtype == np.uint16 and f"img_{i}" in crops_fx:
                assert np.array_equal(_host(out["raw"]), crops_fx[f"img_{i}"])
                assert np.array_equal(out["show"].cpu().numpy(), crops_fx[f"show_{i}"])
                if f"x_{i}" in crops_fx:
                    assert np.array_equal(out["x"].cpu().numpy()[:, 0].view(np.uint32), crops_fx[f"x_{i}"].view(np.uint32))
        # keep_normalization: the range of the dtype, zero padding
        _check_extract(dev, frame, [(0, 0), (ph - S, pw - S)], 0, int(np.iinfo(dtype).max), 0)
    assert tested_k == {1, 2, 3}


@pytest.mark.parametrize("dtype", DTYPES)
def test_crops_extract_narrow_range_null_outputs_and_constant_frame(dev, dtype):
    from microbeseg_amd import _lib
    from microbeseg_amd.utils.data_cropping import extract_crops_device
    rng = np.random.Generator(np.random.PCG64(4))
    top = int(np.iinfo(dtype).max)
    frame = rng.integers(top // 2, top // 2 + 2, size=(70, 100)).astype(dtype)
    assert int(frame.max()) - int(frame.min()) == 1
    _check_extract(dev, frame, [(3, 5), (6, 36)], np.min(frame), np.max(frame), np.min(frame))
    wide = rng.integers(0, top + 1, size=(60, 100)).astype(dtype)
    wide[0, 0], wide[0, 1] = 0, top
    _check_extract(dev, wide, [(0, 0), (0, 36)], np.min(wide), np.max(wide), np.min(wide))
    # an export range narrower than the data: values clip at both ends of uint16
    out = extract_crops_device(_up(wide, dev), dtype, [(0, 17)], S, 0, top // 4, top // 2, want=("u16",))
    want = R.crop_views(R.pad_to_crop(wide, S, 0), [(0, 17)], S, top // 4, top // 2)[3]
    assert np.array_equal(out["u16"].cpu().numpy().view(np.uint16), want) and want.min() == 0 and want.max() == 65535
    # null outputs are skipped: what is asked for alone equals the full call
    raw = _up(wide, dev)
    full = extract_crops_device(raw, dtype, [(0, 9)], S, 0, 0, top)
    for name in ("raw", "show", "u16", "x"):
        one = extract_crops_device(raw, dtype, [(0, 9)], S, 0, 0, top, want=(name,))
        assert list(one) == [name] and torch.equal(one[name], full[name])
    # hi == lo: MSEG_EINVAL, nothing launched
    lib = _lib.load()
    org = torch.zeros(2, dtype=torch.int32, device=dev)
    show = torch.full((1, S, S), 7, dtype=torch.uint8, device=dev)
    pix = 0 if dtype == np.uint8 else 1
    assert lib.mseg_crops_extract(raw.data_ptr(), pix, 60, 100, 1, org.data_ptr(), S, 0, 5, 5, None, show.data_ptr(), None,
                                  None, None) == -1
    torch.cuda.synchronize()
    assert bool((show == 7).all())


# ---- 3. mseg_crop_census ----------------------------------------------------------------------------------------------------
def test_crop_census_equals_numpy_unique(dev, import_fx):
    from microbeseg_amd.utils.data_import import crop_census_device, import_grid
    rng = np.random.Generator(np.random.PCG64(6))
    many = np.where(rng.random((299, 301)) < 0.6, rng.integers(1, 65536, size=(299, 301)), 0).astype(np.uint16)
    many[21:85, 22:86] = 0                                              # an empty crop
    small = np.where(rng.random((135, 140)) < 0.5, rng.integers(1, 256, size=(135, 140)), 0).astype(np.uint8)
    for mask in (import_fx["mask_A"], import_fx["mask_B"], many, small):
        ny, nx, y0, x0 = import_grid(mask.shape, S)
        assert (mask.shape[0] - ny * S) % 2 == 1 or (mask.shape[1] - nx * S) % 2 == 1
        cells, area = crop_census_device(_up(mask, dev), mask.dtype, y0, x0, ny, nx, S)
        want_cells, want_area = R.census_ref(mask, y0, x0, ny, nx, S)
        print(mask.shape, mask.dtype, cells.tolist(), area.tolist())
        assert np.array_equal(cells, want_cells) and np.array_equal(area, want_area)
    a = import_fx["mask_A"]
    ny, nx, y0, x0 = import_grid(a.shape, S)
    cells, area = crop_census_device(_up(a, dev), a.dtype, y0, x0, ny, nx, S)
    assert cells[-1] < cells[:-1].sum()            # ids span crops: the region's count is not the sum
    assert 0 in cells[:-1].tolist()                # an empty crop
    assert 300 in a and cells[-1] == len(np.unique(a[y0:y0 + ny * S, x0:x0 + nx * S])) - 1   # border-only id not counted
    assert 300 not in a[y0:y0 + ny * S, x0:x0 + nx * S]


def test_crop_census_rejects_a_grid_outside_the_mask(dev):
    from microbeseg_amd import _lib
    lib = _lib.load()
    mask = torch.zeros((130, 130), dtype=torch.int16, device=dev)
    cells = torch.zeros(5, dtype=torch.int32, device=dev)
    area = torch.zeros(5, dtype=torch.int64, device=dev)
    ws = torch.zeros(8192, dtype=torch.uint8, device=dev)
    args = (cells.data_ptr(), area.data_ptr(), ws.data_ptr())
    assert lib.mseg_crop_census(mask.data_ptr(), 1, 130, 130, 3, 2, 2, 2, S, *args, 8192, None) == -1
    assert lib.mseg_crop_census(mask.data_ptr(), 1, 130, 130, -1, 0, 2, 2, S, *args, 8192, None) == -1
    assert lib.mseg_crop_census(mask.data_ptr(), 1, 130, 130, 2, 2, 2, 2, S, *args, 100, None) == -1
    assert lib.mseg_crop_census(mask.data_ptr(), 1, 130, 130, 2, 2, 2, 2, S, *args, 8192, None) == 0
    torch.cuda.synchronize()
    assert cells.tolist() == [0] * 5 and area.tolist() == [0] * 5


# ---- mseg_crops_overlay -----------------------------------------------------------------------------------------------------
def test_crops_overlay_equals_numpy(dev):
    from microbeseg_amd import _lib
    lib = _lib.load()
    rng = np.random.Generator(np.random.PCG64(8))
    show = rng.integers(0, 256, size=(3, 37, 37)).astype(np.uint8)
    outl = rng.random((3, 37, 37)) < 0.2
    rgb = torch.zeros((3, 37, 37, 3), dtype=torch.uint8, device=dev)
    s_d, o_d = torch.from_numpy(show).to(dev), torch.from_numpy(outl.astype(np.uint8) * 3).to(dev)
    assert lib.mseg_crops_overlay(s_d.data_ptr(), o_d.data_ptr(), rgb.data_ptr(), 3, 37, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(rgb.cpu().numpy(), np.stack([R.overlay_ref(show[k], outl[k]) for k in range(3)]))


# ---- 4. import end to end -----------------------------------------------------------------------------------------------------
class _Draws:
    def __init__(self, values):
        self.values = list(values)

    def random(self):
        return self.values.pop(0)


def _write_annotated(import_fx, src, names):
    from microbeseg_amd.utils import tiffio
    src.mkdir()
    for n in names:
        tiffio.imwrite(str(src / f"img_{n}.tif"), import_fx[f"img_{n}"])
        tiffio.imwrite(str(src / f"mask_{n}.tif"), import_fx[f"mask_{n}"])
    return [src / f"img_{n}.tif" for n in names]


def test_import_end_to_end_equals_fixture_and_feeds_training(dev, import_fx, tmp_path):
    from microbeseg_amd.utils import tiffio
    from microbeseg_amd.training.training_dataset import TrainingDataset
    from src.training.train import CreateLabelsWorker
    from src.utils.data_import import DataImportWorker
    names = ["A", "D", "B", "E", "C", "F"]
    ids = _write_annotated(import_fx, tmp_path / "annotated", names)
    kept = ("A", "B", "C", "F")
    sets = dict(zip(kept, ("train", "val", "test", "train")))
    assert sum(len(import_fx[f"offsets_{n}"]) for n in kept) >= 4
    for keep_norm, raw_masks in ((False, False), (True, True)):
        out = tmp_path / f"set_{int(keep_norm)}"
        said = []
        records = DataImportWorker().import_local(ids, keep_norm, S, out, 0.5, 0.3, 0.2, rng=_Draws([0.9, 0.3, 0.1, 0.95]),
                                                  raw_masks=raw_masks, text_output=said.append, device=dev)
        assert sum("too much pads" in s for s in said) == 1 and sum("empty mask" in s for s in said) == 1
        k = 0
        for n in kept:
            tag = f"{n}_keep" if keep_norm else n
            assert len(import_fx[f"offsets_{tag}"]) == len(import_fx[f"offsets_{n}"])
            stats = import_fx[f"stats_{tag}"]
            for j in range(len(import_fx[f"offsets_{n}"])):
                r = records[k]
                assert r["file"] == "img_ext{:03d}.tif".format(k) and r["set"] == sets[n] and r["image"] == f"ext_img_{n}.tif"
                assert (int(r["x_start"]), int(r["y_start"])) == tuple(import_fx[f"offsets_{n}"][j])
                assert (r["min_frame"], r["max_frame"]) == (stats[0], stats[1])
                assert abs(float(r["mean_frame"]) - float(stats[2])) <= 1e-12 * float(stats[2])
                assert abs(float(r["std_frame"]) - float(stats[3])) <= 1e-12 * float(stats[3])
                img = tiffio.imread(str(out / r["set"] / r["file"]))
                assert img.dtype == np.uint16 and np.array_equal(img, import_fx[f"u16_{tag}"][j]), (n, j)
                mask = tiffio.imread(str(out / r["set"] / "mask_ext{:03d}.tif".format(k)))
                want = import_fx[f"rawmask_{n}"][j] if raw_masks else import_fx[f"roundtrip_{n}"][j]
                assert mask.dtype == want.dtype and np.array_equal(mask, want), (n, j, int((mask != want).sum()))
                k += 1
        assert k == len(records)
        assert json.load(open(out / "split_info.json"))["num_ext"] == k
    # the round-trip set goes through label creation and loads in the training data set
    out = tmp_path / "set_0"
    CreateLabelsWorker().create_labels(out, "distance")
    for mode, n in (("train", len(import_fx["offsets_A"]) + 1), ("val", len(import_fx["offsets_B"]))):
        ds = TrainingDataset(root_dir=out, label_type="distance", mode=mode)
        assert len(ds) == n
        sample = ds[0]
        assert sample["image"].shape == (S, S, 1) and sample["image"].dtype == np.uint16
        assert sample["cell_label"].shape == (S, S, 1) and float(sample["cell_label"].max()) > 0


# ---- 5. crop route without a model -------------------------------------------------------------------------------------------
KEYS = {'frame', 'crop_size', 'min_frame', 'max_frame', 'mean_frame', 'std_frame', 'pre_labeled', 'x_start', 'y_start',
        'img', 'img_show', 'roi', 'roi_show'}


def test_crop_route_without_model_equals_fixture(dev, crops_fx):
    from src.utils.data_cropping import crops_local
    said = []
    for i, shape in enumerate(R.SHAPES):
        frame = crops_fx[f"frame_{i}"]
        got = crops_local([frame], S, device=dev, rng=random.Random(1), text_output=said.append)
        want = crops_fx[f"origins_s1_{i}"]
        if len(want) == 0:
            assert got == [] and shape == (50, 50)
            continue
        assert len(got) == 1 and len(got[0]) == len(want)
        stats = crops_fx[f"stats_{i}"]
        for k, d in enumerate(got[0]):
            assert set(d) == KEYS and d['roi'] is None and d['roi_show'] is None
            assert (int(d['y_start']), int(d['x_start'])) == tuple(want[k])
            assert (d['crop_size'], d['pre_labeled'], d['min_frame'], d['max_frame']) == ('64', 'False', stats[0], stats[1])
            assert abs(float(d['mean_frame']) - float(stats[2])) <= 1e-12 * float(stats[2])
            assert abs(float(d['std_frame']) - float(stats[3])) <= 1e-12 * float(stats[3])
            assert d['img'].dtype == np.uint16 and np.array_equal(d['img'], crops_fx[f"img_{i}"][k])
            assert d['img_show'].dtype == np.uint8 and np.array_equal(d['img_show'], crops_fx[f"show_{i}"][k])
    # one rng across frames of different sizes and dtypes; a float frame takes the host formulas; a constant one is skipped
    frames = [crops_fx["frame_3"], (crops_fx["frame_5"] >> 8).astype(np.uint8), crops_fx["frame_0"].astype(np.float32),
              np.full((70, 70), 9, np.uint16), crops_fx["frame_10"]]
    got = crops_local(frames, S, device=dev, rng=random.Random(2), text_output=said.append)
    assert [len(g) for g in got] == [3, 2, 1] and [g[0]['frame'] for g in got] == [0, 1, 2]
    assert any("constant frame" in s for s in said)
    rng = random.Random(2)
    for g, frame in zip(got, frames[:3]):
        padded, origins = R.origins_ref(frame, S, rng)
        img, show, _, _ = R.crop_views(padded, origins, S, np.min(frame), np.max(frame))
        for k, d in enumerate(g):
            assert np.array_equal(d['img'], img[k]) and np.array_equal(d['img_show'], show[k]) and d['img'].dtype == frame.dtype


# ---- 6. pre-labelling ---------------------------------------------------------------------------------------------------------
def _model(tmp_path, unet_type, norm, seed=5):
    from microbeseg_amd.utils.unets import build_unet
    torch.manual_seed(seed)
    label_type = "distance" if unet_type == "DU" else "boundary"
    net = build_unet(unet_type, "relu", "conv", norm, torch.device("cuda:0"), 1, ch_out=1 if unet_type == "DU" else 3,
                     filters=(8, 16))
    if norm == "bn":
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.uniform_(-0.2, 0.2)
                    m.running_var.uniform_(0.5, 1.5)
    base = tmp_path / f"{label_type}_model_{unet_type}_{norm}"
    torch.save(net.state_dict(), str(base) + ".pth")
    with open(str(base) + ".json", "w") as f:
        json.dump({"architecture": [unet_type, "conv", "relu", norm, [8, 16]], "label_type": label_type}, f)
    return base.with_suffix(".json")


def _crop_worker(tmp_path, unet_type="DU", norm="bn", ths=(0.10, 0.45)):
    from src.utils.data_cropping import DataCropWorker
    return DataCropWorker(crop_size=S, pre_labeling=True, model=_model(tmp_path, unet_type, norm), device="cuda:0",
                          ths=list(ths))


def _net_inputs(worker):
    seen = []
    worker.net.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach().clone()))
    return seen


def _fixture_hook(crops_fx, dev):
    """the fixture's synthetic distance maps, crop k gets maps k % 3; counts its calls"""
    border = torch.from_numpy(crops_fx["pl_border"]).to(dev)
    cell = torch.from_numpy(crops_fx["pl_cell"]).to(dev)
    calls = []

    def hook(pred):
        assert pred[0].shape == (1, 1, S, S) and pred[1].shape == (1, 1, S, S)
        k = len(calls) % 3
        calls.append(k)
        return border[k][None, None], cell[k][None, None]
    return hook, calls


def _host_x(frame, origins):
    padded = R.pad_to_crop(frame, S, np.min(frame))
    return R.crop_views(padded, origins, S, np.min(frame), np.max(frame))[2]


@pytest.mark.parametrize("unet_type,norm", [("DU", "bn"), ("DU", "gn"), ("U", "bn")])
def test_prelabel_network_input_and_forward_match_host_formula_and_oracle(dev, crops_fx, tmp_path, unet_type, norm):
    from oracle import unet_ref
    worker = _crop_worker(tmp_path, unet_type, norm)
    seen, preds = _net_inputs(worker), []

    def passthrough(pred):
        preds.append(pred)
        return pred
    worker.prediction_hook = passthrough
    frames = [crops_fx["frame_3"], (crops_fx["frame_5"] >> 8).astype(np.uint8), crops_fx["frame_0"]]
    got = worker.crops_local(frames, rng=random.Random(3))
    assert [len(g) for g in got] == [3, 2, 1] and len(seen) == 1 and tuple(seen[0].shape) == (6, 1, S, S)
    rng = random.Random(3)
    want_x = np.concatenate([_host_x(f, R.origins_ref(f, S, rng)[1]) for f in frames])
    x = seen[0].cpu()
    assert np.array_equal(x.numpy()[:, 0].view(np.uint32), want_x.view(np.uint32))
    sd = {k: v.detach().cpu() for k, v in worker.net.state_dict().items()}
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, x, unet_type, "relu", norm, (8, 16), training=False)
    ref = ref if isinstance(ref, tuple) else (ref,)
    assert len(preds) == 6
    for i, pred in enumerate(preds):
        outs = pred if isinstance(pred, tuple) else (pred,)
        for o, r in zip(outs, ref):
            err = (o[0].cpu() - r[i]).abs().max().item()
            bound = 1e-4 * max(1.0, r[i].abs().max().item())
            print(f"{unet_type}/{norm} crop {i}: max abs err {err:.3e} (bound {bound:.3e})")
            assert err <= bound


def test_prelabel_hooked_equals_oracle_masks_rois_and_skimage_outlines(dev, crops_fx, tmp_path):
    from oracle import postproc_ref
    from microbeseg_amd.inference.infer import InferWorker
    worker = _crop_worker(tmp_path)
    hook, calls = _fixture_hook(crops_fx, dev)
    worker.prediction_hook = hook
    got = worker.crops_local([crops_fx["frame_3"]], rng=random.Random(1))
    assert len(got) == 1 and len(got[0]) == 3 and calls == [0, 1, 2]
    tracer = InferWorker(device="cuda:0")
    for k, d in enumerate(got[0]):
        assert set(d) == KEYS | {'mask'}
        want = postproc_ref.distance_postprocessing(crops_fx["pl_border"][k][..., None], crops_fx["pl_cell"][k][..., None],
                                                    0.45, 0.10)
        assert int(want.max()) >= 5 and np.array_equal(want, crops_fx["pl_mask"][k])
        assert d['mask'].dtype == np.uint16 and np.array_equal(d['mask'], want), int((d['mask'] != want).sum())
        assert d['roi'] == [r['points'] for r in tracer.polygon_rois(want)] == crops_fx[f"pl_rois_{k}"].tolist()
        assert np.array_equal(d['img_show'], crops_fx["show_3"][k])
        assert d['roi_show'].shape == (S, S, 3) and np.array_equal(d['roi_show'], crops_fx["pl_roi_show"][k])
        outlines = (d['roi_show'] == np.array([255, 255, 0], np.uint8)).all(-1)
        assert np.array_equal(outlines & crops_fx["pl_outlines"][k], crops_fx["pl_outlines"][k])
    # DataCropWorker.inference on one crop = that crop's entry
    del calls[:]
    frame = crops_fx["frame_3"]
    one = worker.inference(got[0][0]['img'], np.min(frame), np.max(frame))
    assert one.dtype == np.uint16 and one.shape == (S, S) and np.array_equal(one, got[0][0]['mask'])


def test_prelabel_batches_of_frames_give_identical_dicts(dev, crops_fx, tmp_path):
    worker = _crop_worker(tmp_path)
    rng = np.random.Generator(np.random.PCG64(15))
    frames = [rng.integers(100 * t, 4000 + 7000 * t, size=(75, 225)).astype(np.uint16) for t in range(8)]
    runs = {}
    for batch in (8, 1):
        seen = _net_inputs(worker) if batch == 8 else seen
        del seen[:]
        hook, calls = _fixture_hook(crops_fx, dev)
        worker.prediction_hook = hook
        runs[batch] = worker.crops_local(frames, rng=random.Random(5), batch_frames=batch)
        assert [int(x.shape[0]) for x in seen] == ([24] if batch == 8 else [3] * 8)
        assert len(calls) == 24
    assert len(runs[8]) == len(runs[1]) == 8
    for a, b in zip(runs[8], runs[1]):
        for da, db in zip(a, b):
            assert set(da) == set(db)
            for key in da:
                same = np.array_equal(da[key], db[key]) if isinstance(da[key], np.ndarray) else da[key] == db[key]
                assert same, key
    assert max(int(d['mask'].max()) for g in runs[8] for d in g) >= 5


def test_prelabel_survives_out_of_memory_and_shape_errors(dev, crops_fx, tmp_path):
    worker = _crop_worker(tmp_path)
    rng = np.random.Generator(np.random.PCG64(16))
    frames = [rng.integers(0, 60000, size=(75, 225)).astype(np.uint16) for t in range(8)]
    hook, calls = _fixture_hook(crops_fx, dev)
    worker.prediction_hook = hook
    want = worker.crops_local(frames, rng=random.Random(6), batch_frames=4)
    forward, asked, limit = worker.net.forward, [], [5]

    def short_of_memory(x):
        asked.append(int(x.shape[0]))
        if x.shape[0] > limit[0]:
            raise RuntimeError("HIP out of memory. Tried to allocate 1.00 GiB")
        return forward(x)
    worker.net.forward = short_of_memory
    del calls[:]
    got = worker.crops_local(frames, rng=random.Random(6), batch_frames=4)
    assert asked == [12, 6, 3, 3, 3, 3] + [3] * 4, asked           # later groups start at the size that fitted
    assert len(calls) == 24
    for a, b in zip(got, want):
        for da, db in zip(a, b):
            assert np.array_equal(da['mask'], db['mask']) and da['roi'] == db['roi']
            assert np.array_equal(da['roi_show'], db['roi_show'])
    limit[0] = 0
    said = []
    worker.text_output.connect(said.append)
    del calls[:], asked[:]
    got = worker.crops_local(frames[:1], rng=random.Random(6))
    assert asked == [3, 1, 1, 1] and not calls and len(said) == 3 and "not enough ram/vram" in said[0]
    for d in got[0]:
        assert not d['mask'].any() and d['roi'] == [] and np.array_equal(d['roi_show'][..., 2], d['img_show'])
    # the one-crop surface: out of memory and a crop the network cannot take both give the zero mask and the message
    del said[:]
    assert not worker.inference(frames[0][:64, :64], 0, 60000).any() and len(said) == 1
    worker.net.forward = forward
    del said[:]
    odd = worker.inference(frames[0][:61, :61], 0, 60000)         # 61 is not a multiple of the network's stride
    assert odd.shape == (61, 61) and odd.dtype == np.uint16 and not odd.any() and len(said) == 1


def test_prelabel_without_hook_equals_oracle_of_own_predictions(dev, tmp_path):
    from oracle import postproc_ref
    from microbeseg_amd import engine
    from microbeseg_amd.utils import synth
    worker = _crop_worker(tmp_path)
    rng = np.random.Generator(np.random.PCG64(10))
    frames = []
    for t in range(4):                                      # smooth frames: an untrained network maps blobs to blobs
        cell, _ = synth.synth_prediction_maps(rng, 75, 225, 8 + t, rmin=5.0, rmax=11.0)
        frames.append(np.clip(cell * 50000 + rng.normal(0, 800, cell.shape), 0, 65535).astype(np.uint16))
    seen = _net_inputs(worker)
    worker.crops_local(frames, rng=random.Random(8))        # a first pass for the network's own output range
    with torch.no_grad(), engine.precision_scope("fp32"):
        border, cell = worker.net(seen[0])
    b = torch.tan(border[0, 0].clamp(0, 1) ** 2)
    b = torch.where(b < 0.05, torch.zeros_like(b), b).clamp(0, 1)
    ths = [float(torch.quantile(cell[0, 0].flatten(), 0.85)), float(torch.quantile((cell[0, 0] - b).flatten(), 0.96))]
    del seen[:]
    got = worker.crops_local(frames, ths=ths, rng=random.Random(8))
    assert len(seen) == 1 and seen[0].shape[0] == 12
    with torch.no_grad(), engine.precision_scope("fp32"):
        border, cell = worker.net(seen[0])
    masks = [d['mask'] for g in got for d in g]
    total = 0
    for i, mask in enumerate(masks):
        want = postproc_ref.distance_postprocessing(border[i, 0].cpu().numpy()[..., None], cell[i, 0].cpu().numpy()[..., None],
                                                    ths[1], ths[0])
        assert np.array_equal(mask, want), f"crop {i}: {(mask != want).sum()} px differ"
        total += int(want.max())
    print("instances:", total, "thresholds (cell, seed):", ths)
    assert total > 0


def test_prelabel_boundary_model_equals_oracle_of_its_own_softmax(dev, crops_fx, tmp_path):
    from oracle import postproc_ref
    worker = _crop_worker(tmp_path, "U", "bn")
    logits = []
    for k in range(3):
        cell, border = crops_fx["pl_cell"][k], crops_fx["pl_border"][k]
        p1 = np.clip(cell * 2.0, 0, 1) * (1 - np.clip(border * 1.2, 0, 1))
        p2 = np.clip(border * 1.2, 0, 1) * (cell > 0.02)
        p0 = np.clip(1 - p1 - p2, 0.0, 1)
        probs = np.stack([p0, p1, p2], 0).astype(np.float32)
        probs = probs / probs.sum(0, keepdims=True)
        logits.append(torch.from_numpy(np.log(probs + 1e-6)[None]).to(dev))
    calls = []

    def hook(pred):
        assert pred.shape == (1, 3, S, S)
        calls.append(len(calls) % 3)
        return logits[calls[-1]]
    worker.prediction_hook = hook
    rng = np.random.Generator(np.random.PCG64(17))
    frames = [rng.integers(0, 60000, size=(75, 225)).astype(np.uint16) for t in range(4)]      # 12 crops: floods of 8 + 4
    got = worker.crops_local(frames, rng=random.Random(9))
    assert len(calls) == 12
    want = [postproc_ref.boundary_postprocessing(worker._infer._softmax_hwc(lg, (0, 0)).cpu().numpy()) for lg in logits]
    assert max(int(w.max()) for w in want) >= 3
    for i, d in enumerate(d for g in got for d in g):
        assert np.array_equal(d['mask'], want[i % 3]), i
        assert len(d['roi']) == int(want[i % 3].max())


def test_one_pixel_instance_is_outlined_through_its_vertex(dev, tmp_path):
    from src.utils.data_cropping import DataCropWorker
    worker = DataCropWorker(crop_size=S, device="cuda:0")
    mask = np.zeros((1, S, S), np.uint16)
    mask[0, 10:20, 10:20] = 1
    mask[0, 40, 50] = 2
    mask[0, 63, 0] = 3
    show = np.full((1, S, S), 90, np.uint8)
    rois, rgb = worker._rois_and_overlays(_up(mask, dev), torch.from_numpy(show).to(dev))
    assert rois[0][1:] == ["50,40 ", "0,63 "] and len(rois[0]) == 3
    assert rgb[0, 40, 50].tolist() == [255, 255, 0] and rgb[0, 63, 0].tolist() == [255, 255, 0]
    assert rgb[0, 10, 10].tolist() == [255, 255, 0] and rgb[0, 15, 15].tolist() == [90, 90, 90]
    assert rgb[0, 41, 50].tolist() == [90, 90, 90]


# ---- 7. CLI ---------------------------------------------------------------------------------------------------------------------
def test_prepare_script_crops_and_import(dev, crops_fx, import_fx, tmp_path):
    from microbeseg_amd.utils import tiffio
    model = _model(tmp_path, "DU", "bn")
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    tiffio.imwrite(str(imgs / "movie.tif"), np.stack([crops_fx["frame_3"], crops_fx["frame_3"][::-1], crops_fx["frame_3"],
                                                          crops_fx["frame_3"][:, ::-1]]))      # 2D+t: (T, H, W)
    tiffio.imwrite(str(imgs / "single.tif"), crops_fx["frame_5"])
    out = tmp_path / "crops"
    r = subprocess.run([sys.executable, str(ROOT / "prepare_script.py"), "crops", "-i", str(imgs), "--crop_size", "64", "--out",
                        str(out), "--model", str(model.with_suffix("")), "--step", "2", "--seed", "3"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    records = json.load(open(out / "crops.json"))
    assert len(records) == 3 + 3 + 2 and [rec["image"] for rec in records] == ["movie.tif"] * 6 + ["single.tif"] * 2
    assert [rec["frame"] for rec in records] == ["0"] * 3 + ["2"] * 3 + ["0"] * 2
    for k in range(8):
        assert tiffio.imread(str(out / f"img_{k}.tif")).shape == (S, S)
        assert tiffio.imread(str(out / f"show_{k}.tif")).dtype == np.uint8
        mask = tiffio.imread(str(out / f"mask_{k}.tif"))
        assert mask.dtype == np.uint16 and mask.shape == (S, S)
        assert np.squeeze(tiffio.imread(str(out / f"overlay_{k}.tif"))).shape == (S, S, 3)
        assert len(json.load(open(out / f"rois_{k}.json"))["rois"]) == len(np.unique(mask)) - 1
    ids = _write_annotated(import_fx, tmp_path / "annotated", ["A", "B", "C"])
    trainset = tmp_path / "trainset"
    r = subprocess.run([sys.executable, str(ROOT / "prepare_script.py"), "import", "-i", str(ids[0].parent), "--crop_size", "64",
                        "--out", str(trainset), "--seed", "1", "--keep_normalization"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    info = json.load(open(trainset / "import_info.json"))
    n = sum(len(import_fx[f"offsets_{k}"]) for k in ("A", "B", "C"))
    assert len(info) == n and json.load(open(trainset / "split_info.json"))["num_ext"] == n
    for rec in info:
        assert tiffio.imread(str(trainset / rec["set"] / rec["file"])).dtype == np.uint16
        assert tiffio.imread(str(trainset / rec["set"] / rec["file"].replace("img_", "mask_"))).max() > 0
