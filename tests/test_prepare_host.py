"""CPU: the host side of the training-set preparation (microbeseg_amd/utils/data_cropping.py, data_import.py) — crop
origins against the fixture and the numpy restatement, the import's padding / border / grid arithmetic, its skip rules,
split draws and file naming (the device calls replaced by the restatement), and the new symbols of the C ABI."""
import json
import pathlib
import random
import re

import numpy as np
import pytest
import torch

import prepare_ref as R
from helpers import load_npz

ROOT = pathlib.Path(__file__).resolve().parents[1]
S = 64


@pytest.fixture(scope="module")
def crops_fx():
    return load_npz("prepare_crops.npz")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_propose_origins_equals_fixture_and_restatement(crops_fx, seed):
    from microbeseg_amd.utils.data_cropping import propose_origins
    assert [tuple(s) for s in crops_fx["shapes"]] == R.SHAPES
    skipped = []
    for i, shape in enumerate(R.SHAPES):
        got = propose_origins(shape, S, random.Random(seed))
        want = crops_fx[f"origins_s{seed}_{i}"]
        ref = R.origins_ref(np.ones(shape, np.uint8), S, random.Random(seed))
        if got is None:
            skipped.append(shape)
            assert ref is None and len(want) == 0
            continue
        assert ref is not None and got == ref[1], (shape, got, ref[1])
        assert np.array_equal(np.asarray(got, np.int32).reshape(-1, 2), want), (shape, got, want.tolist())
        ph, pw = max(shape[0], S), max(shape[1], S)
        assert all(0 <= a <= ph - S and 0 <= b <= pw - S for a, b in got)
    assert skipped == [(50, 50)]


def test_propose_origins_branches_and_draw_order():
    from microbeseg_amd.utils.data_cropping import propose_origins

    class Recorder(random.Random):
        def __init__(self):
            super().__init__(4)
            self.calls = []

        def randint(self, a, b):
            self.calls.append((a, b))
            return super().randint(a, b)
    n = {shape: len(propose_origins(shape, S, random.Random(1)) or []) for shape in R.SHAPES}
    assert n == {(60, 75): 1, (64, 64): 1, (60, 60): 1, (75, 225): 3, (225, 75): 3, (140, 100): 2, (60, 200): 3,
                 (193, 64): 3, (64, 193): 3, (58, 300): 3, (50, 50): 0}
    assert propose_origins((64, 64), S, None) == [(0, 0)] and propose_origins((60, 60), S, None) == [(0, 0)]
    assert propose_origins((200, 60), S, None) == [(0, 0)] * 3        # padded in x: no draw at all, three equal crops
    rec = Recorder()
    propose_origins((75, 225), S, rec)                                 # row first, then the column of segment i
    assert rec.calls == [(0, 11), (0, 11), (0, 11), (75, 86), (0, 11), (150, 161)]
    rec = Recorder()
    propose_origins((225, 75), S, rec)
    assert rec.calls == [(0, 11), (0, 11), (75, 86), (0, 11), (150, 161), (0, 11)]
    rec = Recorder()
    propose_origins((193, 64), S, rec)                                 # degenerate ranges: randint(i * 64, i * 64)
    assert rec.calls == [(0, 0), (0, 0), (64, 64), (0, 0), (128, 128), (0, 0)]
    rec = Recorder()
    propose_origins((60, 75), S, rec)                                  # padded in y alone still draws (the reference's
    assert rec.calls == [(0, 0), (0, 11)]                              # condition tests x_pads twice)
    rec = Recorder()
    propose_origins((58, 300), S, rec)
    assert rec.calls == [(0, 0), (0, 36), (0, 0), (100, 136), (0, 0), (200, 236)]


def test_stats_from_exact_sums():
    from microbeseg_amd.utils.data_cropping import stats_from_sums
    rng = np.random.Generator(np.random.PCG64(3))
    a = rng.integers(0, 65536, size=(211, 97)).astype(np.uint16)
    v = [int(x) for x in a.ravel()]
    mean, std = stats_from_sums(min(v), max(v), sum(v), sum(x * x for x in v), len(v))
    assert abs(mean - np.mean(a)) <= 1e-12 * np.mean(a) and abs(std - np.std(a)) <= 1e-12 * np.std(a)
    n = 2048 * 2048                                                     # sum of squares beyond 2^53
    assert stats_from_sums(65535, 65535, 65535 * n, 65535 * 65535 * n, n) == (65535.0, 0.0)


@pytest.mark.parametrize("h", [64, 65, 128, 135, 150, 191])
@pytest.mark.parametrize("w", [64, 70, 139, 203])
def test_import_grid_equals_the_reference_slicing(h, w):
    """odd and even remainders on both axes: floor(border) rows go at the top, one more at the bottom when odd"""
    from microbeseg_amd.utils.data_import import import_grid
    img = np.arange(h * w, dtype=np.int64).reshape(h, w)
    yy, xx = np.mgrid[:h, :w]
    mask = (1 + (yy // 16) * 100 + xx // 16).astype(np.uint16)       # many small cells: no crop is rejected
    ref = R.import_ref(img, mask, S, False)
    grid = import_grid((h, w), S)
    if h == 64 and w == 64:
        assert grid is None and len(ref["crops"]) == 1
        return
    ny, nx, y0, x0 = grid
    assert (ny, nx) == (h // S, w // S) and y0 == (h - ny * S) // 2 and x0 == (w - nx * S) // 2
    assert y0 + ny * S <= h and x0 + nx * S <= w
    assert len(ref["crops"]) == ny * nx
    for k, (img_crop, _, x_start, y_start) in enumerate(ref["crops"]):
        hh, ww = divmod(k, nx)
        assert (x_start, y_start) == (x0 + ww * S, y0 + hh * S)
        assert np.array_equal(img_crop, img[y_start:y_start + S, x_start:x_start + S])


def test_centred_pads_and_too_much_pads():
    from microbeseg_amd.utils.data_import import centred_pads
    assert centred_pads((64, 64), S) == ((0, 0), (0, 0)) and centred_pads((300, 70), S) == ((0, 0), (0, 0))
    assert centred_pads((50, 59), S) == ((7, 7), (3, 2))               # the odd pixel goes to the left
    assert centred_pads((32, 64), S) == ((16, 16), (0, 0))              # pads == size is still allowed
    assert centred_pads((31, 64), S) is None and centred_pads((64, 20), S) is None
    for shape in ((50, 59), (33, 64), (64, 47)):
        img = np.ones(shape, np.uint8)
        ref = R.import_ref(img, img, S, False)["crops"][0][0]
        assert np.array_equal(np.pad(img, centred_pads(shape, S), mode='constant'), ref)
    assert R.import_ref(np.ones((20, 64), np.uint8), np.ones((20, 64), np.uint8), S, False) is None


def test_rejection_rule_and_split():
    from microbeseg_amd.utils.data_import import accept_crop, split_of
    assert not accept_crop(0, 0, 0, 0)                                  # no division for a region without cells
    assert not accept_crop(0, 0, 4, 400) and not accept_crop(1, 99, 4, 400)
    assert accept_crop(1, 100, 4, 400) and accept_crop(2, 101, 4, 401)
    assert [split_of(r, 0.2, 0.1) for r in (0.0, 0.099, 0.1, 0.299, 0.31, 0.99)] == ['test', 'test', 'val', 'val', 'train',
                                                                                    'train']


def _host_backend(monkeypatch):
    """the device calls of data_import.py replaced by the numpy restatement (CPU tensors in the same storage)"""
    from microbeseg_amd.utils import data_import as D
    from oracle import contour_ref

    def views(t):
        a = t.numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a

    def stats(raw):
        v = views(raw).astype(object)
        return int(v.min()), int(v.max()), int(v.sum()), int((v * v).sum())

    def extract(raw, np_dtype, origins, crop_size, pad_value, lo, hi, want=()):
        padded = R.pad_to_crop(views(raw), crop_size, pad_value)
        img, _, _, u16 = R.crop_views(padded, origins, crop_size, lo, hi)
        out = {"raw": torch.from_numpy(np.ascontiguousarray(img).view(np.int16) if img.dtype == np.uint16
                                       else np.ascontiguousarray(img)),
               "u16": torch.from_numpy(u16.view(np.int16))}
        return {k: out[k] for k in want}

    def census(mask, np_dtype, y0, x0, ny, nx, crop_size):
        return R.census_ref(views(mask), y0, x0, ny, nx, crop_size)

    def round_trip(mask_crops):
        m = views(mask_crops)
        return m.astype(np.uint16), [sum(len(p) for p in contour_ref.label_polygons(c).values()) for c in m]
    monkeypatch.setattr(D, "frame_stats_device", stats)
    monkeypatch.setattr(D, "extract_crops_device", extract)
    monkeypatch.setattr(D, "crop_census_device", census)
    monkeypatch.setattr(D, "round_trip_masks", round_trip)
    return D


def test_import_skips_split_draws_and_naming_across_two_runs(tmp_path, monkeypatch):
    from microbeseg_amd.utils import tiffio
    D = _host_backend(monkeypatch)
    fx = load_npz("prepare_import.npz")
    src = tmp_path / "annotated"
    src.mkdir()
    names = ["A", "D", "E", "B", "C", "F"]
    for n in names:
        tiffio.imwrite(str(src / f"img_{n}.tif"), fx[f"img_{n}"])
        tiffio.imwrite(str(src / f"mask_{n}.tif"), fx[f"mask_{n}"])
    tiffio.imwrite(str(src / "img_nomask.tif"), fx["img_F"])
    (src / "img_notes.txt").write_text("not an image")
    ids = [src / f"img_{n}.tif" for n in names] + [src / "img_nomask.tif", src / "img_notes.txt"]
    said = []
    out = tmp_path / "set"
    records = D.DataImportWorker().import_local(ids, False, S, out, 0.5, 0.3, 0.2, rng=random.Random(7), raw_masks=True,
                                                text_output=said.append, device="cpu")
    assert any("img_D.tif: too much pads needed --> skip" in s for s in said)
    assert any("img_E.tif: empty mask --> skip" in s for s in said)
    assert any("img_nomask.tif: No mask found" in s for s in said)
    # one draw per image that reaches the split (A, B, C, F), none for the skipped ones, in that order
    rng = random.Random(7)
    sets = {n: D.split_of(rng.random(), 0.3, 0.2) for n in ("A", "B", "C", "F")}
    counts = {n: len(fx[f"offsets_{n}"]) for n in ("A", "B", "C", "F")}
    assert [r["image"] for r in records] == [f"ext_img_{n}.tif" for n in ("A", "B", "C", "F") for _ in range(counts[n])]
    assert [r["set"] for r in records] == [sets[n] for n in ("A", "B", "C", "F") for _ in range(counts[n])]
    total = sum(counts.values())
    assert [r["file"] for r in records] == ["img_ext{:03d}.tif".format(k) for k in range(total)]
    k = 0
    for n in ("A", "B", "C", "F"):
        stats = fx[f"stats_{n}"]
        for j in range(counts[n]):
            r = records[k]
            assert (int(r["x_start"]), int(r["y_start"])) == tuple(fx[f"offsets_{n}"][j])
            assert (r["min_frame"], r["max_frame"]) == (stats[0], stats[1])
            assert abs(float(r["mean_frame"]) - float(stats[2])) <= 1e-12 * float(stats[2])
            assert abs(float(r["std_frame"]) - float(stats[3])) <= 1e-12 * float(stats[3])
            assert r["crop_size"] == "64" and r["pre_labeled"] == "False" and r["dataset"] == "annotated"
            img = tiffio.imread(str(out / r["set"] / r["file"]))
            assert img.dtype == np.uint16 and np.array_equal(img, fx[f"u16_{n}"][j])
            mask = tiffio.imread(str(out / r["set"] / r["file"].replace("img_", "mask_")))
            assert np.array_equal(mask, fx[f"rawmask_{n}"][j]) and mask.dtype == fx[f"rawmask_{n}"].dtype
            k += 1
    assert json.load(open(out / "split_info.json")) == {"used": [], "num_ext": total}
    # a second run continues the numbering and the records
    again = D.DataImportWorker().import_local([src / "img_C.tif"], True, S, out, 1.0, 0.0, 0.0, rng=random.Random(1),
                                              text_output=said.append, device="cpu")
    assert [r["file"] for r in again] == ["img_ext{:03d}.tif".format(total)] and again[0]["set"] == "train"
    assert (again[0]["min_frame"], again[0]["max_frame"]) == ("0", "65535")
    assert np.array_equal(tiffio.imread(str(out / "train" / again[0]["file"])), fx["u16_C_keep"][0])
    assert json.load(open(out / "split_info.json"))["num_ext"] == total + 1
    assert len(json.load(open(out / "import_info.json"))) == total + 1


def test_omero_routes_raise_and_shims_export_the_reference_names():
    from src.utils.data_cropping import DataCropWorker
    from src.utils.data_import import DataImportWorker
    worker = DataCropWorker([], 64, 1, None, "u", "p", "h", "4064", None)
    for call in (worker.connect, worker.next_crop, worker.get_crop):
        with pytest.raises(RuntimeError, match="OMERO"):
            call()
    with pytest.raises(RuntimeError, match="OMERO"):
        DataImportWorker().import_data([], False, 64, 1, None, "u", "p", "h", "4064", None, 0.8, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="model"):
        worker.inference(np.zeros((64, 64), np.uint16), 0, 1)


def test_new_symbols_are_declared_and_bound():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    declared = set(re.findall(r"\b(mseg_[a-z0-9_]+)\s*\(", header))
    new = {"mseg_frame_stats", "mseg_crops_extract", "mseg_crop_census", "mseg_crop_census_workspace_bytes",
           "mseg_crops_overlay"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.mseg_crop_census_workspace_bytes() == 8192
    # argument validation happens before any GPU work
    assert lib.mseg_frame_stats(None, 0, 10, None, None) == -1
    assert lib.mseg_crops_extract(None, 0, 1, 1, 1, None, 1, 0, 0, 1, None, None, None, None, None) == -1
    assert lib.mseg_crop_census(None, 0, 1, 1, 0, 0, 1, 1, 1, None, None, None, 0, None) == -1
    assert lib.mseg_crops_overlay(None, None, None, 1, 1, None) == -1
