"""CPU: the host side of the library-exact CLAHE — the numpy restatement (tests/clahe_ref.py) reproduces scikit-image's
output on every fixture of tests/golden/clahe_library.npz (written by tools/gen_golden_clahe.py with scikit-image 0.18.3),
the C ABI declares the entry points and the ctypes table carries them, the random decisions of the augmentation are
what they were, and the new switches exist with their defaults."""
import pathlib
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from clahe_ref import clahe_ref, clip_histogram

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "clahe_library.npz"
NEW = {"mseg_clahe_workspace_bytes": 3, "mseg_clahe_u16": 11}
CASES = {"c1_32x32_u16": ((32, 32), np.uint16), "c2_40x56_u16": ((40, 56), np.uint16),
         "c3_67x93_u16": ((67, 93), np.uint16), "c4_100x130_u16_blobs": ((100, 130), np.uint16),
         "c5_64x64_u8": ((64, 64), np.uint8), "c6_32x32_u16_const": ((32, 32), np.uint16),
         "c7_256x256_u16": ((256, 256), np.uint16), "c8_16x24_u16": ((16, 24), np.uint16)}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_file_holds_the_cases_and_the_library_version(golden):
    assert sorted(golden["names"].tolist()) == sorted(CASES)
    assert str(golden["skimage_version"]) == "0.18.3"
    for name, (shape, dtype) in CASES.items():
        assert golden["in_" + name].shape == shape and golden["in_" + name].dtype == dtype, name
        assert golden["out_" + name].shape == shape and golden["out_" + name].dtype == np.uint16, name
    assert GOLDEN.stat().st_size < 1 << 20
    assert (golden["in_c6_32x32_u16_const"] == 500).all() and (golden["out_c6_32x32_u16_const"] == 2047).all()
    blobs = golden["in_c4_100x130_u16_blobs"]
    assert np.median(blobs) <= 502 and blobs.max() > 3000          # a nearly flat background with a few cells


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_library(golden, name):
    got, want = clahe_ref(golden["in_" + name]), golden["out_" + name]
    assert got.dtype == np.uint16
    assert np.array_equal(got, want), f"{name}: {(got != want).sum()} px differ"


def test_fixtures_enter_the_leftover_loop(golden):
    """the library's leftover redistribution (the part that differs from the textbook) must be exercised: count the tiles
    of a fixture whose first clipping pass leaves an excess"""
    from clahe_ref import BIN, NBINS, reflect, stretch
    img = golden["in_c3_67x93_u16"]
    g = stretch(img)
    H, W = img.shape
    ky, kx = H // 8, W // 8
    clim = int(max(0.01 * ky * kx, 1))
    entered = 0
    for i in range(-(-H // ky)):
        for j in range(-(-W // kx)):
            rows, cols = reflect(np.arange(i * ky, (i + 1) * ky), H), reflect(np.arange(j * kx, (j + 1) * kx), W)
            h = np.bincount((g[np.ix_(rows, cols)] // BIN).ravel(), minlength=NBINS)
            first = np.minimum(h, clim)
            excess = int((h - first).sum())
            incr = excess // NBINS
            low = first < clim - incr
            after = np.where(low, first + incr, first)
            mid = (after >= clim - incr) & (after < clim)
            excess += -incr * int(low.sum()) + int((after[mid] - clim).sum())
            entered += excess > 0
            assert sum(clip_histogram(h, clim)) <= ky * kx + NBINS
    assert entered >= 40, entered


def test_header_and_ctypes_table_carry_the_entry_points():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    for name, nargs in NEW.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/mseg_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"#define\s+MSEG_PIX_F32\s+3\b", header) and _lib.PIX_F32 == 3
    assert "clahe.hip" in (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()


def test_draw_parameters_is_untouched():
    """same generators consumed in the same order: a seeded draw gives what it gave before the CLAHE keyword existed"""
    from microbeseg_amd.training.device_augment import draw_parameters
    p = draw_parameters(12, random.Random(5), np.random.RandomState(5))
    assert sorted(p) == ["blur_sigma", "contrast", "flip", "noise_frac", "rot_apply", "rot_deg", "scale_apply", "scale_xy"]
    assert p["flip"].tolist() == [5, 3, 3, 2, 3, 0, 7, 0, 7, 1, 4, 7]
    assert p["contrast"][:, 0].tolist() == [0, 0, 3, 3, 2, 0, 0, 0, 1, 2, 0, 3]
    assert p["scale_apply"].tolist() == [0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1]
    assert p["rot_apply"].tolist() == [0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 1]
    assert np.allclose(p["blur_sigma"][:4], [0.0, 1.543761, 1.797147, 1.961478], atol=1e-6) and not p["blur_sigma"][4:].any()
    assert np.allclose(p["noise_frac"], [.04, 0, .05, 0, .03, 0, .04, .02, 0, 0, 0, .04], atol=1e-7)
    assert (p["contrast"][p["contrast"][:, 0] == 3] == (3, 0, 0, 0)).all()


def test_device_augment_clahe_keyword():
    from microbeseg_amd.training.device_augment import DeviceAugment
    assert DeviceAugment("distance", 0, 65535, seed=1).clahe == "zuiderveld"        # the default stays the old operation
    assert DeviceAugment("distance", 0, 65535, seed=1, clahe="library").clahe == "library"
    with pytest.raises(ValueError, match="clahe"):
        DeviceAugment("distance", 0, 65535, seed=1, clahe="skimage")


def test_worker_defaults():
    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.training.train import TrainWorker
    assert InferWorker.apply_clahe is False
    assert TrainWorker.augment_clahe == "zuiderveld"


def test_float_images_are_rejected_before_the_device_is_touched():
    from microbeseg_amd.utils.clahe import equalize_adapthist_device
    import torch
    with pytest.raises(ValueError, match="uint8 or uint16"):
        equalize_adapthist_device(np.zeros((16, 16), np.float32))
    with pytest.raises(ValueError, match="uint8 or uint16"):
        equalize_adapthist_device(torch.zeros((16, 16), dtype=torch.float32))


def test_dataset_transform_refuses_a_worker_process(monkeypatch):
    import torch.utils.data
    from microbeseg_amd.inference.inference_dataset import ContrastEnhancement
    sample = {"image": np.zeros((16, 16), np.uint16), "id": "img_000"}
    assert ContrastEnhancement(False)(sample) is sample
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="num_workers=0"):
        ContrastEnhancement(True)(sample)


@pytest.mark.parametrize("script,flag", [("infer_script_local.py", "--clahe"), ("train_script.py", "--augment_clahe")])
def test_scripts_list_the_flags(script, flag):
    r = subprocess.run([sys.executable, str(ROOT / script), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert flag in r.stdout
