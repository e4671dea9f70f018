"""CPU: the host side of inference at a chosen resolution (--scale) — the axis tables of
microbeseg_amd/inference/resample.py against torch's CPU float64 ``interpolate(mode='bilinear', align_corners=False,
antialias=True)`` and against the restatement tests/resample_ref.py, their invariants, ``out_size``, the validation of
``scale`` and the C ABI table."""
import pathlib
import re

import numpy as np
import pytest
import torch

import resample_ref

ROOT = pathlib.Path(__file__).resolve().parents[1]
SHAPES = [(37, 53), (70, 131), (1, 5), (16, 257)]
FACTORS = [0.25, 0.3, 0.5, 0.73, 1.6, 3.1, 4]
NEW = {"mseg_resample_frames": 10, "mseg_resample_planes": 15}


def _pairs():
    """(source shape, destination shape): every shape at every factor, and the way back"""
    for h, w in SHAPES:
        for s in FACTORS:
            small = (resample_ref.out_size(h, s), resample_ref.out_size(w, s))
            yield (h, w), small
            yield small, (h, w)


def _apply(table, n_in, planes, axis):
    return np.moveaxis(np.tensordot(resample_ref.table_matrix(*table, n_in), planes, axes=([1], [axis])), 0, axis)


def test_tables_applied_in_float64_equal_torch_antialiased_bilinear():
    from microbeseg_amd.inference import resample as R
    rng = np.random.Generator(np.random.PCG64(5))
    worst = 0.0
    for (h, w), (ho, wo) in _pairs():
        a = rng.uniform(-1, 1, size=(h, w))
        want = torch.nn.functional.interpolate(torch.from_numpy(a)[None, None], size=(ho, wo), mode="bilinear",
                                               align_corners=False, antialias=True)[0, 0].numpy()
        got = _apply(R.axis_table(w, wo, dtype=np.float64), w, a, 1)
        got = _apply(R.axis_table(h, ho, dtype=np.float64), h, got, 0)
        assert got.shape == want.shape == (ho, wo)
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        assert err <= 1e-12, f"{(h, w)} -> {(ho, wo)}: {err:.3e}"
        ref = resample_ref.resample(a, ho, wo, fp32_weights=False)          # the restatement states the same rule
        assert float(np.abs(ref - want).max()) <= 1e-12
    print(f"largest difference to torch float64: {worst:.3e}")


def test_table_invariants():
    from microbeseg_amd.inference import resample as R
    widest = 0
    for (h, w), (ho, wo) in _pairs():
        for n_in, n_out in ((h, ho), (w, wo)):
            first, count, weight = R.axis_table(n_in, n_out)
            assert first.dtype == np.int32 and count.dtype == np.int32 and weight.dtype == np.float32
            assert first.shape == count.shape == (n_out,) and weight.shape[0] == n_out
            taps = weight.shape[1]
            widest = max(widest, taps)
            assert taps == int(count.max()) and int(count.min()) >= 1 and taps <= 12 == R.MAX_TAPS
            assert (first >= 0).all() and (first + count <= n_in).all()
            assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()
            assert np.abs(weight.astype(np.float64).sum(axis=1) - 1).max() <= 1e-6
            for i in range(n_out):
                assert not weight[i, count[i]:].any()
            # the fp32 table is the float64 table, rounded; and it is the restatement's matrix
            w64 = R.axis_table(n_in, n_out, dtype=np.float64)[2]
            assert np.array_equal(weight, w64.astype(np.float32))
            assert np.array_equal(resample_ref.table_matrix(first, count, weight, n_in),
                                  resample_ref.axis_matrix(n_in, n_out))
    print("widest window:", widest)


@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_equal_sizes_give_the_identity_table(n):
    from microbeseg_amd.inference import resample as R
    first, count, weight = R.axis_table(n, n)
    assert np.array_equal(resample_ref.table_matrix(first, count, weight, n), np.eye(n))
    assert (count <= 2).all()


def test_out_size():
    from microbeseg_amd.inference import resample as R
    hand = {(37, 0.5): 19, (1, 0.25): 1, (53, 0.5): 27, (70, 0.73): 51, (131, 0.25): 33, (2048, 0.5): 1024, (256, 2): 512,
            (3, 0.25): 1, (5, 0.3): 2, (2048, 4): 8192, (64, 1.0): 64, (257, 3.1): 797}
    for (n, s), want in hand.items():
        assert R.out_size(n, s) == want == resample_ref.out_size(n, s), (n, s)


def test_scale_validation():
    from microbeseg_amd.inference import resample as R
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.scale == 1.0
    for good in (0.25, 0.5, 1, 1.0, 2, 4, 4.0, np.float32(0.75)):
        assert R.check_scale(good) == float(good)
    for bad in (0.2, 4.5, True, False, float("nan"), 0, -1, float("inf"), "0.5", None):
        with pytest.raises(ValueError):
            R.check_scale(bad)


def test_worker_refuses_bad_scales_and_combinations_before_anything_runs():
    """no model, no GPU: the checks come first"""
    from microbeseg_amd.inference.infer import InferWorker
    stack = np.zeros((1, 16, 16), np.uint16)
    for bad in (0.2, 4.5, True, float("nan")):
        worker = InferWorker(model=None, device="cpu")
        worker.scale = bad
        with pytest.raises(ValueError):
            worker.infer_stack(stack)
        with pytest.raises(ValueError):
            worker.predict_scaled(stack)
        with pytest.raises(ValueError):
            worker.inference(stack[0], 0, 1, [0, 0])
    worker = InferWorker(model=None, device="cpu")
    worker.scale = 0.5
    with pytest.raises(RuntimeError, match="GPU"):
        worker.infer_stack(stack)
    worker.tta = 4
    with pytest.raises(RuntimeError, match="tta"):
        worker.infer_stack(stack)
    worker.tta, worker.sliding_window = 1, True
    with pytest.raises(RuntimeError, match="sliding_window"):
        worker.infer_stack(stack)


def test_too_many_taps_are_refused_by_the_wrapper():
    from microbeseg_amd.inference import resample as R
    assert R.axis_table(100, 10)[2].shape[1] > R.MAX_TAPS
    with pytest.raises(RuntimeError, match="taps"):
        R.Axis(100, 10, "cpu")


def test_header_ctypes_table_and_build_script_carry_the_entry_points():
    import ctypes as C
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/mseg_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    build = (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()
    assert "resample.hip" in build and (ROOT / "microbeseg_amd" / "csrc" / "resample.hip").is_file()
    assert C.sizeof(_lib.MsegResampleAxis) == 56
    decl = re.search(r"typedef struct MsegResampleAxis \{(.*?)\} MsegResampleAxis;", header, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", decl))
    assert names == [f[0] for f in _lib.MsegResampleAxis._fields_], names
    # bad tables are refused on the host, before anything could be launched (no GPU is touched)
    lib = _lib.load()
    first, count = np.zeros(4, np.int32), np.ones(4, np.int32)
    ok = _lib.MsegResampleAxis(8, 8, 8, first.ctypes.data, count.ctypes.data, 4, 4, 1, 0)
    for n_in, n_out, taps in ((4, 4, 13), (4, 0, 1), (0, 4, 1), (4, 4, 0)):
        bad = _lib.MsegResampleAxis(8, 8, 8, first.ctypes.data, count.ctypes.data, n_in, n_out, taps, 0)
        assert lib.mseg_resample_frames(8, _lib.PIX_F32, 1, None, C.byref(bad), C.byref(ok), 0, 0, 8, None) == -1
        assert lib.mseg_resample_planes(8, 16, 16, 4, 1, 1, 1, C.byref(ok), C.byref(bad), 8, 16, 16, 4, 1, None) == -1
    past = np.array([0, 1, 2, 4], np.int32)                         # the last window would pass n_in = 4
    bad = _lib.MsegResampleAxis(8, 8, 8, past.ctypes.data, count.ctypes.data, 4, 4, 1, 0)
    assert lib.mseg_resample_planes(8, 16, 16, 4, 1, 1, 1, C.byref(bad), C.byref(ok), 8, 16, 16, 4, 1, None) == -1
    assert lib.mseg_resample_frames(8, _lib.PIX_I32, 1, None, C.byref(ok), C.byref(ok), 0, 0, 8, None) == -1
