"""GPU (MI355X): the device Analysis / Export pipeline (csrc/analysis.hip, mseg_stack_relabel) against the reference's own
outputs (tests/golden/analysis_*.npz) and against the CPU restatement (tests/analysis_ref.py).  Masks, outlines, overlay,
counts, total_area and mean_area exact; axis means rtol 1e-9 / atol 1e-6 px (regionprops uses eigvalsh on float moments)."""
import pathlib
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import analysis_ref as ref
from test_analysis_host import CASES, check_table, load_case

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _coords(rois, H, W):
    return [(r["theT"],) + tuple(np.asarray(v) for v in ref.make_coordinates(r["points"], W, H)) for r in rois]


def _pts(r, c):
    return "".join(f"{x},{y} " for y, x in zip(r, c))


@pytest.mark.parametrize("name", CASES)
def test_device_pipeline_equals_reference(name, tmp_path):
    from microbeseg_amd.inference.analysis import analyze_local, analyze_masks, rois_to_masks
    from microbeseg_amd.inference.result_export import export_local
    from microbeseg_amd.utils import tiffio
    z, rois, T, H, W = load_case(name)
    mask, outl = rois_to_masks(rois, T, H, W)
    msgs = []
    files = export_local(z["img"], rois, tmp_path / "exp", f"{name}.tif", text_output=msgs.append)
    csv = tmp_path / f"{name}_analysis.csv"
    df_local = analyze_local(rois, T, H, W, csv, text_output=msgs.append)
    if "csv" not in z:
        assert mask.max(initial=0) == 0 and files == [] and df_local is None and not csv.exists()
        assert not (tmp_path / "exp").exists()
        assert all("no segmentation results found" in m for m in msgs) and len(msgs) == 2
        return
    assert mask.dtype == z["mask"].dtype and np.array_equal(mask, z["mask"])
    assert np.array_equal(outl, z["outlines"])
    check_table(analyze_masks(mask), str(z["csv"]))
    check_table(pd.read_csv(csv, float_precision="round_trip"), str(z["csv"]))
    assert [f.name for f in files] == [f"{name}{s}" for s in (".tif", "_mask.tif", "_overlay.tif", "_outlines.tif",
                                                                  "_analysis.csv")]
    ov = tiffio.imread(str(files[2]))
    assert ov.dtype == np.uint8 and np.array_equal(ov.reshape(z["overlay"].shape), z["overlay"])
    m2 = tiffio.imread(str(files[1]))
    assert m2.dtype == z["mask"].dtype and np.array_equal(m2.reshape(mask.shape), z["mask"])
    o2 = tiffio.imread(str(files[3]))
    assert o2.dtype == bool and np.array_equal(o2.reshape(outl.shape), z["outlines"])
    check_table(pd.read_csv(files[4], float_precision="round_trip"), str(z["csv"]))


def test_random_small_polygons_incl_degenerate_vs_restatement():
    from microbeseg_amd.inference.analysis import analyze_masks, rois_to_masks
    rng = np.random.default_rng(11)
    T, H, W = 3, 96, 128
    rois = []
    for i in range(2000):
        n = int(rng.integers(1, 10))                 # 1- and 2-point polygons included (the reference raises on them)
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        r = np.clip(cy + rng.integers(-9, 10, n), -3, H + 2)
        c = np.clip(cx + rng.integers(-9, 10, n), -3, W + 2)
        if i % 7 == 0:
            r, c = np.repeat(r[:1], n), np.repeat(c[:1], n)    # all vertices equal
        rois.append({"theT": int(rng.integers(0, T)), "points": _pts(r, c)})
    mask, outl = rois_to_masks(rois, T, H, W)
    wm, wo = ref.rois_to_masks(_coords(rois, H, W), T, H, W)
    assert mask.dtype == wm.dtype and np.array_equal(mask, wm)
    assert np.array_equal(outl, wo)
    got, want = analyze_masks(mask), pd.DataFrame(ref.analyze(wm))
    check_table(got, want.to_csv(index=False))


def test_synthetic_2048_stack_from_traced_rois_vs_restatement():
    from microbeseg_amd.inference.analysis import analyze_masks, rois_to_masks
    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.utils.synth import synth_instance_mask
    rng = np.random.Generator(np.random.PCG64(21))
    T, S = 4, 2048
    worker = InferWorker.__new__(InferWorker)
    worker.channel = 0
    rois = []
    for t in range(T):
        lab = np.zeros((S, S), np.uint16)            # 4 x 4 tiles of 512^2 synthetic masks, ids made unique
        nxt = 0
        for i in range(16):
            m = synth_instance_mask(rng, 512, 40, rmin=3, rmax=16).astype(np.int64)
            lab[(i // 4) * 512:(i // 4 + 1) * 512, (i % 4) * 512:(i % 4 + 1) * 512] = np.where(m > 0, m + nxt, 0)
            nxt += int(m.max())
        rois += worker.polygon_rois(lab, t)
    mask, outl = rois_to_masks(rois, T, S, S)
    wm, wo = ref.rois_to_masks(_coords(rois, S, S), T, S, S)
    assert np.array_equal(mask, wm) and np.array_equal(outl, wo)
    check_table(analyze_masks(mask), pd.DataFrame(ref.analyze(wm)).to_csv(index=False))


def test_two_runs_identical():
    from microbeseg_amd.inference.analysis import analyze_masks, rois_to_masks
    z, rois, T, H, W = load_case("mixed")
    a = rois_to_masks(rois, T, H, W)
    b = rois_to_masks(rois, T, H, W)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    da, db = analyze_masks(a[0]), analyze_masks(b[0])
    assert da.to_csv(index=False) == db.to_csv(index=False)


def test_empty_frame_nan_and_all_empty_writes_nothing(tmp_path):
    from microbeseg_amd.inference.analysis import analyze_local, analyze_masks
    m = np.zeros((3, 20, 20), np.uint16)
    m[0, 2:5, 2:6] = 1
    m[2, 10:12, 1:3] = 1
    df = analyze_masks(m)
    assert df["counts"].tolist() == [1, 0, 1] and np.isnan(df["mean_area"][1])
    assert df.to_csv(index=False).splitlines()[2] == "1,0,,0,,"
    out = tmp_path / "x_analysis.csv"
    msgs = []
    assert analyze_local([], 2, 8, 8, out, text_output=msgs.append) is None and not out.exists()
    assert "no segmentation results found" in msgs[0]


def test_overlay_two_channels_raises():
    from microbeseg_amd.inference.result_export import overlay
    with pytest.raises(ValueError):
        overlay(np.zeros((1, 4, 4, 2), np.uint8), np.zeros((1, 4, 4), bool))


def _constant_distance_model(path):
    """a DU-Net checkpoint whose output heads are zero convolutions with constant biases: cell distance 0.9 and border
    0.0 everywhere, so the distance post-processing finds exactly one cell per frame whatever the input (the test does
    not depend on how a training run turns out)"""
    import json
    from microbeseg_amd.utils.unets import DUNet
    torch.manual_seed(0)
    net = DUNet(filters=(8, 16))
    sd = net.state_dict()
    for head, bias in (("decoder1Conv.1", 0.0), ("decoder2Conv.1", 0.9)):
        sd[head + ".weight"].zero_()
        sd[head + ".bias"].fill_(bias)
    torch.save(sd, str(path.with_suffix(".pth")))
    with open(path.with_suffix(".json"), "w") as f:
        json.dump({"architecture": ["DU", "conv", "relu", "bn", [8, 16]], "label_type": "distance"}, f)
    return path


def test_infer_script_export_end_to_end(tmp_path):
    import json
    from microbeseg_amd.inference.analysis import analyze_masks, rois_to_masks
    from microbeseg_amd.utils import synth, tiffio
    model = _constant_distance_model(tmp_path / "distance_model_00")
    rng = np.random.Generator(np.random.PCG64(9))
    stack = np.stack([synth.synth_crop(rng, 128)["img"] for _ in range(4)])     # 3 frames would read as channels
    assert stack.dtype == np.uint16
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    tiffio.imwrite(str(imgs / "movie.tif"), stack)
    tiffio.imwrite(str(imgs / "movie_f32.tif"), stack.astype(np.float32))   # segmented, but not exported
    res = tmp_path / "results"
    r = subprocess.run([sys.executable, str(ROOT / "infer_script_local.py"), "-i", str(imgs), "-m", str(model), "-r",
                        str(res), "--rois", "--export"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Skip export of movie_f32 (the overlay needs uint8 / uint16 images, got float32)" in r.stdout
    assert (res / "mask_movie_f32_channel0.tif").is_file() and not (res / "movie_f32_channel0_export").exists()
    rois = json.load(open(res / "mask_movie_channel0_rois.json"))["rois"]
    assert sorted(r["theT"] for r in rois) == [0, 1, 2, 3]            # one cell per frame
    exp = res / "movie_channel0_export"
    names = ["movie.tif", "movie_mask.tif", "movie_overlay.tif", "movie_outlines.tif", "movie_analysis.csv"]
    assert sorted(p.name for p in exp.iterdir()) == sorted(names)
    mask, outl = rois_to_masks(rois, 4, 128, 128)
    assert np.array_equal(mask, tiffio.imread(str(res / "mask_movie_channel0.tif")))   # the ROIs give back the masks
    assert (exp / "movie_analysis.csv").read_text() == analyze_masks(mask).to_csv(index=False)
    assert np.array_equal(tiffio.imread(str(exp / "movie.tif")), stack)
    assert np.array_equal(tiffio.imread(str(exp / "movie_mask.tif")), mask)
    assert np.array_equal(tiffio.imread(str(exp / "movie_outlines.tif")), outl)
    assert np.array_equal(tiffio.imread(str(exp / "movie_overlay.tif")), ref.overlay(stack, outl))


def test_fill_rule_probe_polygons_on_the_device():
    """the probe shapes of the recovered rule through the kernels themselves"""
    from microbeseg_amd.inference.analysis import rois_to_masks
    H, W = 24, 32
    shapes = [([1, 5, 9, 2], [2, 8, 3, 1]),          # vertices and the edge point (3, 5) filled
              ([15, 7], [0, 22]),                      # exact edge point (11, 11) excluded
              ([4], [6]),                              # 1-point polygon: its vertex
              ([0, 8, 8, 0], [26, 26, 30, 30]),        # every edge point of a rectangle
              ([20, 20], [3, 9])]                      # horizontal 2-point polygon
    for r, c in shapes:
        mask, outl = rois_to_masks([{"theT": 0, "points": _pts(r, c)}], 1, H, W)
        rr, cc = ref.fill_polygons([(np.array(r), np.array(c))])[0]
        want = np.zeros((H, W), bool)
        want[rr, cc] = True
        assert np.array_equal(mask[0] > 0, want), (r, c)
        pr, pc = ref.perimeter(np.array(r), np.array(c), (H, W))
        wo = np.zeros((H, W), bool)
        wo[pr, pc] = True
        assert np.array_equal(outl[0], wo), (r, c)
    m, _ = rois_to_masks([{"theT": 0, "points": _pts([1, 5, 9, 2], [2, 8, 3, 1])}], 1, H, W)
    assert all(m[0][p] for p in [(1, 2), (5, 8), (9, 3), (3, 5)])
    m, _ = rois_to_masks([{"theT": 0, "points": _pts([15, 7], [0, 22])}], 1, H, W)
    assert m[0, 11, 11] == 0 and m[0, 15, 0] and m[0, 7, 22]
    m, o = rois_to_masks([{"theT": 0, "points": _pts([4], [6])}], 1, H, W)
    assert np.argwhere(m[0]).tolist() == [[4, 6]] and np.argwhere(o[0]).tolist() == [[4, 6]]
