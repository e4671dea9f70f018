"""CPU: the restatement of the reference's Analysis / Export loops (tests/analysis_ref.py) against the reference's own
outputs (tests/golden/analysis_*.npz, tools/gen_golden_analysis.py), the make_coordinates contract, the recovered fill
rule on probe examples, and the RGB / bool pages of utils/tiffio.py."""
import io
import pathlib

import numpy as np
import pandas as pd
import pytest

import analysis_ref as ref

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
CASES = ["mixed", "rgb", "wrap", "empty"]


def load_case(name):
    z = np.load(GOLDEN / f"analysis_{name}.npz")
    T, H, W = (int(v) for v in z["shape"])
    pts = str(z["points"]).split("\n") if z["theT"].size else []
    rois = [{"theT": int(t), "points": p} for t, p in zip(z["theT"], pts)]
    return z, rois, T, H, W


def check_table(df, csv_text):
    """the reference's CSV: integer columns and mean_area exact, axis means rtol 1e-9 / atol 1e-6 px, NaN where NaN"""
    want = pd.read_csv(io.StringIO(csv_text), float_precision="round_trip")
    assert list(df.columns) == list(want.columns)
    for col in ("frame", "counts", "total_area"):
        assert np.array_equal(np.asarray(df[col], np.int64), np.asarray(want[col], np.int64)), col
    assert np.array_equal(np.asarray(df["mean_area"], float), np.asarray(want["mean_area"], float), equal_nan=True)
    for col in ("mean_minor_axis_length", "mean_major_axis_length"):
        np.testing.assert_allclose(np.asarray(df[col], float), np.asarray(want[col], float), rtol=1e-9, atol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_reference(name):
    z, rois, T, H, W = load_case(name)
    coords = [(r["theT"],) + tuple(np.asarray(v) for v in ref.make_coordinates(r["points"], W, H)) for r in rois]
    mask, outl = ref.rois_to_masks(coords, T, H, W)
    if "csv" not in z:
        assert mask.max(initial=0) == 0 and "no segmentation results found" in str(z["messages"])
        return
    assert mask.dtype == z["mask"].dtype and np.array_equal(mask, z["mask"])
    assert np.array_equal(outl, z["outlines"])
    check_table(pd.DataFrame(ref.analyze(mask)), str(z["csv"]))
    assert np.array_equal(ref.overlay(z["img"], outl), z["overlay"])


def test_wrap_case_crosses_the_cast():
    z, rois, T, H, W = load_case("wrap")
    assert len(rois) > 66600 - 1 >= ref.CAST_AT
    # the wrapped cell 65536 writes 0: it erases pixel (1, 1) of cell 400, whose other pixels stay
    assert ref.cell_value(65536) == 0 and ref.cell_value(65537) == 1 and ref.cell_value(66535) == 66535
    (rr, cc), = ref.fill_polygons([ref.make_coordinates(rois[399]["points"], W, H)])
    assert (1, 1) in set(zip(rr.tolist(), cc.tolist())) and rois[399]["theT"] == 0
    m = z["mask"]
    assert m[0, 1, 1] == 0 and m[0, 1, 2] > 0 and m[0, 2, 1] > 0


def test_empty_frame_gives_nan_and_empty_csv_field():
    z, rois, T, H, W = load_case("mixed")
    df = pd.read_csv(io.StringIO(str(z["csv"])))
    assert df["counts"][1] == 0 and np.isnan(df["mean_area"][1])
    line = str(z["csv"]).splitlines()[2]
    assert line == "1,0,,0,,"


def test_make_coordinates_contract():
    from microbeseg_amd.inference.analysis import make_coordinates
    s = "3.5,2.5 -4,7 100.4,1e1 nocomma 2,3,  0.5,99.5 "
    r, c = make_coordinates(s, size_x=50, size_y=40)
    # Python round: half to even; clamped to 0 .. size-1; tokens without a comma skipped; extra fields ignored
    assert [int(v) for v in r] == [2, 7, 10, 3, 39]
    assert [int(v) for v in c] == [4, 0, 49, 2, 0]
    assert (r, c) == tuple(map(list, ref.make_coordinates(s, 50, 40)))


def _fill_set(r, c):
    rr, cc = ref.fill_polygons([(np.array(r), np.array(c))])[0]
    return set(zip(rr.tolist(), cc.tolist()))


def test_fill_rule_probe_examples():
    filled = _fill_set([1, 5, 9, 2], [2, 8, 3, 1])
    # vertices (1,2), (5,8), (9,3) and the edge point (3,5) are filled, unlike textbook half-open PNPOLY
    assert {(1, 2), (5, 8), (9, 3), (3, 5)} <= filled
    # 2-point polygon (15,0)-(7,22): the exact edge point (11,11) is excluded, its end points are vertices
    seg = _fill_set([15, 7], [0, 22])
    assert (11, 11) not in seg and {(15, 0), (7, 22)} <= seg
    # a single-point polygon fills its vertex
    assert _fill_set([4], [6]) == {(4, 6)}


def test_fill_rule_closed_edges_of_a_rectangle():
    # every edge point of an axis-aligned rectangle is filled (left and right crossing parities differ: 'edge')
    assert _fill_set([0, 8, 8, 0], [26, 26, 30, 30]) == {(y, x) for y in range(9) for x in range(26, 31)}


def test_bresenham_and_perimeter():
    rr, cc = ref.line(0, 0, 3, 7)
    assert rr.tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and cc.tolist() == list(range(8))
    pr, pc = ref.perimeter(np.array([5]), np.array([5]), (10, 10))
    assert set(zip(pr.tolist(), pc.tolist())) == {(5, 5)}


def test_tiffio_rgb_and_bool_pages(tmp_path):
    from microbeseg_amd.utils import tiffio
    rng = np.random.default_rng(3)
    arrays = {"rgb": rng.integers(0, 256, (3, 9, 11, 3)).astype(np.uint8),
              "rgb16": rng.integers(0, 65536, (2, 9, 11, 3)).astype(np.uint16),   # export of a uint16 3-channel image
              "c5": rng.integers(0, 65536, (2, 6, 7, 5)).astype(np.uint16),      # more than 3 channels
              "b": rng.random((2, 7, 13)) > 0.5}
    saved = tiffio._tf
    tiffio._tf = None                      # the dependency-free writer / reader
    try:
        for name, a in arrays.items():
            tiffio.imwrite(str(tmp_path / f"{name}.tif"), a)
        back = {name: tiffio.imread(str(tmp_path / f"{name}.tif")) for name in arrays}
    finally:
        tiffio._tf = saved
    for name, a in arrays.items():
        assert back[name].dtype == a.dtype and back[name].shape == a.shape and np.array_equal(back[name], a), name
