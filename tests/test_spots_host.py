"""CPU: the per-cell fluorescent foci — the two restatements of the band-pass response in tests/spots_ref.py
against each other and against closed forms, the peak test, the position along the cell's axes, the columns and their
formulas, the --spots flag and the declarations.  Every comparison is exact unless it says otherwise."""
import functools
import math
import pathlib
import re
import sys
from math import comb

import numpy as np
import pytest

import spots_ref as sref

ROOT = pathlib.Path(__file__).resolve().parents[1]
SCALES = (1, 2, 3, 4, 5)
SPOT_COLUMNS = ["n_spots_ch{c}", "spot_max_ch{c}", "spot_sum_ch{c}", "bg_spots_ch{c}"]
SPOT_TABLE_COLUMNS = ["frame", "channel", "label", "y", "x", "value", "response", "axis_pos", "axis_off"]


def cells_module():
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    from microbeseg_amd.inference import cells
    return cells


# ---- the response -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES)
def test_the_two_restatements_agree(s):
    rng = np.random.default_rng(10 + s)
    for H, W in ((1, 1), (1, 7), (3, 3), (9, 14), (23, 17)):
        for dtype, top in ((np.uint8, 256), (np.uint16, 65536)):
            v = rng.integers(0, top, (H, W)).astype(dtype)
            a, b = sref.response(v, s), sref.response_passes(v, s)
            assert a.dtype == b.dtype == np.int64 and a.shape == (H, W) and np.array_equal(a, b), (H, W, dtype)
            assert a.any() or H * W == 1                         # a 1 x 1 frame is constant under edge extension


@pytest.mark.parametrize("s", SCALES)
def test_constant_planes_have_no_response(s):
    for value in (0, 1, 255, 65535):
        assert not sref.response(np.full((7, 9), value, np.uint16), s).any()
        assert not sref.response_passes(np.full((1, 1), value, np.uint16), s).any()
    assert sref.spots(sref.response(np.full((7, 9), 65535, np.uint16), s), 1, s) == []


@pytest.mark.parametrize("s", SCALES)
def test_single_pixel_gives_the_product_of_binomial_coefficients(s):
    n = 8 * s + 3                                                # the pixel's whole footprint stays inside the frame
    v = np.zeros((n, n), np.uint8)
    c = n // 2
    v[c, c] = 1
    d = sref.response(v, s)
    for dy in range(-2 * s - 1, 2 * s + 2):
        for dx in range(-2 * s - 1, 2 * s + 2):
            narrow = comb(2 * s, s + dy) * comb(2 * s, s + dx) if abs(dy) <= s and abs(dx) <= s else 0
            wide = comb(4 * s, 2 * s + dy) * comb(4 * s, 2 * s + dx) if abs(dy) <= 2 * s and abs(dx) <= 2 * s else 0
            assert int(d[c + dy, c + dx]) == 16 ** s * narrow - wide
    assert int(d.sum()) == 16 ** s * 4 ** (2 * s) - 4 ** (4 * s) == 0         # a band-pass: no response to the mean
    assert sref.spots(d, 1, s) == [] and sref.spots(200 * d, 1, s) == [(c, c)]    # 1 grey level answers with < 1


def saturated_planes(H=9, W=11):
    """the all-65535 plane with one 0 pixel, and its inverse; read only"""
    full = np.full((H, W), 65535, np.uint16)
    full[H // 2, W // 2 + 1] = 0
    hole, peak = full, (65535 - full).astype(np.uint16)
    hole.setflags(write=False)
    peak.setflags(write=False)
    return hole, peak


def test_saturated_planes_stay_below_2_to_56_and_equal_python_integers():
    s = 5
    for v in saturated_planes():
        d = sref.response(v, s)
        assert np.array_equal(d, sref.response_passes(v, s))
        H, W = v.shape
        big = [[int(v[min(max(y, 0), H - 1), min(max(x, 0), W - 1)]) for x in range(-2 * s, W + 2 * s)]
               for y in range(-2 * s, H + 2 * s)]                # Python integers, edge-extended by hand

        def smooth(k, y, x):
            return sum(comb(2 * k, i) * comb(2 * k, j) * big[y + 2 * s - k + i][x + 2 * s - k + j]
                       for i in range(2 * k + 1) for j in range(2 * k + 1))

        for y, x in ((0, 0), (H // 2, W // 2 + 1), (H // 2, W // 2), (H - 1, W - 1), (2, 7)):
            first, second = 16 ** s * smooth(s, y, x), smooth(2 * s, y, x)
            assert first < 2 ** 56 and second < 2 ** 56 and int(d[y, x]) == first - second
        assert int(np.abs(d).max()) < 2 ** 56 and d.any()
    hole, peak = saturated_planes()
    assert np.array_equal(sref.response(hole, s), -sref.response(peak, s))     # linear, and constants give 0
    assert sref.spots(sref.response(peak, s), 1, s) == [(4, 6)]


# ---- the peak test ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", (1, 2, 5))
def test_plateaus_yield_one_spot_the_first_in_raster_order(s):
    for pixels in ([(10, 12), (10, 13)], [(10, 12), (11, 12)], [(10, 12), (11, 13)], [(10, 13), (11, 12)],
                   [(10, 12), (10, 13), (11, 12), (11, 13)]):
        v = np.full((24, 27), 100, np.uint16)
        for y, x in pixels:
            v[y, x] = 5000
        d = sref.response(v, s)
        assert len({int(d[y, x]) for y, x in pixels}) == 1       # a plateau of the response by symmetry
        assert sref.spots(d, 1, s) == [min(pixels)]
    d = np.zeros((3, 4), np.int64)                                # a plateau over the whole frame, at the threshold
    d[:] = 7 * 16 ** (2 * s)
    assert sref.spots(d, 7, s) == [(0, 0)] and sref.spots(d, 8, s) == []


@pytest.mark.parametrize("s", SCALES)
def test_no_two_spots_are_adjacent(s):
    rng = np.random.default_rng(s)
    for H, W in ((12, 15), (1, 30), (30, 1), (2, 2)):
        v = rng.integers(0, 4, (H, W)).astype(np.uint8) * 60      # few levels: many ties
        found = sref.spots(sref.response(v, s), 1, s)
        assert len(found) <= ((H + 1) // 2) * ((W + 1) // 2)
        assert found == sorted(found) and (len(found) > 0 or H * W <= 4)
        for i, (y, x) in enumerate(found):
            assert all(max(abs(y - yy), abs(x - xx)) > 1 for yy, xx in found[i + 1:])


def blob_plane(H, W, centres, amplitude, sigma, base=200, dtype=np.uint16):
    yy, xx = np.mgrid[:H, :W]
    v = np.full((H, W), float(base))
    for cy, cx in centres:
        v += amplitude * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sigma * sigma))
    return np.rint(v).astype(dtype)


@pytest.mark.parametrize("s", SCALES)
def test_gaussian_blobs_are_found_once_at_their_centre(s):
    centres = [(20, 20), (20, 60), (50, 41), (70, 75)]           # further apart than the filters reach
    v = blob_plane(90, 100, centres, 3000, math.sqrt(s / 2.0) + 0.5)
    d = sref.response(v, s)
    best = min(int(d[c]) for c in centres) // 16 ** (2 * s)      # whole grey levels every blob reaches
    assert best >= 100
    assert sref.spots(d, best, s) == centres
    assert sref.spots(d, 5, s) == centres                        # the flat background has no response
    assert sref.spots(d, max(int(d[c]) for c in centres) // 16 ** (2 * s) + 1, s) == []


# ---- the position along the cell ----------------------------------------------------------------------------------------------------
def rod(angle_deg, half_len=20, half_wid=3, n=64):
    """a rod through the centre of an n x n frame, its long axis (cos a, sin a) in (row, column); label 1"""
    a = math.radians(angle_deg)
    yy, xx = np.mgrid[:n, :n] - (n - 1) / 2.0
    along, across = yy * math.cos(a) + xx * math.sin(a), xx * math.cos(a) - yy * math.sin(a)
    return ((np.abs(along) <= half_len) & (np.abs(across) <= half_wid)).astype(np.int32)


def sums_of(mask):
    ys, xs = (v.astype(object) for v in np.nonzero(mask))
    return len(ys), int(ys.sum()), int(xs.sum()), int((ys * ys).sum()), int((xs * xs).sum()), int((xs * ys).sum())


def raw_of(mask):
    """the part of measure_raw's result spots_from_records reads, for one frame holding label 1"""
    return {"shape": np.array(sums_of(mask), np.uint64).reshape(6, 1)}


@pytest.mark.parametrize("angle", (-80, -50, -20, 0, 30, 40, 60, 90))
def test_axis_position_of_a_slanted_rod(angle):
    cells = cells_module()
    mask = rod(angle)
    n, sy, sx, syy, sxx, sxy = sums_of(mask)
    major, minor, orientation = cells._axes(n, sy, sx, syy, sxx, sxy)
    want = math.radians(angle)                                   # the table's orientation is the rod's angle (mod pi)
    assert abs(math.remainder(orientation - want, math.pi)) < 0.02
    cy, cx = sy / n, sx / n
    ys, xs = np.nonzero(mask)
    along = (ys - cy) * math.cos(want) + (xs - cx) * math.sin(want)
    across = (xs - cx) * math.cos(want) - (ys - cy) * math.sin(want)
    # A uniform rod of half length a = 20 and half width b = 3 has variances a^2 / 3 and b^2 / 3: half its major axis is
    # 2 a / sqrt(3) = 1.155 a, half its minor axis 1.155 b.  The last pixel centre on the axis lies within a - 1.5 .. a of the
    # centroid, so |axis_pos| is in 0.80 .. 0.87 and, less than a pixel off the axis, |axis_off| < 1 / (1.155 b) = 0.29; a
    # rim pixel at mid-cell lies b - 1.5 .. b off the axis: |axis_off| in 0.43 .. 0.87
    far = int(np.argmax(along - 2 * np.abs(across)))             # the pixel at the far end of the rod, on its axis
    pos, offs = cells.spot_axes(ys[far] - cy, xs[far] - cx, major, minor, orientation)
    assert 0.78 < abs(float(pos)) < 0.89 and abs(float(offs)) < 0.29, (pos, offs)
    near = int(np.argmin(along - 2 * np.abs(across)))            # the other pole: the other sign
    assert float(cells.spot_axes(ys[near] - cy, xs[near] - cx, major, minor, orientation)[0]) * float(pos) < -0.6
    mid = int(np.argmin(np.abs(along) + np.abs(across)))
    pos, offs = cells.spot_axes(ys[mid] - cy, xs[mid] - cx, major, minor, orientation)
    assert abs(float(pos)) < 0.05 and abs(float(offs)) < 0.29    # within a pixel of the centroid
    side = int(np.argmax(across - np.abs(along)))
    pos, offs = cells.spot_axes(ys[side] - cy, xs[side] - cx, major, minor, orientation)
    assert abs(float(pos)) < 0.05 and 0.43 < abs(float(offs)) < 0.89, (pos, offs)         # on the rim at mid-cell
    assert cells.spot_axes(0.0, 0.0, major, minor, orientation) == (0.0, 0.0)
    records = np.array([(0, 0, int(ys[far]), int(xs[far]), 1, 900, 5 << 16), (0, 0, 0, 0, 0, 7, 3 << 16)], cells.SPOT_RECORD)
    df = cells.spots_from_records(records, 2, [0, 1], raw_of(mask), [3], background=True)
    assert list(df.columns) == SPOT_TABLE_COLUMNS and df["channel"].tolist() == [3, 3]
    assert df["response"].tolist() == [5.0, 3.0] and df["value"].tolist() == [900, 7]
    want_pos, want_off = cells.spot_axes(ys[far] - cy, xs[far] - cx, major, minor, orientation)
    assert df["axis_pos"][0] == float(want_pos) and df["axis_off"][0] == float(want_off)
    assert math.isnan(df["axis_pos"][1]) and math.isnan(df["axis_off"][1])                # label 0
    assert len(cells.spots_from_records(records, 2, [0, 1], raw_of(mask), [3])) == 1      # background=False drops it


def test_axis_position_is_nan_on_a_zero_axis():
    cells = cells_module()
    line = np.zeros((8, 8), np.int32)
    line[3, 1:7] = 1                                             # one pixel wide: no minor axis
    major, minor, orientation = cells._axes(*sums_of(line))
    assert major > 0 and minor == 0
    pos, offs = cells.spot_axes(0.0, 2.5, major, minor, orientation)
    assert abs(abs(float(pos)) - 2.5 / (0.5 * major)) < 1e-12 and math.isnan(float(offs))
    dot = np.zeros((8, 8), np.int32)
    dot[2, 2] = 1
    records = np.array([(0, 0, 2, 2, 1, 9, 1 << 8), (0, 0, 5, 5, 4, 9, 1 << 8)], cells.SPOT_RECORD)
    df = cells.spots_from_records(records, 1, [0, 1], raw_of(dot), [0])
    assert df["label"].tolist() == [1, 4] and df["axis_pos"].isna().all() and df["axis_off"].isna().all()


# ---- the columns and their formulas -----------------------------------------------------------------------------------------------------
def test_columns():
    cells = cells_module()
    assert cells.SPOT_COLUMNS == SPOT_COLUMNS and cells.SPOT_TABLE_COLUMNS == SPOT_TABLE_COLUMNS
    plain = cells.columns([0, 2], True, neighbors=True)
    assert cells.columns([0, 2], True, neighbors=True, spots=False) == plain
    assert cells.columns([0, 2], True, neighbors=True, spots=True) == plain + [
        "n_spots_ch0", "spot_max_ch0", "spot_sum_ch0", "bg_spots_ch0", "n_spots_ch2", "spot_max_ch2", "spot_sum_ch2", "bg_spots_ch2"]
    assert cells.columns([], False, spots=True) == cells.columns([], False)
    assert cells.SPOT_RECORD.itemsize == 32 and cells.SPOT_RECORD.fields["d"][1] == 24
    assert cells.spot_bound(2, 5, 3, 2) == 2 * 2 * 3 * 2 and cells.spot_bound(1, 1, 1) == 1


def test_check_spots():
    cells = cells_module()
    assert cells.check_spots(None) is None and cells.check_spots(None, 99) is None
    assert cells.check_spots(50) == (50, 2) and cells.check_spots(np.int64(1), 5.0) == (1, 5)
    assert cells.check_spots(65535, 1) == (65535, 1)
    for thr in (0, -1, 65536, 2.5, "50", True, [50]):
        with pytest.raises(ValueError, match="spots"):
            cells.check_spots(thr)
    for scale in (0, 6, 1.5, None, "2", False):
        with pytest.raises(ValueError, match="spot_scale"):
            cells.check_spots(50, scale)


def test_measure_cells_argument_errors():
    cells = cells_module()
    lab = np.ones((1, 4, 4), np.uint16)
    with pytest.raises(ValueError, match="spots"):               # raised before any device is asked for
        cells.measure_cells(lab, np.zeros((1, 4, 4), np.uint8), spots=0)
    with pytest.raises(ValueError, match="spot_scale"):
        cells.measure_cells(lab, np.zeros((1, 4, 4), np.uint8), spots=5, spot_scale=6)
    with pytest.raises(ValueError, match="spots are taken of an image's channels: no image given"):
        cells.measure_cells(lab, spots=5)
    with pytest.raises(ValueError, match="threshold"):
        cells.cell_spots(lab, np.zeros((1, 4, 4), np.uint8))
    with pytest.raises(ValueError, match="no image given"):
        cells.cell_spots(lab, None, spots=5)


def test_table_columns_from_counts_and_records():
    cells = cells_module()
    mask = np.zeros((2, 6, 8), np.int32)
    mask[0, 1:4, 1:4] = 1
    mask[0, 1:4, 5:7] = 2
    mask[1, 2:5, 2:6] = 1
    off = np.array([0, 2, 3], np.int64)
    shape = np.zeros((6, 3), np.uint64)
    bbox = np.zeros((3, 4), np.int32)
    for slot, (t, l) in enumerate(((0, 1), (0, 2), (1, 1))):
        shape[:, slot] = sums_of(mask[t] == l)
        ys, xs = np.nonzero(mask[t] == l)
        bbox[slot] = ys.min(), xs.min(), ys.max() + 1, xs.max() + 1
    raw = {"shape": shape, "bbox": bbox, "ch_sums": np.ones((2, 1, 3), np.uint64), "ch_minmax": np.zeros((2, 1, 3), np.uint32),
           "bg_sums": np.ones((3, 2, 1), np.uint64), "bg_minmax": np.zeros((2, 2, 1), np.uint32)}
    unit = 16 ** 4
    big = 2 ** 55 + 1                                            # fp64 cannot hold the sum of two of these: Python integers do
    records = np.array([(0, 0, 2, 2, 1, 10, 3 * unit + 1), (0, 0, 2, 6, 2, 10, big), (0, 0, 3, 5, 2, 10, big),
                        (0, 0, 5, 7, 0, 10, 9 * unit), (1, 0, 0, 0, 0, 10, unit), (1, 0, 5, 0, 7, 10, unit)], cells.SPOT_RECORD)
    counts, bg = np.array([[1, 2, 0]], np.int32), np.array([[1], [1]], np.int32)
    df = cells.table_from_sums(off, 6, 8, raw, channels=[4], spots=(2, counts, bg, records))
    assert list(df.columns) == cells.columns([4], False, spots=True)
    assert df["n_spots_ch4"].tolist() == [1, 2, 0] and df["bg_spots_ch4"].tolist() == [1, 1, 1]
    assert df["spot_max_ch4"].tolist()[:2] == [(3 * unit + 1) / unit, big / unit] and math.isnan(df["spot_max_ch4"][2])
    assert df["spot_sum_ch4"].tolist() == [(3 * unit + 1) / unit, (2 * big) / unit, 0.0]
    plain = cells.table_from_sums(off, 6, 8, raw, channels=[4])
    assert list(plain.columns) == cells.columns([4], False) and df[list(plain.columns)].equals(plain)
    with pytest.raises(ValueError, match="spots"):
        cells.table_from_sums(off, 6, 8, raw, channels=[], spots=(2, counts, bg, records))


# ---- the flag and the declarations ------------------------------------------------------------------------------------------------------
def test_flag_rules():
    sys.path.insert(0, str(ROOT))
    try:
        import infer_script_local as cli
    finally:
        sys.path.remove(str(ROOT))
    parser = cli.build_parser()
    base = ["-i", "x", "-m", "y"]
    ns = parser.parse_args(base + ["--cells"])
    assert ns.spots is None and ns.spot_scale == 2
    ns = parser.parse_args(base + ["--cells", "--spots", "50"])
    assert ns.spots == 50 and ns.spot_scale == 2
    ns = parser.parse_args(base + ["--cells", "--spots", "7", "--spot_scale", "5"])
    assert (ns.spots, ns.spot_scale) == (7, 5)
    for bad in (["--spots", "50"], ["--cells", "--spots", "0"], ["--cells", "--spots", "65536"],
                ["--cells", "--spots", "50", "--spot_scale", "6"], ["--cells", "--spots", "50", "--spot_scale", "0"]):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)


def test_declarations_agree():
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    source = (ROOT / "microbeseg_amd" / "csrc" / "spots.hip").read_text()
    build = (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()
    lib = (ROOT / "microbeseg_amd" / "_lib.py").read_text()
    assert "spots.hip" in build
    for name in ("mseg_cell_spots_workspace_bytes", "mseg_cell_spots"):
        assert re.search(r"\b%s\(" % name, header) and re.search(r'extern "C" \w+ %s\(' % name, source)
        assert '"%s"' % name in lib
    proto = re.search(r"int mseg_cell_spots\((.*?)\);", header, re.S).group(1)
    entry = re.search(r'"mseg_cell_spots": \(_I, \[(.*?)\]\)', lib, re.S).group(1)
    assert len(proto.split(",")) == len(entry.split(",")) == 25
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "mseg_cell_spots" in (ROOT / doc).read_text() or doc == "README.md"
    assert "--spots" in (ROOT / "README.md").read_text() and "§6t" in (ROOT / "DESIGN.md").read_text()
