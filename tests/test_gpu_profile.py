"""GPU (MI355X): the per-cell intensity profile (csrc/profile.hip) through the C ABI and through measure_cells /
cell_profiles, every integer equal to the restatement tests/profile_ref.py (which test_profile_host.py checks against
independent forms on the CPU).  Boxes and areas come from tests/cells_ref.py, never from the code under test."""
import ctypes as C
import functools
import math

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
import profile_ref as pref
from test_gpu_cells import PIX, Guarded, _dev, scene_a
from test_gpu_order_stats import SHAPES, image, laid_out, measured, scene, tchw

pytestmark = pytest.mark.gpu
EINVAL = -1
UNIT = 16384
CAP = 8                   # PF_MAXC of csrc/profile.hip: the channels of one call


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def c_profile(lab, off, base, strides, nch, bbox, dirs, N, nch_arg=None, img_code=None, lab_code=None, HW=None):
    """mseg_cell_profile through ctypes.  base: the image's memory (any shape) with the element strides (frame, channel, row,
    pixel) of channel 0 -> (return code, guarded count [N, n], guarded sums [C, N, n], guarded extent [2, n]); the buffers are
    sized for min(max(N, 2), 32) bins, whatever N is passed"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    rows = min(max(N, 2), 32)
    lab_d, off_d, img_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda(), _dev(np.array(base))
    bbox_d = torch.from_numpy(np.array(bbox, np.int32).reshape(-1, 4)).cuda()
    dirs_d = torch.from_numpy(np.array(dirs, np.int32).reshape(-1, 2)).cuda()
    count, sums = Guarded((rows, n), torch.int32), Guarded((nch, rows, n), torch.int64)
    extent = Guarded((2, n), torch.int64)
    if HW is not None:
        H, W = HW
    code = lib.mseg_cell_profile(lab_d.data_ptr(), PIX[lab.dtype] if lab_code is None else lab_code, T, H, W, off_d.data_ptr(),
                                 n, img_d.data_ptr(), PIX[base.dtype] if img_code is None else img_code,
                                 nch if nch_arg is None else nch_arg, *(int(s) for s in strides), bbox_d.data_ptr(),
                                 dirs_d.data_ptr(), N, count.ptr, sums.ptr, extent.ptr,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code, count, sums, extent


def run(lab, off, img, bbox, dirs, N, layout="contig"):
    """one valid call on the logical image img [T, C, H, W] laid out as ``layout`` -> (count, sums, extent); .host() checks
    the guard bands"""
    base, strides = laid_out(img, layout)
    code, count, sums, extent = c_profile(lab, off, base, strides, img.shape[1], bbox, dirs, N)
    assert code == 0, code
    return count.host(np.uint32), sums.host(np.uint64), extent.host(np.int64)


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("count", "sums", "extent")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        assert np.array_equal(g, w), (name, what)


def own_directions(raw):
    from microbeseg_amd.inference import cells
    return cells._cell_directions(raw)


@functools.lru_cache(maxsize=None)
def restated(H, W, T, img_dtype, Cn, N):
    lab, off = scene(H, W, T)
    img, raw = measured(H, W, T, img_dtype, Cn)
    dirs = own_directions(raw)
    return dirs, pref.profile(lab, off, img, raw["bbox"], dirs, N)


# ---- random scenes against the restatement --------------------------------------------------------------------------------------
COMBOS = [(1, 1, "contig", 2), (4, 3, "contig", 16), (4, 3, "hwc", 5), (1, CAP, "hwc", 32), (4, 1, "pitch", 16),
          (1, 3, "pitch", 32), (4, CAP, "contig", 5)]


@pytest.mark.parametrize("img_dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_integers_equal_the_restatement(shape, label_dtype, img_dtype):
    H, W = shape
    for T, Cn, layout, N in COMBOS:
        lab, off = scene(H, W, T)
        img, raw = measured(H, W, T, img_dtype, Cn)
        dirs, want = restated(H, W, T, img_dtype, Cn, N)
        got = run(lab.astype(label_dtype), off, img, raw["bbox"], dirs, N, layout)
        same(got, want, (T, Cn, layout, N))
        assert np.array_equal(got[0].sum(axis=0, dtype=np.int64), raw["shape"][0].astype(np.int64))
        assert np.array_equal(got[1].sum(axis=1), raw["ch_sums"][0])             # the bins add up to the cell's sums


@pytest.mark.parametrize("img_dtype", [np.uint8, np.uint16])
def test_scene_a_absent_and_foreign_ids(img_dtype):
    lab, off = scene_a(np.int32)
    lab = lab.copy()
    lab[0, 12, 30], lab[1, 31, 25] = -7, -2 ** 31                 # negative ids, the second inside the box of the ids above the table
    img = image(img_dtype, (3, 2, 37, 53), seed=9)
    raw = ref.measure(lab, off, img)
    area = raw["shape"][0].astype(np.int64)
    assert area[2] == 0 and area[8] == 0 and (raw["bbox"][2] == 0).all()         # ids 3 and 9 are absent
    dirs = own_directions(raw)
    for N in (2, 5, 16, 32):
        got = run(lab, off, img, raw["bbox"], dirs, N)
        same(got, pref.profile(lab, off, img, raw["bbox"], dirs, N), N)
        assert not got[0][:, [2, 8]].any() and not got[1][:, :, [2, 8]].any() and not got[2][:, [2, 8]].any()
        assert np.array_equal(got[0].sum(axis=0, dtype=np.int64), area)


# ---- directions beyond the ones an orientation gives ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", [(UNIT, 0), (0, UNIT), (11585, 11585), (11585, -11585), (0, 0), (UNIT, -UNIT), (-UNIT, 3)])
def test_given_directions(d):
    lab, off = scene(33, 200, 4)
    img, raw = measured(33, 200, 4, np.uint16, 3)
    dirs = np.tile(np.array(d, np.int32), (int(off[-1]), 1))
    for N in (5, 32):
        got = run(lab.astype(np.uint16), off, img, raw["bbox"], dirs, N, "hwc")
        same(got, pref.profile(lab, off, img, raw["bbox"], dirs, N), (d, N))
        if d == (0, 0):
            assert not got[0][1:].any() and np.array_equal(got[0][0].astype(np.uint64), raw["shape"][0])


def test_any_direction_stays_inside_the_arrays():
    """directions no orientation gives, up to the ends of int32: the bins may be anything, the guard bands hold and every
    pixel is counted once"""
    lab, off = scene(33, 200, 4)
    img, raw = measured(33, 200, 4, np.uint16, 3)
    rng = np.random.default_rng(3)
    dirs = rng.integers(-2 ** 31, 2 ** 31, (int(off[-1]), 2)).astype(np.int32)
    dirs[:4] = [[2 ** 31 - 1, 2 ** 31 - 1], [-2 ** 31, -2 ** 31], [2 ** 31 - 1, -2 ** 31], [-2 ** 31, 2 ** 31 - 1]]
    got = run(lab.astype(np.int32), off, img, raw["bbox"], dirs, 32)
    assert np.array_equal(got[0].sum(axis=0, dtype=np.int64), raw["shape"][0].astype(np.int64))
    assert np.array_equal(got[1].sum(axis=1), raw["ch_sums"][0])
    same(got, pref.profile(lab, off, img, raw["bbox"], dirs, 32))          # 33 x 200: (qmax - qmin + 1) * 32 < 2^63 even so


# ---- structured cases -------------------------------------------------------------------------------------------------------------
def structured_scene():
    """one 48 x 70 frame (int64 labels): 1 a cell of one row (wider than a wave), 2 a cell of one column, 3 .. 6 one-pixel cells
    in the corners, 7 and 8 a checkerboard sharing one box, 9 a slanted rod with an id beyond the table, a negative id and
    background inside its box"""
    H, W = 48, 70
    lab = np.zeros((1, H, W), np.int64)
    lab[0, 2, 1:68] = 1
    lab[0, 4:47, 68] = 2
    for k, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        lab[0, y, x] = 3 + k
    board = np.indices((9, 13)).sum(axis=0) % 2
    lab[0, 6:15, 3:16] = 7 + board
    for i in range(30):
        lab[0, 16 + i, 5 + i:11 + i] = 9
    lab[0, 20, 12], lab[0, 30, 22], lab[0, 35, 26] = 5000, -3, 0
    return lab


@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
def test_structured_cells(label_dtype):
    lab = structured_scene()
    if label_dtype == np.uint16:
        lab = np.where(lab < 0, 0, lab)
    off = ref.frame_tables(np.where(lab > 100, 0, lab))
    assert off.tolist() == [0, 9]
    img = image(np.uint16, (1, 2, 48, 70), seed=6)
    raw = ref.measure(lab, off, img)
    assert raw["bbox"][0].tolist() == [2, 1, 3, 68] and raw["bbox"][1].tolist() == [4, 68, 47, 69]
    assert raw["bbox"][6].tolist() == raw["bbox"][7].tolist() == [6, 3, 15, 16]                    # one shared box
    own = own_directions(raw)
    assert own[0].tolist() == [0, UNIT] and own[1].tolist() == [UNIT, 0]
    for dirs in (own, np.tile(np.array([11585, -11585], np.int32), (9, 1))):
        for N in (2, 5, 16, 32):
            got = run(lab.astype(label_dtype), off, img, raw["bbox"], dirs, N)
            same(got, pref.profile(lab, off, img, raw["bbox"], dirs, N), N)
            assert np.array_equal(got[0].sum(axis=0, dtype=np.int64), raw["shape"][0].astype(np.int64))
            assert got[0][0, 2:6].tolist() == [1, 1, 1, 1] and not got[0][1:, 2:6].any()         # one pixel: bin 0
            assert got[0][:, 6].sum() == 59 and got[0][:, 7].sum() == 58                          # the neighbour's pixels do not count


def test_one_cell_over_the_whole_frame():
    """5 x 200: the lanes wrap rows wider than a wave, and the box touches all four frame edges"""
    lab = np.ones((2, 5, 200), np.int64)
    off = ref.frame_tables(lab)
    img = image(np.uint16, (2, 3, 5, 200), seed=2)
    raw = ref.measure(lab, off, img)
    assert raw["bbox"].tolist() == [[0, 0, 5, 200]] * 2
    for d in ((0, UNIT), (UNIT, 0), (3000, 16107)):
        dirs = np.tile(np.array(d, np.int32), (2, 1))
        for N in (2, 5, 16, 32):
            got = run(lab.astype(np.uint16), off, img, raw["bbox"], dirs, N, "pitch")
            same(got, pref.profile(lab, off, img, raw["bbox"], dirs, N), (d, N))
    assert got[0].sum() == 2000


def test_sums_past_32_bits():
    lab = np.ones((1, 400, 400), np.int32)
    img = np.full((1, 1, 400, 400), 65535, np.uint16)
    count, sums, extent = run(lab, np.array([0, 1]), img, [[0, 0, 400, 400]], [[0, UNIT]], 2)
    assert count[:, 0].tolist() == [80000, 80000]
    assert sums[0, :, 0].tolist() == [80000 * 65535] * 2 and 80000 * 65535 > 2 ** 32
    assert extent[:, 0].tolist() == [0, 399 * UNIT]


def test_tall_frame_numerators_past_32_bits():
    """H = 70000: q reaches 2^30 and (q - qmin) * 32 reaches 2^35; every bin edge is exact"""
    H, W, N = 70000, 3, 32
    rng = np.random.default_rng(4)
    lab = np.zeros((1, H, W), np.int32)
    lab[0, :, 1] = 1
    lab[0, :, 0] = rng.random(H) < 0.3
    lab[0, :, 2] = rng.random(H) < 0.3
    img = rng.integers(0, 256, (1, 1, H, W)).astype(np.uint8)
    off, bbox, dirs = np.array([0, 1]), [[0, 0, H, W]], [[UNIT, 0]]
    want = pref.profile(lab, off, img, bbox, dirs, N)
    assert want[2][1, 0] == UNIT * (H - 1) > 2 ** 30 and (want[2][1, 0] * N) > 2 ** 35
    rows = np.bincount((UNIT * np.arange(H, dtype=np.int64) * N) // (UNIT * (H - 1) + 1), minlength=N)
    assert rows.sum() == H and rows.min() >= H // N - 1
    got = run(lab, off, img, bbox, dirs, N)
    same(got, want)
    assert np.array_equal(got[0][:, 0], np.bincount(np.repeat((UNIT * np.arange(H, dtype=np.int64) * N) // (UNIT * (H - 1) + 1),
                                                              lab[0].sum(axis=1)), minlength=N))


# ---- bad arguments, nothing to do -------------------------------------------------------------------------------------------------
def test_bad_arguments_touch_nothing():
    lab, off = scene(5, 65, 1)
    lab = lab.astype(np.int32)
    img, raw = measured(5, 65, 1, np.uint16, 1)
    base, strides = tchw(img)
    dirs = own_directions(raw)
    cases = {"N = 1": dict(N=1), "N = 33": dict(N=33), "N = 0": dict(N=0), "N = -5": dict(N=-5), "C = 0": dict(nch_arg=0),
             "C = cap + 1": dict(nch_arg=CAP + 1), "C = -1": dict(nch_arg=-1), "image dtype int32": dict(img_code=2),
             "image dtype fp32": dict(img_code=3), "image dtype 7": dict(img_code=7), "label dtype uint8": dict(lab_code=0),
             "label dtype 9": dict(lab_code=9), "H W too large": dict(HW=(46341, 46341)), "H = 0": dict(HW=(0, 65))}
    for what, kw in cases.items():
        N = kw.pop("N", 8)
        code, count, sums, extent = c_profile(lab, off, base, strides, 1, raw["bbox"], dirs, N, **kw)
        assert code == EINVAL, what
        assert count.untouched() and sums.untouched() and extent.untouched(), what
    assert 46341 * 46341 >= 2 ** 31 - 512
    code, count, sums, extent = c_profile(lab, off, base, strides, 1, raw["bbox"], dirs, 8)
    assert code == 0 and not count.untouched()


def test_no_labels_is_a_valid_no_op():
    lab = np.zeros((2, 7, 66), np.uint16)
    lab[1, 3, 3] = 5                                              # beyond the empty table
    img = image(np.uint16, (2, 1, 7, 66), seed=4)
    base, strides = tchw(img)
    code, count, sums, extent = c_profile(lab, np.zeros(3, np.int64), base, strides, 1, np.zeros((0, 4)), np.zeros((0, 2)), 16)
    assert code == 0 and count.untouched() and sums.untouched() and extent.untouched()


def test_two_calls_give_identical_bytes():
    lab, off = scene(70, 131, 4)
    img, raw = measured(70, 131, 4, np.uint16, 3)
    dirs = own_directions(raw)
    a = run(lab.astype(np.uint16), off, img, raw["bbox"], dirs, 16, "hwc")
    b = run(lab.astype(np.uint16), off, img, raw["bbox"], dirs, 16, "hwc")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the host call ------------------------------------------------------------------------------------------------------------------
def on_device(lab, img):
    from microbeseg_amd.inference import cells
    dev = torch.device("cuda", torch.cuda.current_device())
    lab_d, pix = cells._labels_to_device(lab, dev)
    return lab_d, pix, cells._image_to_device(img, lab.shape, dev)


def test_profile_raw_splits_long_channel_runs():
    from microbeseg_amd.inference import cells
    lab, off = scene(5, 65, 4)
    img, raw = measured(5, 65, 4, np.uint16, CAP + 1)
    dirs = own_directions(raw)
    lab_d, pix, image_d = on_device(lab.astype(np.int32), img)
    for channels in (list(range(CAP + 1)), [0], [3, 1, 2, 8], list(range(CAP, -1, -1))):
        got = cells.profile_raw(lab_d, pix, off, image_d, channels, raw["bbox"], dirs, 5, raw["shape"][0])
        same(got, pref.profile(lab, off, img[:, channels], raw["bbox"], dirs, 5), channels)
    got = cells.profile_raw(lab_d, pix, off, image_d, [1], raw["bbox"], dirs, 5)           # the areas are measured there
    same(got, pref.profile(lab, off, img[:, [1]], raw["bbox"], dirs, 5))


def test_profile_raw_raises_on_a_short_box():
    from microbeseg_amd.inference import cells
    lab, off = scene(33, 200, 4)
    img, raw = measured(33, 200, 4, np.uint16, 3)
    dirs = own_directions(raw)
    lab_d, pix, image_d = on_device(lab.astype(np.int32), img)
    cells.profile_raw(lab_d, pix, off, image_d, [0], raw["bbox"], dirs, 8, raw["shape"][0])
    bbox = raw["bbox"].copy()
    s = int(np.flatnonzero(bbox[:, 2] - bbox[:, 0] > 1)[0])
    bbox[s, 0] += 1
    want = pref.profile(lab, off, img[:, [0]], bbox, dirs, 8)
    assert want[0][:, s].sum() < raw["shape"][0][s]
    with pytest.raises(RuntimeError, match="outside the bounding box"):
        cells.profile_raw(lab_d, pix, off, image_d, [0], bbox, dirs, 8, raw["shape"][0])
    with pytest.raises(RuntimeError, match="outside the bounding box"):
        cells.profile_raw(lab_d, pix, off, image_d, [0], bbox, dirs, 8)
    # a box that leaves the frame is clipped: nothing outside the arrays is read
    bbox = raw["bbox"].copy()
    bbox[s] = [-5, -5, 2 ** 31 - 1, 2 ** 31 - 1]
    same(cells.profile_raw(lab_d, pix, off, image_d, [0], bbox, dirs, 8, raw["shape"][0]),
         pref.profile(lab, off, img[:, [0]], raw["bbox"], dirs, 8))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_measure_cells_and_cell_profiles():
    from microbeseg_amd.inference import cells
    lab, off = scene(70, 131, 4)
    lab = lab[:2]
    off = off[:3]
    img = np.ascontiguousarray(measured(70, 131, 4, np.uint16, 3)[0][:2, :2])
    raw = ref.measure(lab, off, img)
    N = 8
    plain = cells.measure_cells(lab, img)
    assert list(plain.columns) == cells.columns([0, 1], True)
    df = cells.measure_cells(lab, img, profile=N)
    extra = ["axis_extent", "pole_mid_ratio_ch0", "pole_asym_ch0", "profile_peak_ch0", "pole_mid_ratio_ch1", "pole_asym_ch1",
             "profile_peak_ch1"]
    assert list(df.columns) == cells.columns([0, 1], True, profile=True) == list(plain.columns) + extra
    pd.testing.assert_frame_equal(df[list(plain.columns)], plain, check_exact=True)
    assert cells.measure_cells(lab, img, profile=None).equals(plain)
    # the orientation of the table itself, restated: the direction the device was given
    dirs = cells.profile_direction(df["orientation"].to_numpy())
    slots = (off[df["frame"].to_numpy()] + df["label"].to_numpy() - 1).astype(np.int64)
    all_dirs = np.zeros((int(off[-1]), 2), np.int32)
    all_dirs[slots] = dirs
    count, sums, extent = pref.profile(lab, off, img, raw["bbox"], all_dirs, N)
    want = {c: [] for c in extra}
    for s in slots.tolist():
        want["axis_extent"].append((int(extent[1, s]) - int(extent[0, s])) / 16384 + 1)
        for c in (0, 1):
            for name, v in zip(("pole_mid_ratio", "pole_asym", "profile_peak"), cells.profile_columns(count[:, s], sums[c, :, s])):
                want[f"{name}_ch{c}"].append(v)
    for c in extra:
        assert df[c].dtype == np.float64 and np.array_equal(df[c].to_numpy(), np.array(want[c], np.float64), equal_nan=True), c
    assert (df["axis_extent"] >= 1).all() and df["profile_peak_ch0"].abs().max() <= 1 - 1 / N
    # the profiles themselves
    prof = cells.cell_profiles(lab, img, bins=N)
    assert list(prof.columns) == cells.PROFILE_TABLE_COLUMNS and len(prof) == len(df) * 2 * N
    rows = [(t, c, l, b) for t, l in zip(df["frame"], df["label"]) for c in (0, 1) for b in range(N)]
    rows.sort()
    assert list(zip(prof["frame"], prof["channel"], prof["label"], prof["bin"])) == rows
    sl = (off[prof["frame"].to_numpy()] + prof["label"].to_numpy() - 1).astype(np.int64)
    b, ch = prof["bin"].to_numpy(), prof["channel"].to_numpy()
    assert np.array_equal(prof["count"].to_numpy(), count[b, sl]) and np.array_equal(prof["sum"].to_numpy(), sums[ch, b, sl])
    assert np.array_equal(prof["bin_pos"].to_numpy(), (2 * b + 1) / N - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(count[b, sl] > 0, sums[ch, b, sl].astype(np.float64) / count[b, sl], np.nan)
    assert np.array_equal(prof["mean"].to_numpy(), mean, equal_nan=True) and np.isnan(mean).any()
    one = cells.cell_profiles(lab.astype(np.int32), img, channels=[1], bins=2)
    assert set(one["channel"]) == {1} and len(one) == len(df) * 2
    with pytest.raises(ValueError):
        cells.measure_cells(lab, profile=N)
    with pytest.raises(ValueError):
        cells.measure_cells(lab, img, channels=[], profile=N)
    with pytest.raises(ValueError):
        cells.measure_cells(lab, img, profile=33)
    with pytest.raises(ValueError):
        cells.cell_profiles(lab, img, bins=1)


def test_stack_without_cells_gives_empty_tables():
    """a blank field of view, and a movie in which nothing is segmented: the flag must not stop what --cells alone writes"""
    from microbeseg_amd.inference import cells
    # the single frame without links: linking one frame without a cell is refused with or without the flag (no workspace)
    for lab, link in ((np.zeros((2, 7, 66), np.uint16), True), (np.zeros((1, 5, 5), np.int32), False)):
        img = image(np.uint16, (lab.shape[0], 2) + lab.shape[1:], seed=4)
        plain = cells.measure_cells(lab, img, link=link)
        assert len(plain) == 0
        for N in (2, 16, 32):
            df = cells.measure_cells(lab, img, link=link, profile=N)
            assert len(df) == 0 and list(df.columns) == cells.columns([0, 1], link, profile=True)
            assert list(df.columns)[:len(plain.columns)] == list(plain.columns)
            prof = cells.cell_profiles(lab, img, bins=N)
            assert len(prof) == 0 and list(prof.columns) == cells.PROFILE_TABLE_COLUMNS
    # one empty frame beside a frame with a cell: rows of the second frame only
    lab = np.zeros((2, 7, 66), np.uint16)
    lab[1, 2:5, 3:40] = 1
    img = image(np.uint16, (2, 1, 7, 66), seed=5)
    df = cells.measure_cells(lab, img, profile=8)
    assert df["frame"].tolist() == [1] and df["axis_extent"].tolist() == [37.0]
    assert cells.cell_profiles(lab, img, bins=8)["frame"].tolist() == [1] * 8


def rod_stack():
    """one horizontal rod of 40 x 7 pixels per frame, image [2, 1, 24, 64] uint16 on a dark background: frame 0 with bright
    outer quarters (polar caps), frame 1 with a bright band at mid-cell"""
    lab = np.zeros((2, 24, 64), np.uint16)
    lab[:, 8:15, 10:50] = 1
    img = np.full((2, 1, 24, 64), 100, np.uint16)
    img[0, 0, 8:15, 10:18], img[0, 0, 8:15, 42:50] = 900, 900
    img[1, 0, 8:15, 26:34] = 900
    return lab, img


def test_polar_caps_and_a_mid_cell_band():
    from microbeseg_amd.inference import cells
    lab, img = rod_stack()
    df = cells.measure_cells(lab, img, profile=16)
    assert df["orientation"].abs().sub(math.pi / 2).abs().max() < 1e-12 and df["axis_extent"].tolist() == [40.0, 40.0]
    caps, band = df.iloc[0], df.iloc[1]
    assert caps["pole_mid_ratio_ch0"] > 1 and abs(caps["profile_peak_ch0"]) > 0.5 and caps["pole_asym_ch0"] == 0
    assert band["pole_mid_ratio_ch0"] < 1 and abs(band["profile_peak_ch0"]) < 0.5 and band["pole_asym_ch0"] == 0
    assert caps["pole_mid_ratio_ch0"] == (900 * 8 + 100 * 2) / 10 / ((100 * 20) / 20)             # pole bins 0 .. 3 and 12 .. 15
    prof = cells.cell_profiles(lab, img, bins=16)
    first = prof[(prof["frame"] == 0)]["mean"].tolist()
    assert first[:3] == [900.0] * 3 and first[-3:] == [900.0] * 3 and first[7] == first[8] == 100.0


def test_infer_worker_names_the_columns_by_source_channel():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab = scene(33, 200, 4)[0].astype(np.uint16)
    img = measured(33, 200, 4, np.uint16, 3)[0]
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    assert worker.profile is None
    view = img[:, [2, 0]]
    plain = worker.cell_table(lab, view, channels=(2, 0))
    assert list(plain.columns) == cells.columns([2, 0], link=True)
    worker.profile = 8
    df = worker.cell_table(lab, view, channels=(2, 0))
    assert list(df.columns) == cells.columns([2, 0], link=True, profile=True)
    pd.testing.assert_frame_equal(df[list(plain.columns)], plain, check_exact=True)
    want = cells.measure_cells(lab, img, channels=[2, 0], profile=8)
    pd.testing.assert_frame_equal(df, want, check_exact=True)
    prof = worker.profile_table(lab, view, channels=(2, 0))
    assert list(prof.columns) == cells.PROFILE_TABLE_COLUMNS and sorted(set(prof["channel"])) == [0, 2]
    direct = cells.cell_profiles(lab, img, channels=[2, 0], bins=8)
    assert prof["channel"].tolist() == direct["channel"].tolist()
    pd.testing.assert_frame_equal(prof, direct, check_exact=True)


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_infer_script_profile_end_to_end(tmp_path):
    import subprocess
    import sys
    from microbeseg_amd.inference.cells import PROFILE_TABLE_COLUMNS, cell_profiles, columns, measure_cells
    from microbeseg_amd.utils import synth, tiffio
    from test_cells_host import ROOT
    from test_gpu_analysis import _constant_distance_model
    model = _constant_distance_model(tmp_path / "distance_model_00")      # one cell per frame, whatever the input
    rng = np.random.Generator(np.random.PCG64(9))
    stack = np.stack([synth.synth_crop(rng, 128)["img"] for _ in range(2)])
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    tiffio.imwrite(str(imgs / "movie.tif"), stack)
    tiffio.imwrite(str(imgs / "movie_f32.tif"), stack.astype(np.float32))
    res = tmp_path / "results"
    cmd = [sys.executable, str(ROOT / "infer_script_local.py"), "-i", str(imgs), "-m", str(model), "-r", str(res), "--cells",
           "--profile"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Cell table: with the intensity profile of every cell along its axis in 16 bins" in r.stdout
    read = lambda name: pd.read_csv(res / name, float_precision="round_trip")
    mask = tiffio.imread(str(res / "mask_movie_channel0.tif"))
    df = read("mask_movie_channel0_cells.csv")
    assert list(df.columns) == columns([0], link=True, profile=True)
    pd.testing.assert_frame_equal(df, measure_cells(mask, stack, profile=16), check_exact=True, check_dtype=False)
    prof = read("mask_movie_channel0_profiles.csv")
    assert list(prof.columns) == PROFILE_TABLE_COLUMNS and len(prof) == len(df) * 16
    pd.testing.assert_frame_equal(prof, cell_profiles(mask, stack, bins=16), check_exact=True, check_dtype=False)
    # no intensity view: the profile is switched off for that stack, like the spot columns
    assert list(read("mask_movie_f32_channel0_cells.csv").columns) == columns([], link=True)
    assert not (res / "mask_movie_f32_channel0_profiles.csv").exists()
