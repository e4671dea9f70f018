"""GPU (MI355X): the per-cell order statistics (csrc/order_stats.hip) through the C ABI and through
measure_cells, every integer equal to the restatement tests/order_stats_ref.py (which test_order_stats_host.py checks against
np.percentile on the CPU).  Boxes, areas and background counts come from tests/cells_ref.py, never from the code under test."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
import order_stats_ref as oref
from test_gpu_cells import PIX, Guarded, _dev, scene_a
from test_hull_host import random_cells

pytestmark = pytest.mark.gpu
EINVAL, EWORKSPACE = -1, -3
SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (33, 200), (70, 131)]
BG_SHARE = 65536          # OS_BG_SHARE of csrc/order_stats.hip: the pixels of a frame one workgroup of the background pass walks


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def tchw(img):
    T, Cn, H, W = img.shape
    return img, (Cn * H * W, H * W, W, 1)


def c_order(lab, off, base, strides, nch, bbox, ranks, bg_ranks, short=0, R=None, nch_arg=None, img_code=None, lab_code=None,
            HW=None):
    """mseg_cell_order_stats through ctypes.  base: the image's memory (any shape) with the element strides (frame, channel,
    row, pixel) of channel 0 -> (return code, guarded values [R, C, n], guarded bg_values [R, T, C], guarded status [1])"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    rows = len(bg_ranks)
    lab_d, off_d, img_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda(), _dev(np.array(base))
    bbox_d = torch.from_numpy(np.array(bbox, np.int32).reshape(-1, 4)).cuda()
    ranks_d = torch.from_numpy(np.array(ranks, np.int64).reshape(rows, n)).cuda()
    bg_d = torch.from_numpy(np.array(bg_ranks, np.int64).reshape(rows, T)).cuda()
    values, bg_values = Guarded((rows, nch, n), torch.int32), Guarded((rows, T, nch), torch.int32)
    status = Guarded((1,), torch.int32)
    nbytes = lib.mseg_cell_order_stats_workspace_bytes(T, n, nch, rows)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if HW is not None:
        H, W = HW
    code = lib.mseg_cell_order_stats(lab_d.data_ptr(), PIX[lab.dtype] if lab_code is None else lab_code, T, H, W,
                                     off_d.data_ptr(), n, img_d.data_ptr(), PIX[base.dtype] if img_code is None else img_code,
                                     nch if nch_arg is None else nch_arg, *(int(s) for s in strides),
                                     bbox_d.data_ptr() if n else None, rows if R is None else R,
                                     ranks_d.data_ptr() if n else None, bg_d.data_ptr(), values.ptr if n else None,
                                     bg_values.ptr, status.ptr, ws.data_ptr(), nbytes - short,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code, values, bg_values, status


def run(lab, off, img, bbox, ranks, bg_ranks, layout="contig"):
    """one valid call on the logical image img [T, C, H, W] laid out as ``layout`` -> (values, bg_values, status word)"""
    base, strides = laid_out(img, layout)
    code, values, bg_values, status = c_order(lab, off, base, strides, img.shape[1], bbox, ranks, bg_ranks)
    assert code == 0, code
    return values.host(np.uint32), bg_values.host(np.uint32), int(status.host(np.int32)[0])


def laid_out(img, layout):
    T, Cn, H, W = img.shape
    if layout == "contig":
        return tchw(img)
    if layout == "hwc":                                          # a [T, H, W, C] source viewed channel-first
        return np.ascontiguousarray(np.moveaxis(img, 1, -1)), (H * W * Cn, 1, W * Cn, Cn)
    if layout == "pitch":                                        # rows longer than W, the rest filled with another value
        base = np.full((T, Cn, H, W + 5), 199, img.dtype)
        base[..., :W] = img
        return base, (Cn * H * (W + 5), H * (W + 5), W + 5, 1)
    raise ValueError(layout)


def image(dtype, shape, seed=0):
    """[T, C, H, W]: channel 0 over the whole range, channel 1 in a narrow range around 255 / 256 (uint16: one or two high
    bytes, many ties), channel 2 in 0 .. 4095"""
    rng = np.random.default_rng(seed)
    T, Cn, H, W = shape
    top = 256 if dtype == np.uint8 else 65536
    img = np.zeros(shape, dtype)
    for c in range(Cn):
        lo, hi = ((0, top), (240, min(272, top)), (0, min(4096, top)))[c % 3]
        img[:, c] = rng.integers(lo, hi, (T, H, W))
    return img


def draw_ranks(count, R, seed):
    """[R, len(count)] ranks in 0 .. count - 1 (0 where count is 0); R > 1: row 0 is the first, row 1 the last rank"""
    rng = np.random.default_rng(seed)
    count = np.asarray(count, np.int64)
    r = rng.integers(0, np.maximum(count, 1), (R, len(count)))
    if R > 1:
        r[0], r[1] = 0, np.maximum(count - 1, 0)
    return r.astype(np.int64)


@functools.lru_cache(maxsize=None)
def scene(H, W, T):
    lab = random_cells(H, W, T=T, seed=3)
    off = ref.frame_tables(lab)
    lab.setflags(write=False)
    return lab, off


@functools.lru_cache(maxsize=None)
def measured(H, W, T, img_dtype, Cn):
    """(img, cells_ref.measure of it): read only"""
    lab, off = scene(H, W, T)
    img = image(img_dtype, (T, Cn, H, W), seed=H + W)
    img.setflags(write=False)
    return img, ref.measure(lab, off, img)


# ---- against the restatement --------------------------------------------------------------------------------------------------
COMBOS = [(1, 1, "contig", 1), (4, 3, "contig", 16), (4, 3, "hwc", 16), (1, 3, "hwc", 1), (4, 1, "pitch", 16),
          (1, 3, "pitch", 16), (4, 1, "contig", 1)]


@pytest.mark.parametrize("img_dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_values_equal_the_restatement(shape, label_dtype, img_dtype):
    H, W = shape
    for T, Cn, layout, R in COMBOS:
        lab, off = scene(H, W, T)
        img, raw = measured(H, W, T, img_dtype, Cn)
        area, bg_n = raw["shape"][0].astype(np.int64), raw["bg_sums"][0, :, 0].astype(np.int64)
        ranks, bg_ranks = draw_ranks(area, R, 1), draw_ranks(bg_n, R, 2)
        want_v, want_b, want_s = oref.order_stats(lab, off, img, raw["bbox"], ranks, bg_ranks)
        assert want_s == 0
        got_v, got_b, got_s = run(lab.astype(label_dtype), off, img, raw["bbox"], ranks, bg_ranks, layout)
        what = (T, Cn, layout, R)
        assert got_s == 0, what
        assert np.array_equal(got_v, want_v), what
        assert np.array_equal(got_b, want_b), what
        if R > 1:                                                # the first and the last rank are the extremes
            assert np.array_equal(got_v[0], raw["ch_minmax"][0]) and np.array_equal(got_v[1], raw["ch_minmax"][1]), what
            assert np.array_equal(got_b[0], raw["bg_minmax"][0]) and np.array_equal(got_b[1], raw["bg_minmax"][1]), what


# ---- hand-built cells ---------------------------------------------------------------------------------------------------------
def hand_scene():
    """one 96 x 96 frame, uint16 image; -> (labels int64, image [1, 1, 96, 96], ranks [16, K], the expected values [16, K])"""
    H = W = 96
    lab, img = np.zeros((1, H, W), np.int64), np.full((1, 1, H, W), 31000, np.uint16)
    ranks, expect = [], []

    def cell(pixels, values, rk, exp):
        assert len(pixels) == len(values) and len(rk) == len(exp) == 16
        k = len(ranks) + 1
        for (y, x), v in zip(pixels, values):
            assert lab[0, y, x] == 0
            lab[0, y, x], img[0, 0, y, x] = k, v
        ranks.append(rk)
        expect.append(exp)

    every = list(range(16))
    cell([(20, 20)], [777], [0] * 16, [777] * 16)                                                     # 1: one pixel
    cell([(22 + i // 4, 20 + i % 4) for i in range(16)], [300] * 16, every, [300] * 16)                # 2: one repeated value
    cell([(28, 20), (28, 21), (29, 20), (29, 21)], [65535, 0, 256, 255], [0, 1, 2, 3] * 4, [0, 255, 256, 65535] * 4)   # 3
    one_bin = [0x1200 + 7 * i for i in range(16)]                                                      # 4: all in bin 0x12
    cell([(32 + i // 4, 20 + i % 4) for i in range(16)], [one_bin[(5 * i) % 16] for i in range(16)], every, one_bin)
    assert one_bin[0] == 4608 and one_bin[-1] == 4713
    bins16 = [0x1000 * i + 5 + i for i in range(16)]                                                   # 5: 16 different bins
    cell([(38 + i // 4, 20 + i % 4) for i in range(16)], [bins16[(7 * i) % 16] for i in range(16)], every[::-1], bins16[::-1])
    assert bins16[1] == 4102 and bins16[-1] == 61460
    line = [1000 + 3 * i for i in range(65)]
    pick = [0, 1, 2, 3, 31, 32, 33, 60, 61, 62, 63, 64, 64, 0, 40, 20]
    want = [1000, 1003, 1006, 1009, 1093, 1096, 1099, 1180, 1183, 1186, 1189, 1192, 1192, 1000, 1120, 1060]
    cell([(3, 10 + i) for i in range(65)], [line[(11 * i) % 65] for i in range(65)], pick, want)       # 6: 1 x 65
    cell([(10 + i, 5) for i in range(65)], [line[(17 * i) % 65] for i in range(65)], pick, want)       # 7: 65 x 1
    for y0, x0, b in ((0, 0, 100), (0, W - 2, 200), (H - 2, 0, 60000), (H - 2, W - 2, 254)):            # 8 .. 11: the corners
        cell([(y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)], [b + 3, b + 1, b + 4, b + 2], [0, 1, 2, 3] * 4,
             [b + 1, b + 2, b + 3, b + 4] * 4)
    box = [(50 + y, 50 + x) for y in range(6) for x in range(6)]                                       # 12, 13: a checkerboard
    even, odd = [p for p in box if sum(p) % 2 == 0], [p for p in box if sum(p) % 2]
    cell(even, [100 + 10 * ((7 * i) % 18) for i in range(18)], every, [100 + 10 * i for i in range(16)])
    cell(odd, [40000 + 300 * ((5 * i) % 18) for i in range(18)], [17] + every[1:], [45100] + [40000 + 300 * i for i in range(1, 16)])
    parts = [(60, 70), (60, 71), (61, 70), (70, 80), (70, 81), (75, 60)]                               # 14: disconnected
    cell(parts, [513, 2, 511, 512, 65535, 1], [0, 1, 2, 3, 4, 5] * 2 + [5, 0, 3, 2], [1, 2, 511, 512, 513, 65535] * 2 + [65535, 1, 512, 511])
    return lab, img, np.array(ranks, np.int64).T.copy(), np.array(expect, np.uint32).T.copy()


@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
def test_hand_built_cells(label_dtype):
    lab, img, ranks, expect = hand_scene()
    off = ref.frame_tables(lab)
    assert int(off[-1]) == 14 == ranks.shape[1]
    raw = ref.measure(lab, off, img)
    assert raw["bbox"][5].tolist() == [3, 10, 4, 75] and raw["bbox"][6].tolist() == [10, 5, 75, 6]
    assert raw["bbox"][11].tolist() == raw["bbox"][12].tolist() == [50, 50, 56, 56]                  # one shared box
    bg_ranks = np.zeros((16, 1), np.int64)
    values, bg_values, status = run(lab.astype(label_dtype), off, img, raw["bbox"], ranks, bg_ranks)
    assert status == 0
    for k in range(14):
        assert values[:, 0, k].tolist() == expect[:, k].tolist(), f"cell {k + 1}"
    assert (bg_values == 31000).all()
    assert np.array_equal(values, oref.order_stats(lab, off, img, raw["bbox"], ranks, bg_ranks)[0])


# ---- absent ids, ids beyond the table, negative ids ------------------------------------------------------------------------------
@pytest.mark.parametrize("img_dtype", [np.uint8, np.uint16])
def test_absent_and_foreign_ids(img_dtype):
    lab, off = scene_a(np.int32)
    lab = lab.copy()
    lab[0][tuple(np.argwhere(lab[0] == 0)[40])] = -7
    lab[1][tuple(np.argwhere(lab[1] == 0)[-3])] = -2 ** 31
    img = image(img_dtype, (3, 2, 37, 53), seed=9)
    raw = ref.measure(lab, off, img)
    area = raw["shape"][0].astype(np.int64)
    assert area[2] == 0 and area[8] == 0 and (raw["bbox"][2] == 0).all()                             # ids 3 and 9 are absent
    bg_n = raw["bg_sums"][0, :, 0].astype(np.int64)
    assert bg_n[0] == 37 * 53 - int(((lab[0] > 0) | (lab[0] < 0)).sum())                             # foreign ids: not background
    ranks, bg_ranks = draw_ranks(area, 16, 3), draw_ranks(bg_n, 16, 4)
    ranks[:, 2] = [5, -1, 10 ** 12] + [0] * 13                                                       # not read as ranks
    want_v, want_b, want_s = oref.order_stats(lab, off, img, raw["bbox"], ranks, bg_ranks)
    got_v, got_b, got_s = run(lab, off, img, raw["bbox"], ranks, bg_ranks)
    assert got_s == want_s == 0
    assert np.array_equal(got_v, want_v) and np.array_equal(got_b, want_b)
    assert (got_v[:, :, [2, 8]] == 0).all() and (got_v[:, :, area > 0].astype(np.int64).sum(axis=(0, 1)) > 0).all()
    assert np.array_equal(got_b[0], raw["bg_minmax"][0]) and np.array_equal(got_b[1], raw["bg_minmax"][1])
    # frame 2 has no cells: background only there
    assert off[3] == off[2] and bg_n[2] == 37 * 53


# ---- background ---------------------------------------------------------------------------------------------------------------------
def test_frame_without_background():
    lab = np.zeros((2, 9, 70), np.int32)
    lab[0] = 1                                                    # no label-0 pixel in frame 0
    lab[1, 2:5, 3:60] = 1
    off = ref.frame_tables(lab)
    img = image(np.uint16, (2, 2, 9, 70), seed=1)
    raw = ref.measure(lab, off, img)
    bg_n = raw["bg_sums"][0, :, 0].astype(np.int64)
    assert bg_n[0] == 0 and bg_n[1] > 0
    ranks, bg_ranks = draw_ranks(raw["shape"][0].astype(np.int64), 16, 5), draw_ranks(bg_n, 16, 6)
    bg_ranks[:, 0] = [0, 5, -3, 10 ** 10] + [1] * 12             # not read as ranks
    want = oref.order_stats(lab, off, img, raw["bbox"], ranks, bg_ranks)
    got = run(lab, off, img, raw["bbox"], ranks, bg_ranks)
    assert got[2] == want[2] == 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[1][:, 0] == 0).all() and (got[1][1, 1] > 0).all()


@pytest.mark.parametrize("img_dtype", [np.uint8, np.uint16])
def test_background_merged_from_two_workgroups(img_dtype):
    H = W = 320
    assert BG_SHARE < H * W <= 2 * BG_SHARE                       # two workgroups per frame and channel
    lab = np.zeros((1, H, W), np.int32)
    lab[0, 150:170, 150:170] = 1
    n_bg = H * W - 400
    assert n_bg == 102000
    order = np.random.default_rng(8).permutation(n_bg)            # every workgroup sees values of the whole range
    img = np.zeros((1, 1, H, W), img_dtype)
    if img_dtype == np.uint16:
        img[0, 0][lab[0] == 0] = order // 2 + 7                   # 7 .. 51006, each twice
        first, last, mid_lo, mid_hi = 7, 51006, 25506, 25507
    else:
        img[0, 0][lab[0] == 0] = order * 251 // n_bg              # 0 .. 250
        first, last, mid_lo, mid_hi = 0, 250, 125, 125
    img[0, 0][lab[0] == 1] = 3
    off = np.array([0, 1], np.int64)
    bbox = np.array([[150, 150, 170, 170]], np.int32)
    bg_ranks = np.array([[0], [n_bg - 1], [50999], [51000]], np.int64)      # h = 101999 / 2: the two ranks of the median
    values, bg_values, status = run(lab, off, img, bbox, np.array([[0], [399], [7], [200]]), bg_ranks)
    assert status == 0 and (values == 3).all()
    assert bg_values[:, 0, 0].tolist() == [first, last, mid_lo, mid_hi]


# ---- status -------------------------------------------------------------------------------------------------------------------------
def test_rank_out_of_range_sets_the_status_word():
    lab, off = scene(33, 200, 4)
    img, raw = measured(33, 200, 4, np.uint16, 3)
    area, bg_n = raw["shape"][0].astype(np.int64), raw["bg_sums"][0, :, 0].astype(np.int64)
    s = int(np.flatnonzero(area > 3)[5])
    ranks, bg_ranks = draw_ranks(area, 16, 1), draw_ranks(bg_n, 16, 2)
    ranks[4, s] = area[s]                                         # one past the last
    want = oref.order_stats(lab, off, img, raw["bbox"], ranks, bg_ranks)
    got = run(lab.astype(np.int32), off, img, raw["bbox"], ranks, bg_ranks)      # .host() checks the guard bands
    assert want[2] == 1 and got[2] != 0
    assert (got[0][4, :, s] == 0).all() and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ranks[4, s] = 0
    ranks[9, s] = -1
    assert run(lab.astype(np.int32), off, img, raw["bbox"], ranks, bg_ranks)[2] != 0
    ranks[9, s] = 0
    bg_ranks[15, 2] = bg_n[2]
    got = run(lab.astype(np.uint16), off, img, raw["bbox"], ranks, bg_ranks)
    want = oref.order_stats(lab, off, img, raw["bbox"], ranks, bg_ranks)
    assert want[2] == 1 and got[2] != 0 and (got[1][15, 2] == 0).all() and np.array_equal(got[1], want[1])
    bg_ranks[15, 2] = 0
    assert run(lab.astype(np.uint16), off, img, raw["bbox"], ranks, bg_ranks)[2] == 0


def test_short_box_sets_the_status_word():
    lab = np.zeros((1, 12, 80), np.int32)
    lab[0, 2:7, 4:74] = 1
    lab[0, 8:10, 1:5] = 2
    off = ref.frame_tables(lab)
    img = image(np.uint16, (1, 1, 12, 80), seed=2)
    raw = ref.measure(lab, off, img)
    area = raw["shape"][0].astype(np.int64)
    ranks = np.array([[0, 0], [area[0] - 1, area[1] - 1]], np.int64)
    bg_ranks = np.zeros((2, 1), np.int64)
    assert run(lab, off, img, raw["bbox"], ranks, bg_ranks)[2] == 0
    bbox = raw["bbox"].copy()
    bbox[0, 2] -= 1                                               # one row short: area - 70 pixels are found
    want = oref.order_stats(lab, off, img, bbox, ranks, bg_ranks)
    got = run(lab, off, img, bbox, ranks, bg_ranks)
    assert want[2] == 1 and got[2] != 0 and got[0][1, 0, 0] == 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # a box that leaves the frame is clipped: nothing outside the arrays is read (the guard bands hold, the values stand)
    bbox = raw["bbox"].copy()
    bbox[0], bbox[1] = [-5, -5, 50, 500], [8, 1, 2 ** 31 - 1, 2 ** 31 - 1]
    got = run(lab, off, img, bbox, ranks, bg_ranks)
    assert got[2] == 0 and np.array_equal(got[0], oref.order_stats(lab, off, img, raw["bbox"], ranks, bg_ranks)[0])


# ---- bad arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_touch_nothing():
    from microbeseg_amd import _lib
    lib = _lib.load()
    lab, off = scene(5, 65, 1)
    lab = lab.astype(np.int32)
    img, raw = measured(5, 65, 1, np.uint16, 1)
    base, strides = tchw(img)
    n = int(off[-1])
    ranks, bg_ranks = np.zeros((16, n), np.int64), np.zeros((16, 1), np.int64)
    cases = {"R = 0": dict(R=0), "R = 17": dict(R=17), "C = 0": dict(nch_arg=0), "C = -1": dict(nch_arg=-1),
             "image dtype int32": dict(img_code=2), "image dtype fp32": dict(img_code=3), "image dtype 7": dict(img_code=7),
             "label dtype uint8": dict(lab_code=0), "label dtype 9": dict(lab_code=9),
             "H W too large": dict(HW=(46341, 46341)), "H = 0": dict(HW=(0, 65))}
    for what, kw in cases.items():
        code, values, bg_values, status = c_order(lab, off, base, strides, 1, raw["bbox"], ranks, bg_ranks, **kw)
        assert code == EINVAL, what
        assert values.untouched() and bg_values.untouched() and status.untouched(), what
    assert 46341 * 46341 >= 2 ** 31 - 512
    code, values, bg_values, status = c_order(lab, off, base, strides, 1, raw["bbox"], ranks, bg_ranks, short=1)
    assert code == EWORKSPACE and values.untouched() and bg_values.untouched() and status.untouched()
    size = lib.mseg_cell_order_stats_workspace_bytes
    for bad in ((0, 10, 1, 1), (1, -1, 1, 1), (1, 10, 0, 1), (1, 10, 1, 0), (1, 10, 1, 17)):
        assert size(*bad) == 0, bad
    assert size(1, n, 1, 16) > 0


def test_no_labels_measures_the_background_only():
    lab = np.zeros((2, 7, 66), np.uint16)
    lab[1, 3, 3] = 5                                              # beyond the empty table: neither cell nor background
    off = np.zeros(3, np.int64)
    img = image(np.uint16, (2, 3, 7, 66), seed=4)
    bg_n = np.array([7 * 66, 7 * 66 - 1], np.int64)
    bg_ranks = draw_ranks(bg_n, 16, 1)
    base, strides = laid_out(img, "hwc")
    code, values, bg_values, status = c_order(lab, off, base, strides, 3, np.zeros((0, 4)), np.zeros((16, 0)), bg_ranks)
    assert code == 0 and status.host(np.int32)[0] == 0
    want = oref.order_stats(lab, off, img, np.zeros((0, 4)), np.zeros((16, 0)), bg_ranks)
    assert want[2] == 0 and np.array_equal(bg_values.host(np.uint32), want[1])
    b = np.sort(img[1, 2][lab[1] == 0])
    assert bg_values.host(np.uint32)[1, 1, 2] == b[-1] and len(b) == bg_n[1]


# ---- determinism --------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    lab, off = scene(70, 131, 4)
    img, raw = measured(70, 131, 4, np.uint16, 3)
    ranks = draw_ranks(raw["shape"][0].astype(np.int64), 16, 1)
    bg_ranks = draw_ranks(raw["bg_sums"][0, :, 0].astype(np.int64), 16, 2)
    a = run(lab.astype(np.uint16), off, img, raw["bbox"], ranks, bg_ranks, "hwc")
    b = run(lab.astype(np.uint16), off, img, raw["bbox"], ranks, bg_ranks, "hwc")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_measure_cells_with_percentiles():
    from microbeseg_amd.inference import cells
    lab, off = scene(70, 131, 4)
    img = np.ascontiguousarray(measured(70, 131, 4, np.uint16, 3)[0][:, :2])
    pct = (5, 50, 95)
    plain = cells.measure_cells(lab, img)
    df = cells.measure_cells(lab, img, percentiles=pct)
    assert list(df.columns) == cells.columns([0, 1], True, percentiles=pct) == list(plain.columns) + [
        "p5_ch0", "p50_ch0", "p95_ch0", "p5_ch1", "p50_ch1", "p95_ch1",
        "bg_p5_ch0", "bg_p50_ch0", "bg_p95_ch0", "bg_p5_ch1", "bg_p50_ch1", "bg_p95_ch1"]
    pd.testing.assert_frame_equal(df[list(plain.columns)], plain, check_exact=True)
    assert cells.measure_cells(lab, img, percentiles=()).equals(plain) and cells.measure_cells(lab, img, percentiles=None).equals(plain)
    want = oref.percentile_columns(lab, img, [0, 1], pct)
    worst = 0.0
    for c in df.columns[len(plain.columns):]:
        assert df[c].dtype == np.float64 and np.array_equal(df[c].to_numpy(), np.array(want[c])), c
    for row in df.itertuples(index=False):
        m, b = lab[row.frame] == row.label, lab[row.frame] == 0
        for c in (0, 1):
            for P in pct:
                for got, v in ((getattr(row, f"p{P}_ch{c}"), img[row.frame, c][m]), (getattr(row, f"bg_p{P}_ch{c}"), img[row.frame, c][b])):
                    worst = max(worst, abs(got - float(np.percentile(v, P))))
    print(f"largest difference to np.percentile: {worst:.3e}")
    assert worst <= 1e-9
    # one channel of a strided view, uint8, with the other options
    img8 = image(np.uint8, (4, 3, 70, 131), seed=12)
    one = cells.measure_cells(lab.astype(np.int32), np.moveaxis(np.ascontiguousarray(np.moveaxis(img8, 1, -1)), -1, 1),
                              channels=[2], link=False, hull=True, midline=True, percentiles=[50])
    assert list(one.columns) == cells.columns([2], False, False, True, True, (50,))
    assert np.array_equal(one["p50_ch2"].to_numpy(), np.array(oref.percentile_columns(lab, img8, [2], (50,))["p50_ch2"]))
    with pytest.raises(ValueError):
        cells.measure_cells(lab, percentiles=pct)
    with pytest.raises(ValueError):
        cells.measure_cells(lab, img, channels=[], percentiles=pct)
    with pytest.raises(ValueError):
        cells.measure_cells(lab, img, percentiles=(50, 101))


def test_order_stats_raw_raises_on_a_short_box():
    from microbeseg_amd.inference import cells
    lab, off = scene(33, 200, 4)
    img, raw = measured(33, 200, 4, np.uint16, 3)
    dev = torch.device("cuda", torch.cuda.current_device())
    lab_d, pix = cells._labels_to_device(lab.astype(np.int32), dev)
    image_d = cells._image_to_device(img, lab.shape, dev)
    area, bg_n = raw["shape"][0].astype(np.int64), raw["bg_sums"][0, :, 0].astype(np.int64)
    ranks, bg_ranks = draw_ranks(area, 16, 1), draw_ranks(bg_n, 16, 2)
    values, bg_values = cells.order_stats_raw(lab_d, pix, off, image_d, [0, 2, 1], raw["bbox"], ranks, bg_ranks)
    want = oref.order_stats(lab, off, img[:, [0, 2, 1]], raw["bbox"], ranks, bg_ranks)
    assert values.dtype == bg_values.dtype == np.uint32
    assert np.array_equal(values, want[0]) and np.array_equal(bg_values, want[1])
    bbox = raw["bbox"].copy()
    s = int(np.flatnonzero(bbox[:, 2] - bbox[:, 0] > 1)[0])
    bbox[s, 0] += 1
    with pytest.raises(RuntimeError):
        cells.order_stats_raw(lab_d, pix, off, image_d, [0], bbox, ranks, bg_ranks)


def test_infer_worker_names_the_columns_by_source_channel():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab = scene(33, 200, 4)[0].astype(np.uint16)
    img = measured(33, 200, 4, np.uint16, 3)[0]
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    assert worker.percentiles is None
    view = img[:, [2, 0]]
    plain = worker.cell_table(lab, view, channels=(2, 0))
    assert list(plain.columns) == cells.columns([2, 0], link=True)
    worker.percentiles = (50, 95)
    df = worker.cell_table(lab, view, channels=(2, 0))
    assert list(df.columns) == list(plain.columns) + ["p50_ch2", "p95_ch2", "p50_ch0", "p95_ch0", "bg_p50_ch2", "bg_p95_ch2",
                                                      "bg_p50_ch0", "bg_p95_ch0"]
    pd.testing.assert_frame_equal(df[list(plain.columns)], plain, check_exact=True)
    want = oref.percentile_columns(lab, img, [2, 0], (50, 95))
    for c in df.columns[len(plain.columns):]:
        assert np.array_equal(df[c].to_numpy(), np.array(want[c])), c
