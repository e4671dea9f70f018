"""GPU (MI355X): the per-cell fluorescent foci (csrc/spots.hip) through the C ABI, through spots_raw /
measure_cells / cell_spots and through the command line, every integer equal to the restatement tests/spots_ref.py (which
test_spots_host.py checks on the CPU).  All comparisons are exact: the only floats are single divisions of exact integers."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
import spots_ref as sref
from test_gpu_cells import PIX, Guarded, _dev
from test_hull_host import random_cells
from test_spots_host import SPOT_COLUMNS, SPOT_TABLE_COLUMNS, saturated_planes

pytestmark = pytest.mark.gpu
EINVAL, EWORKSPACE = -1, -3
TILE_H, TILE_W = 32, 64                 # SP_TH, SP_TW of csrc/spots.hip
H, W, T = 70, 130, 2                    # ragged tiles in both directions: seams at rows 32, 64 and columns 64, 128
THR = {np.dtype(np.uint8): 4, np.dtype(np.uint16): 900}
RECORD = np.dtype([("frame", "<i4"), ("channel", "<i4"), ("y", "<i4"), ("x", "<i4"), ("label", "<i4"), ("value", "<i4"),
                   ("d", "<i8")])


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def c_spots(lab, off, img, s, thr, cap=None, base=None, strides=None, nch=None, short=0, label_code=None, img_code=None,
            no_list=False, null=()):
    """mseg_cell_spots through ctypes.  img: uint8 / uint16 [T, C, H, W] (contiguous), or ``base`` = the image's memory (any
    shape) with the element ``strides`` (frame, channel, row, pixel) of channel 0 and ``nch`` channels.  -> (return code,
    guarded cell_count [C, n], bg_count [T, C], list [cap, 4] int64, n_spots [1], status [1]); by default with room for
    every spot the frames can hold"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    Tn, Hn, Wn = lab.shape
    n = int(off[-1])
    if base is None:
        base, nch = np.ascontiguousarray(img), img.shape[1]
        strides = (nch * Hn * Wn, Hn * Wn, Wn, 1)
    cap = Tn * nch * ((Hn + 1) // 2) * ((Wn + 1) // 2) if cap is None else cap
    lab_d, off_d, img_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda(), _dev(np.array(base))
    cell, bg = Guarded((nch, n), torch.int32), Guarded((Tn, nch), torch.int32)
    lst, found, status = Guarded((max(cap, 1), 4), torch.int64), Guarded((1,), torch.int64), Guarded((1,), torch.int32)
    nbytes = lib.mseg_cell_spots_workspace_bytes(Tn, n, max(nch, 1))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ptr = lambda name, p: None if name in null else p
    code = lib.mseg_cell_spots(ptr("labels", lab_d.data_ptr()), PIX[lab.dtype] if label_code is None else label_code, Tn, Hn,
                               Wn, ptr("off", off_d.data_ptr()), n, ptr("img", img_d.data_ptr()),
                               PIX[base.dtype] if img_code is None else img_code, nch, *strides, s, thr, ptr("cell", cell.ptr),
                               ptr("bg", bg.ptr), None if no_list else ptr("list", lst.ptr), 0 if no_list else cap,
                               ptr("found", found.ptr), ptr("status", status.ptr), ptr("ws", ws.data_ptr()), nbytes - short,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code, cell, bg, lst, found, status


def sort_records(r):
    return r[np.lexsort((r["x"], r["y"], r["channel"], r["frame"]))]


def as_records(rows):
    return np.array([tuple(r) for r in rows], RECORD)


def spots_of(lab, off, img, s, thr, **kw):
    """the valid outputs of one call: (cell_count, bg_count, the records sorted)"""
    code, cell, bg, lst, found, status = c_spots(lab, off, img, s, thr, **kw)
    assert code == 0 and status.host(np.int32)[0] == 0
    m = int(found.host(np.int64)[0])
    raw = lst.host(np.int64)
    assert m <= raw.shape[0] and not raw[m:].any()              # zeros behind the last record
    return cell.host(np.int32), bg.host(np.int32), sort_records(raw.reshape(-1).view(RECORD)[:m])


def check(got, want):
    cell, bg, recs = got
    assert np.array_equal(cell, want[0]) and np.array_equal(bg, want[1])
    assert recs.tobytes() == as_records(want[2]).tobytes(), (len(recs), len(want[2]))


def _blob(img, t, c, y, x, amp, sigma=1.2):
    yy, xx = np.mgrid[:img.shape[2], :img.shape[3]]
    g = amp * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * sigma * sigma))
    img[t, c] = np.minimum(img[t, c].astype(np.int64) + np.rint(g).astype(np.int64), np.iinfo(img.dtype).max)


# blobs whose centre is the last row / column of a tile (frame 0) or the first of the next one (frame 1), in the four corners
# and on the borders; two blobs of one plane are at least 6 pixels apart, so each stays a peak of its own up to s = 2
LAST = [(y, x) for y in (5, 31, 63) for x in (5, 63, 100, 127)] + \
       [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 30), (45, 0), (45, W - 1), (H - 1, 90)]
FIRST = [(y, x) for y in (12, 32, 64) for x in (20, 64, 128)] + [(0, 90), (H - 1, 40), (50, 0), (22, W - 1)]
SEAM_SPOTS = [(0,) + p for p in LAST] + [(1,) + p for p in FIRST]


@functools.lru_cache(maxsize=None)
def labels():
    lab = random_cells(H, W, T=T, seed=11)
    off = ref.frame_tables(lab)
    lab.setflags(write=False)
    off.setflags(write=False)
    return lab, off


@functools.lru_cache(maxsize=None)
def image(dtype):
    """[T, 2, H, W]: (0, 0) and (1, 0) noise and blobs of several widths on every tile seam, in the corners and on the
    borders; (0, 1) four grey levels at random: ties everywhere; (1, 1) flat, with plateaus of two and four equal pixels that
    straddle the seams, and single pixels in the corners"""
    dtype = np.dtype(dtype)
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(21)
    img = np.zeros((T, 2, H, W), dtype)
    for t in range(T):
        img[t, 0] = rng.integers(0, top // 40, (H, W))
    for i, (t, y, x) in enumerate(SEAM_SPOTS):
        _blob(img, t, 0, y, x, top * 0.6, (0.8, 1.0, 1.2)[i % 3])
    img[0, 1] = rng.integers(0, 4, (H, W)) * (top // 4)
    img[1, 1] = top // 10
    for pixels in ([(31, 10), (32, 10)], [(10, 63), (10, 64)], [(31, 63), (31, 64), (32, 63), (32, 64)],
                   [(63, 127), (64, 128)], [(64, 100), (63, 101)], [(50, 127), (50, 128)], [(H - 1, 20), (H - 1, 21)],
                   [(0, 0)], [(0, W - 1)], [(H - 1, 0)], [(H - 1, W - 1)], [(20, 0), (21, 0)]):
        for y, x in pixels:
            img[1, 1, y, x] = top // 2
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(dtype, s):
    lab, off = labels()
    want = sref.reference(lab, off, image(dtype), [0, 1], THR[np.dtype(dtype)], s)
    assert len(want[2]) >= 36 and want[0].any() and want[1].all(), (len(want[2]), want[1])
    return want


# ---- against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("s", [1, 2, 5])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_outputs_equal_the_restatement(dtype, s, label_dtype):
    lab, off = labels()
    want = expected(dtype, s)
    check(spots_of(lab.astype(label_dtype), off, image(dtype), s, THR[np.dtype(dtype)]), want)
    found = {(r[0], r[1], r[2], r[3]) for r in want[2]}
    if s <= 2:
        assert all((t, 0, y, x) in found for t, y, x in SEAM_SPOTS)         # every planted spot, at its pixel
    for first in ((31, 10), (10, 63), (31, 63), (63, 127), (63, 101), (50, 127), (H - 1, 20), (0, 0), (0, W - 1), (H - 1, 0),
                  (H - 1, W - 1), (20, 0)):
        if s <= 2:
            assert (1, 1) + first in found                                    # the first pixel of every plateau


def test_saturated_planes_at_scale_5():
    hole, peak = saturated_planes(40, 70)                        # two tiles side by side and one below
    img = np.stack([hole, peak])[None]                           # [1, 2, H, W]
    lab = np.zeros((1, 40, 70), np.uint16)
    lab[0, 15:25, 30:45] = 1
    off = np.array([0, 1], np.int64)
    want = sref.reference(lab, off, img, [0, 1], 1, 5)
    assert [r[1:4] for r in want[2] if r[1] == 1] == [(1, 20, 36)] and want[2][-1][6] > 2 ** 50
    check(spots_of(lab, off, img, 5, 1), want)
    check(spots_of(lab, off, img, 5, 65535), sref.reference(lab, off, img, [0, 1], 65535, 5))


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (1, 7), (33, 65)])
def test_frames_smaller_than_the_halo(shape):
    rng = np.random.default_rng(shape[0])
    for dtype, top in ((np.uint8, 256), (np.uint16, 65536)):
        img = rng.integers(0, top, (2, 1) + shape).astype(dtype)
        lab = rng.integers(0, 3, (2,) + shape).astype(np.int32)
        off = np.array([0, 2, 4], np.int64)
        for s in (1, 3, 5):
            want = sref.reference(lab, off, img, [0], 1, s)
            assert len(want[2]) > 0 or shape == (1, 1)
            check(spots_of(lab, off, img, s, 1), want)


def test_strided_views_are_read_in_place():
    lab, off = labels()
    rng = np.random.default_rng(5)
    src = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)    # one [H, W, 3] frame: channels interleaved
    for _, y, x in SEAM_SPOTS[::3]:
        src[y, x] = 65535
    view = np.ascontiguousarray(src.transpose(2, 0, 1))[None]   # the same numbers as [1, 3, H, W]
    want = sref.reference(lab[:1], off[:2], view, [0, 1, 2], 2000, 2)
    assert len(want[2]) > 30
    check(spots_of(lab[:1].astype(np.uint16), off[:2], None, 2, 2000, base=src, strides=(0, 1, 3 * W, 3), nch=3), want)
    planes = np.ascontiguousarray(src.transpose(2, 0, 1))       # [3, H, W]: a channel stride of H * W, no frame stride
    check(spots_of(lab[:1].astype(np.uint16), off[:2], None, 2, 2000, base=planes, strides=(0, H * W, W, 1), nch=3), want)
    wide = np.zeros((T, 2, H, W + 9), np.uint8)                  # rows longer than the frame is wide
    wide[..., :W] = image(np.uint8)
    check(spots_of(lab.astype(np.int32), off, None, 1, THR[np.dtype(np.uint8)], base=wide,
                   strides=(2 * H * (W + 9), H * (W + 9), W + 9, 1), nch=2), expected(np.uint8, 1))


def test_only_channel_1_of_a_stack_is_measured():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab, off = labels()
    img = image(np.uint16)
    want = sref.reference(lab, off, img, [1], THR[np.dtype(np.uint16)], 2)
    lab_d = _dev(lab.astype(np.uint16))
    dev_img = cells._image_to_device(img, lab.shape, lab_d.device)
    cell, bg, recs = cells.spots_raw(lab_d, _lib.PIX_U16, off, dev_img, [1], THR[np.dtype(np.uint16)], 2)
    assert cell.dtype == bg.dtype == np.int32 and recs.dtype == cells.SPOT_RECORD == RECORD
    check((cell, bg, recs), want)
    both = cells.spots_raw(lab_d, _lib.PIX_U16, off, dev_img, [1, 0], THR[np.dtype(np.uint16)], 2)      # two calls: two groups
    check(both, sref.reference(lab, off, img, [1, 0], THR[np.dtype(np.uint16)], 2))


def test_no_cells_and_labels_beyond_the_table():
    lab64, off = labels()
    img = image(np.uint8)
    thr = THR[np.dtype(np.uint8)]
    none = np.zeros(T + 1, np.int64)                             # no cells at all: every label is beyond the table
    want = sref.reference(lab64, none, img, [0, 1], thr, 2)
    assert want[0].shape == (2, 0) and len(want[2]) == len(expected(np.uint8, 2)[2])
    code, cell, bg, lst, found, status = c_spots(lab64.astype(np.uint16), none, img, 2, thr, null=("cell",))
    assert code == 0 and cell.untouched() and np.array_equal(bg.host(np.int32), want[1])
    assert int(found.host(np.int64)[0]) == len(want[2])
    lab = np.array(lab64, np.int32)
    lab[1] = 0                                                   # a frame without cells, inside a stack with some
    k0 = int(off[1])
    lab[0, 28:36, 60:70] = k0 + 5                                # beyond the table, under planted spots
    lab[0, 60:68, 120:130] = -3
    short = np.array([0, k0 - 4, k0 - 4], np.int64)             # the last four ids of frame 0 are no cells either
    want = sref.reference(lab, short, img, [0, 1], thr, 2)
    assert {r[4] for r in want[2]} >= {k0 + 5, -3} and want[1][1].sum() == sum(r[0] == 1 for r in want[2])
    assert want[0].sum() + want[1].sum() < len(want[2])         # spots that are neither a cell's nor background
    check(spots_of(lab, short, img, 2, thr), want)


# ---- the list is too short ----------------------------------------------------------------------------------------------------------
def test_short_list_sets_the_status_word_and_the_wrapper_redoes_the_call():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab64, off = labels()
    lab, img, thr = lab64.astype(np.uint16), image(np.uint16), THR[np.dtype(np.uint16)]
    want = expected(np.uint16, 2)
    assert len(want[2]) > 36
    for cap in (1, 10):
        code, cell, bg, lst, found, status = c_spots(lab, off, img, 2, thr, cap=cap)
        assert code == 0 and status.host(np.int32)[0] != 0 and int(found.host(np.int64)[0]) == len(want[2])
        assert np.array_equal(cell.host(np.int32), want[0]) and np.array_equal(bg.host(np.int32), want[1])
        some = lst.host(np.int64).reshape(-1).view(RECORD)       # asserts the guard bands; every record written is a spot
        assert len({tuple(r) for r in some.tolist()}) == cap and all(tuple(r) in set(want[2]) for r in some.tolist())
    code, cell, bg, lst, found, status = c_spots(lab, off, img, 2, thr, no_list=True)
    assert code == 0 and lst.untouched() and status.host(np.int32)[0] != 0
    assert int(found.host(np.int64)[0]) == len(want[2]) and np.array_equal(cell.host(np.int32), want[0])
    lab_d = _dev(lab)
    dev_img = cells._image_to_device(img, lab.shape, lab_d.device)
    for cap in (1, 0, None, 10 ** 6):
        check(cells.spots_raw(lab_d, _lib.PIX_U16, off, dev_img, [0, 1], thr, 2, spot_cap=cap), want)


def test_two_calls_give_identical_bytes():
    lab, off = labels()
    lab, img = lab.astype(np.uint16), image(np.uint16)
    a, b = (spots_of(lab, off, img, 5, THR[np.dtype(np.uint16)]) for _ in range(2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    check(a, expected(np.uint16, 5))


def test_argument_errors_touch_nothing():
    from microbeseg_amd import _lib
    lib = _lib.load()
    lab, off = labels()
    lab, img = lab.astype(np.uint16), image(np.uint8)
    bad_calls = [dict(s=0), dict(s=6), dict(s=-1), dict(thr=0), dict(thr=65536), dict(thr=-5), dict(label_code=0),
                 dict(label_code=3), dict(img_code=2), dict(img_code=3), dict(cap=-1), dict(nch=0)] + \
                [dict(null=(name,)) for name in ("labels", "off", "img", "cell", "bg", "list", "found", "status", "ws")]
    for kw in bad_calls:
        extra = dict(base=np.array(img), strides=(2 * H * W, H * W, W, 1)) if "nch" in kw else {}
        code, *bufs = c_spots(lab, off, img, kw.pop("s", 2), kw.pop("thr", 50), **kw, **extra)
        assert code == EINVAL and all(b.untouched() for b in bufs), kw
    code, *bufs = c_spots(lab, off, img, 2, 50, short=1)
    assert code == EWORKSPACE and all(b.untouched() for b in bufs)
    n = int(off[-1])
    assert lib.mseg_cell_spots_workspace_bytes(0, n, 2) == 0 and lib.mseg_cell_spots_workspace_bytes(2, -1, 2) == 0
    assert lib.mseg_cell_spots_workspace_bytes(2, n, 0) == 0 and lib.mseg_cell_spots_workspace_bytes(2, n, 2) > 0


# ---- measure_cells(spots=...), cell_spots ---------------------------------------------------------------------------------------------
def spot_columns(channels):
    return [name.format(c=c) for c in channels for name in SPOT_COLUMNS]


def test_measure_cells_with_spots():
    from microbeseg_amd.inference import cells
    lab64, off = labels()
    lab, img, thr = lab64.astype(np.uint16), image(np.uint16), THR[np.dtype(np.uint16)]
    for s in (2, 5):
        want = expected(np.uint16, s)
        df = cells.measure_cells(lab, img, spots=thr, spot_scale=s)
        assert list(df.columns) == cells.columns([0, 1], True, spots=True) and len(df) > 100
        table = cells.table_from_sums(off, H, W, ref.measure(lab, off, img), channels=[0, 1], links=ref.links(lab, off),
                                      spots=(s, want[0], want[1], as_records(want[2])))
        pd.testing.assert_frame_equal(df, table, check_exact=True)
        unit = 16 ** (2 * s)
        for ci in (0, 1):                                        # the floats: one division of an exact integer each
            on_cells = [r for r in want[2] if r[1] == ci and r[4] > 0]
            assert df[f"n_spots_ch{ci}"].sum() == len(on_cells) > 0
            bg = df.groupby("frame")[f"bg_spots_ch{ci}"].agg(["min", "max"])
            assert (bg["min"] == bg["max"]).all() and bg["min"].tolist() == want[1][:, ci].tolist()
            assert df[f"n_spots_ch{ci}"].sum() + bg["min"].sum() == sum(r[1] == ci for r in want[2])
            for _, row in df[df[f"n_spots_ch{ci}"] > 0].head(20).iterrows():
                mine = [r[6] for r in on_cells if r[0] == row["frame"] and r[4] == row["label"]]
                assert len(mine) == row[f"n_spots_ch{ci}"]
                assert row[f"spot_max_ch{ci}"] == max(mine) / unit and row[f"spot_sum_ch{ci}"] == sum(mine) / unit
            none = df[df[f"n_spots_ch{ci}"] == 0]
            assert len(none) > 0 and none[f"spot_max_ch{ci}"].isna().all() and (none[f"spot_sum_ch{ci}"] == 0).all()
    plain = cells.measure_cells(lab, img)                        # the keywords off: the frame of before
    assert list(plain.columns) == cells.columns([0, 1], True)
    assert plain.to_csv().encode() == cells.measure_cells(lab, img, spots=None, spot_scale=5).to_csv().encode()
    pd.testing.assert_frame_equal(df[list(plain.columns)], plain, check_exact=True)      # on: columns appended, no more
    assert list(df.columns)[len(plain.columns):] == spot_columns([0, 1])
    assert cells.measure_cells(lab.astype(np.int32), img, spots=thr, spot_scale=5).to_csv().encode() == df.to_csv().encode()
    one = cells.measure_cells(lab, img, channels=[1], link=False, percentiles=(50,), neighbors=2, spots=thr, spot_scale=5)
    assert list(one.columns) == cells.columns([1], False, percentiles=(50,), neighbors=True, spots=True)
    assert one[spot_columns([1])].equals(df[spot_columns([1])])
    with pytest.raises(ValueError, match="spots are taken of an image's channels: none is measured"):
        cells.measure_cells(lab, img, channels=[], spots=thr)
    with pytest.raises(ValueError, match="only uint8 / uint16"):
        cells.measure_cells(lab, img.astype(np.float32), spots=thr)


def test_cell_spots():
    from microbeseg_amd.inference import cells
    lab64, off = labels()
    img, thr = image(np.uint8), THR[np.dtype(np.uint8)]
    want = expected(np.uint8, 2)
    raw = ref.measure(lab64, off)
    for lab in (lab64.astype(np.uint16), torch.from_numpy(lab64.astype(np.int32)).cuda()):
        full = cells.cell_spots(lab, img, spots=thr, background=True)                  # the default scale is 2
        assert list(full.columns) == SPOT_TABLE_COLUMNS and len(full) == len(want[2])
        table = cells.spots_from_records(as_records(want[2]), 2, off, raw, [0, 1], background=True)
        pd.testing.assert_frame_equal(full, table, check_exact=True)
        assert full[["frame", "channel", "y", "x", "label", "value"]].to_numpy().tolist() == [list(r[:6]) for r in want[2]]
        assert full["response"].tolist() == [r[6] / 16 ** 4 for r in want[2]]
        on_cells = cells.cell_spots(lab, img, spots=thr)
        assert on_cells.equals(full[full["label"] != 0].reset_index(drop=True)) and 0 < len(on_cells) < len(full)
        assert full[full["label"] == 0]["axis_pos"].isna().all() and on_cells["axis_pos"].notna().any()
    only = cells.cell_spots(lab64.astype(np.uint16), img, channels=[1], spots=thr, background=True)
    assert only.equals(full[full["channel"] == 1].reset_index(drop=True))
    df = cells.measure_cells(lab64.astype(np.uint16), img, link=False, spots=thr)
    for ci in (0, 1):
        assert df[f"n_spots_ch{ci}"].sum() + df.groupby("frame")[f"bg_spots_ch{ci}"].first().sum() == (full["channel"] == ci).sum()
    with pytest.raises(ValueError, match="spots"):
        cells.cell_spots(lab64.astype(np.uint16), img, spots=0)


def test_infer_worker_passes_spots_on():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab = labels()[0].astype(np.uint16)
    img, thr = image(np.uint8), THR[np.dtype(np.uint8)]
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    assert worker.spots is None and worker.spot_scale == 2
    assert list(worker.cell_table(lab, img).columns) == cells.columns([0, 1], link=True)
    worker.spots, worker.spot_scale = thr, 1
    df = worker.cell_table(lab, img)
    assert df.equals(cells.measure_cells(lab, img, spots=thr, spot_scale=1))
    named = worker.cell_table(lab, img[:, 1:], channels=[3])     # a view of the chosen channel, named by its source
    assert list(named.columns) == cells.columns([3], True, spots=True)
    assert named["n_spots_ch3"].equals(df["n_spots_ch1"]) and named["spot_sum_ch3"].equals(df["spot_sum_ch1"])
    spots = worker.spot_table(lab, img)
    assert spots.equals(cells.cell_spots(lab, img, spots=thr, spot_scale=1)) and len(spots) > 0
    assert set(worker.spot_table(lab, img[:, 1:], channels=[3])["channel"]) == {3}


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_infer_script_spots_end_to_end(tmp_path):
    import subprocess
    import sys
    from microbeseg_amd.inference.cells import cell_spots, columns, measure_cells
    from microbeseg_amd.utils import synth, tiffio
    from test_cells_host import ROOT
    from test_gpu_analysis import _constant_distance_model
    model = _constant_distance_model(tmp_path / "distance_model_00")      # one cell per frame, whatever the input
    rng = np.random.Generator(np.random.PCG64(9))
    stack = np.stack([synth.synth_crop(rng, 128)["img"] for _ in range(2)])
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    tiffio.imwrite(str(imgs / "movie.tif"), stack)
    out = tmp_path / "flagged"
    cmd = [sys.executable, str(ROOT / "infer_script_local.py"), "-i", str(imgs), "-m", str(model), "--cells", "-r", str(out)]
    r = subprocess.run(cmd + ["--spots", "50"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Cell table: with the fluorescent foci of every cell (response >= 50 grey levels at scale 2)" in r.stdout
    assert sorted(p.name for p in out.iterdir()) == ["mask_movie_channel0.tif", "mask_movie_channel0_cells.csv",
                                                     "mask_movie_channel0_spots.csv"]
    mask = tiffio.imread(str(out / "mask_movie_channel0.tif"))
    read = lambda path: pd.read_csv(path, float_precision="round_trip")
    df = read(out / "mask_movie_channel0_cells.csv")
    assert list(df.columns) == columns([0], True, spots=True)
    pd.testing.assert_frame_equal(df, measure_cells(mask, stack, spots=50), check_exact=True, check_dtype=False)
    old = measure_cells(mask, stack)
    pd.testing.assert_frame_equal(df[list(old.columns)], old, check_exact=True, check_dtype=False)
    spots = read(out / "mask_movie_channel0_spots.csv")
    assert list(spots.columns) == SPOT_TABLE_COLUMNS
    pd.testing.assert_frame_equal(spots, cell_spots(mask, stack, spots=50), check_exact=True, check_dtype=False)
    assert len(spots) == df["n_spots_ch0"].sum() and (spots["response"] >= 50).all() and (spots["label"] > 0).all()
