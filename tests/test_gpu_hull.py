"""GPU (MI355X): the per-cell outline measures (csrc/hull.hip) through the C ABI and through measure_cells,
every integer equal to the restatement tests/hull_ref.py (which test_hull_host.py checks on the CPU).  The bounding boxes the
kernels are given come from tests/cells_ref.py, never from the code under test."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
import hull_ref as href
from test_gpu_cells import PIX, Guarded, _dev
from test_hull_host import HULL_COLUMNS, random_cells

pytestmark = pytest.mark.gpu
EINVAL, EWORKSPACE = -1, -3
SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (33, 200), (70, 131)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rows_from(bbox):
    """row_off of the boxes: r1 - r0 + 1 corner rows for a present cell, none for an absent one"""
    bbox = np.asarray(bbox, np.int64).reshape(-1, 4)
    rows = np.where(bbox[:, 2] > bbox[:, 0], bbox[:, 2] - bbox[:, 0] + 1, 0)
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


def c_hull(lab, off, bbox, row_off=None, short=0, dtype_code=None):
    """mseg_cell_hull through ctypes -> (return code, guarded out [10, n], guarded status [1])"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    row_off = rows_from(bbox) if row_off is None else np.asarray(row_off, np.int64)
    n_rows = int(row_off[-1])
    lab_d, off_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda()
    bbox_d = torch.from_numpy(np.array(bbox, np.int32).reshape(-1, 4)).cuda()
    row_d = torch.from_numpy(np.array(row_off, np.int64)).cuda()
    out, status = Guarded((10, n), torch.int64), Guarded((1,), torch.int32)
    nbytes = lib.mseg_cell_hull_workspace_bytes(n, n_rows)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    code = lib.mseg_cell_hull(lab_d.data_ptr(), PIX[lab.dtype] if dtype_code is None else dtype_code, T, H, W,
                              off_d.data_ptr(), n, bbox_d.data_ptr(), row_d.data_ptr(), n_rows, out.ptr, status.ptr,
                              ws.data_ptr(), nbytes - short, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code, out, status


def hull_of(lab, off, bbox=None):
    """the valid outputs of one call: int64 [10, n]"""
    bbox = ref.measure(np.asarray(lab), off)["bbox"] if bbox is None else bbox
    code, out, status = c_hull(lab, off, bbox)
    assert code == 0 and status.host(np.int32)[0] == 0
    return out.host(np.int64)


@functools.lru_cache(maxsize=None)
def scene(H, W):
    """random rectangles plus speckle, 4 frames -> (int64 labels, label_off, reference boxes, reference outputs); read only"""
    lab = random_cells(H, W, T=4, seed=3)
    off = ref.frame_tables(lab)
    bbox = ref.measure(lab, off)["bbox"]
    want = href.hull(lab, off)
    for a in (lab, off, bbox, want):
        a.setflags(write=False)
    return lab, off, bbox, want


# ---- against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_outputs_equal_the_restatement(shape, label_dtype):
    lab, off, bbox, want = scene(*shape)
    assert want[0].any()
    for T in (1, 4):
        n = int(off[T])
        got = hull_of(lab[:T].astype(label_dtype), off[:T + 1], bbox[:n])
        assert got.shape == (10, n) and np.array_equal(got, want[:, :n]), T


def test_closed_forms():
    H, W = 5, 65
    whole = np.ones((1, H, W), np.uint16)                       # touches all four borders: corner rows 0 and H
    assert hull_of(whole, np.array([0, 1], np.int64))[:, 0].tolist() == [2 * (H + W), 4, 2 * H * W, H * H + W * W, 0, 0, H, W,
                                                                         H, 1]
    single = np.zeros((1, H, W), np.int32)
    places = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for l, (y, x) in enumerate(places, start=1):
        single[0, y, x] = l
    got = hull_of(single, np.array([0, 4], np.int64))
    for l, (y, x) in enumerate(places):
        assert got[:, l].tolist() == [4, 4, 2, 2, y, x, y + 1, x + 1, 1, 1]
    n = 300
    line = np.zeros((1, 320, 320), np.uint16)
    line[0, np.arange(n) + 7, np.arange(n) + 11] = 1
    assert hull_of(line, np.array([0, 1], np.int64))[:, 0].tolist() == [4 * n, 6, 4 * n - 2, 2 * n * n, 7, 11, n + 7, n + 11,
                                                                        2, 2]


def test_chains_and_rows_beyond_one_wave():
    yy, xx = np.mgrid[0:210, 0:210]
    r2 = (yy - 105) ** 2 + (xx - 105) ** 2
    lab = np.zeros((1, 210, 210), np.uint16)
    lab[0][r2 <= 100 ** 2] = 1                                  # an annulus with the hull of the disc of radius 100 ...
    lab[0][r2 <= 40 ** 2] = 2                                   # ... around a disc of radius 40
    off = np.array([0, 2], np.int64)
    bbox = ref.measure(lab, off)["bbox"]
    assert rows_from(bbox).tolist() == [0, 202, 284]            # 201 and 81 pixel rows
    want = np.array([href.andrew(lab[0], 1), href.andrew(lab[0], 2)], np.int64).T
    assert want[1, 0] > 64 and want[1, 1] <= 64                 # more hull vertices than a wave has lanes, and fewer
    got = hull_of(lab, off, bbox)
    assert np.array_equal(got, want)
    disc = (lab[0] > 0).astype(np.int64)
    assert got[1:, 0].tolist() == href.andrew(disc, 1)[1:] and got[0, 0] == href.perimeter(disc > 0) + got[0, 1]


def test_two_blobs_of_one_id_and_a_ring():
    lab = np.zeros((1, 40, 70), np.uint16)
    lab[0, 2:6, 3:9] = 1                                        # one id in two pieces, 20 empty rows between them
    lab[0, 26:31, 50:66] = 1
    lab[0, 8:21, 20:41] = 2                                     # a ring
    lab[0, 11:18, 24:37] = 0
    off = np.array([0, 2], np.int64)
    got = hull_of(lab, off)
    assert np.array_equal(got, href.hull(lab, off))
    assert got[0].tolist() == [2 * (4 + 6) + 2 * (5 + 16), 2 * (13 + 21) + 2 * (7 + 13)]
    assert got[1:, 1].tolist() == [4, 2 * 13 * 21, 13 ** 2 + 21 ** 2, 8, 20, 21, 41, 13, 1]      # the hull does not see the hole
    assert got[1, 0] == 6 and got[3, 0] == 29 ** 2 + 63 ** 2 and got[4:8, 0].tolist() == [2, 3, 31, 66]


def test_ids_outside_the_table_are_not_a_cell():
    lab = np.array(scene(33, 200)[0][:2], np.int32)
    k0 = int(lab[0].max())
    lab[0, 5:12, 40:90] = k0 + 3                                # beyond the table, amid the cells
    lab[0, 20:26, 100:160] = -7
    lab[1, 2:30, 60:64] = -2 ** 31
    lab[1][lab[1] == 2] = 0                                     # an absent id inside the table
    lab[1][lab[1] == 5] = 0
    off = np.array([0, k0, k0 + int(lab[1].max())], np.int64)
    want = href.hull(lab, off)
    assert not want[:, k0 + 1].any() and not want[:, k0 + 4].any() and want[0, :k0].any()
    got = hull_of(lab, off)
    assert np.array_equal(got, want)
    # the same frames under a shorter table: the ids it drops are not a cell any more, also as neighbours
    short = np.array([0, k0 - 2, k0 - 2 + 3], np.int64)
    assert np.array_equal(hull_of(lab, short), href.hull(lab, short))


def test_two_calls_give_identical_bytes():
    lab, off, bbox, want = scene(70, 131)
    a, b = (hull_of(lab.astype(np.uint16), off, bbox) for _ in range(2))
    assert a.tobytes() == b.tobytes() == want.tobytes()


def test_argument_errors_touch_nothing():
    from microbeseg_amd import _lib
    lib = _lib.load()
    lab, off, bbox, _ = scene(5, 65)
    lab = lab.astype(np.uint16)
    for bad in (0, 3):                                          # uint8 labels and an unknown code
        code, out, status = c_hull(lab, off, bbox, dtype_code=bad)
        assert code == EINVAL and out.untouched() and status.untouched()
    code, out, status = c_hull(lab, off, bbox, short=1)
    assert code == EWORKSPACE and out.untouched() and status.untouched()
    assert lib.mseg_cell_hull_workspace_bytes(-1, 10) == 0 and lib.mseg_cell_hull_workspace_bytes(10, -1) == 0
    assert lib.mseg_cell_hull_workspace_bytes(10, 50) >= 50 * 24
    code, out, status = c_hull(lab, np.zeros(5, np.int64), np.zeros((0, 4), np.int32))       # no cells: no launch
    assert code == 0 and out.untouched() and status.host(np.int32)[0] == 0


def test_inconsistent_box_sets_the_status_word():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab, off, bbox, want = scene(33, 200)
    lab = lab.astype(np.uint16)
    n = int(off[-1])
    s = next(i for i in range(n // 2, n) if bbox[i, 2] - bbox[i, 0] >= 2)       # a cell in the middle of the table
    small = np.array(bbox)
    small[s, 2] -= 1                                            # its last pixel row is outside the box now
    code, out, status = c_hull(lab, off, small, rows_from(small))
    assert code == 0 and status.host(np.int32)[0] != 0
    out.host(np.int64)                                          # the guard bands are intact
    with pytest.raises(RuntimeError, match="outside the bounding box"):
        cells.hull_raw(_dev(lab), _lib.PIX_U16, off, small)
    assert np.array_equal(cells.hull_raw(_dev(lab), _lib.PIX_U16, off, np.array(bbox)), want)


# ---- measure_cells(hull=True) ---------------------------------------------------------------------------------------------------
def test_measure_cells_with_hull():
    from microbeseg_amd.inference import cells
    lab64, off, _, ints = scene(70, 131)
    lab = lab64.astype(np.uint16)
    H, W = lab.shape[1:]
    img = np.random.default_rng(5).integers(0, 65536, (4, 1, H, W)).astype(np.uint16)
    df = cells.measure_cells(lab, img, hull=True)
    assert list(df.columns) == cells.columns([0], True, False, True) and len(df) > 100
    want = cells.table_from_sums(off, H, W, ref.measure(lab, off, img), channels=[0], links=ref.links(lab, off), hull=ints)
    pd.testing.assert_frame_equal(df[HULL_COLUMNS], want[HULL_COLUMNS], check_exact=True)
    plain = cells.measure_cells(lab, img)
    assert list(plain.columns) == cells.columns([0], True)
    pd.testing.assert_frame_equal(df[list(plain.columns)], plain, check_exact=True)
    assert cells.measure_cells(lab.astype(np.int32), img, hull=True).to_csv().encode() == df.to_csv().encode()
    bare = cells.measure_cells(lab, link=False, hull=True)      # hull does not need link
    assert list(bare.columns) == cells.columns([], False, False, True) and bare[HULL_COLUMNS].equals(df[HULL_COLUMNS])
    both = cells.measure_cells(lab, drift=2, hull=True)
    assert list(both.columns) == cells.columns([], True, True, True) and both[HULL_COLUMNS].equals(df[HULL_COLUMNS])


def test_infer_worker_passes_hull_on():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab = scene(33, 200)[0].astype(np.uint16)
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    assert worker.hull is False
    assert list(worker.cell_table(lab).columns) == cells.columns([], link=True)
    worker.hull = True
    df = worker.cell_table(lab)
    assert list(df.columns) == cells.columns([], True, False, True) and df.equals(cells.measure_cells(lab, hull=True))
