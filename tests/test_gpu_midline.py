"""GPU (MI355X): the per-cell midline (csrc/midline.hip) through the C ABI and through measure_cells, every
integer and the skeleton image equal to the restatement tests/midline_ref.py (which test_midline_host.py checks on the CPU).
The bounding boxes the kernels are given come from tests/cells_ref.py, never from the code under test."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
import midline_ref as mref
from test_gpu_cells import GUARD, PIX, Guarded, _dev
from test_gpu_hull import scene as hull_scene
from test_hull_host import random_cells
from test_midline_host import MIDLINE_COLUMNS, rectangle, spherocylinder

pytestmark = pytest.mark.gpu
EINVAL, EWORKSPACE = -1, -3
SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (33, 200), (70, 131)]
ONE = np.array([0, 1], np.int64)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class GuardedBytes(Guarded):
    """Guarded for uint8 buffers: the skeleton image and the workspace"""

    def __init__(self, shape):
        self.shape, self.n, self.fill = shape, int(np.prod(shape)), 0x5A
        self.t = torch.full((self.n + 2 * GUARD,), self.fill, dtype=torch.uint8, device="cuda")


def words_from(bbox):
    """word_off of the boxes: (r1 - r0 + 2) rows of ceil((c1 - c0 + 2) / 64) words for a present cell, none for an absent one"""
    b = np.asarray(bbox, np.int64).reshape(-1, 4)
    words = np.where(b[:, 2] > b[:, 0], (b[:, 2] - b[:, 0] + 2) * ((b[:, 3] - b[:, 1] + 2 + 63) // 64), 0)
    return np.concatenate([[0], np.cumsum(words)]).astype(np.int64)


def c_midline(lab, off, bbox, word_off=None, short=0, dtype_code=None, skeleton=True, dims=None):
    """mseg_cell_midline through ctypes -> (return code, guarded out [12, n], guarded skeleton or None, guarded status [1],
    guarded workspace)"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    word_off = words_from(bbox) if word_off is None else np.asarray(word_off, np.int64)
    n_words = int(word_off[-1])
    lab_d, off_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda()
    bbox_d = torch.from_numpy(np.array(bbox, np.int32).reshape(-1, 4)).cuda()
    word_d = torch.from_numpy(np.array(word_off, np.int64)).cuda()
    out, status = Guarded((12, n), torch.int64), Guarded((1,), torch.int32)
    skel = GuardedBytes((T, H, W)) if skeleton else None
    nbytes = lib.mseg_cell_midline_workspace_bytes(n, n_words)
    assert nbytes >= 16 * n_words and nbytes > 0
    ws = GuardedBytes((nbytes,))
    code = lib.mseg_cell_midline(lab_d.data_ptr(), PIX[lab.dtype] if dtype_code is None else dtype_code,
                                 *((T, H, W) if dims is None else dims), off_d.data_ptr(), n, bbox_d.data_ptr(),
                                 word_d.data_ptr(), n_words, out.ptr, skel.ptr if skeleton else None, status.ptr, ws.ptr,
                                 nbytes - short, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code, out, skel, status, ws


def midline_of(lab, off=ONE, bbox=None, skeleton=True):
    """the valid outputs of one call: int64 [12, n] and the uint8 skeleton image (None if not asked for)"""
    bbox = ref.measure(np.asarray(lab), off)["bbox"] if bbox is None else bbox
    code, out, skel, status, ws = c_midline(lab, off, bbox, skeleton=skeleton)
    assert code == 0 and status.host(np.int32)[0] == 0                  # neither a pixel outside a box nor the round cap
    ws.host(np.uint8)                                                   # the guard bands of the workspace are intact
    return out.host(np.int64), (skel.host(np.uint8) if skeleton else None)


def check(lab, off=ONE):
    """outputs of the device == the restatement, for the labels as they are; -> the twelve planes"""
    want, want_skel = mref.midline(lab, off)
    got, skel = midline_of(lab, off)
    assert np.array_equal(got, want) and np.array_equal(skel, want_skel)
    return got


@functools.lru_cache(maxsize=None)
def scene(H, W):
    """random rectangles plus speckle, 4 frames -> (int64 labels, label_off, reference boxes, reference outputs, reference
    skeleton image); read only"""
    lab = random_cells(H, W, T=4, seed=3)
    off = ref.frame_tables(lab)
    bbox = ref.measure(lab, off)["bbox"]
    want, skel = mref.midline(lab, off)
    for a in (lab, off, bbox, want, skel):
        a.setflags(write=False)
    return lab, off, bbox, want, skel


# ---- against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_outputs_equal_the_restatement(shape, label_dtype):
    lab, off, bbox, want, want_skel = scene(*shape)
    assert want[0].any()
    for T in (1, 4):
        n = int(off[T])
        got, skel = midline_of(lab[:T].astype(label_dtype), off[:T + 1], bbox[:n])
        assert got.shape == (12, n) and np.array_equal(got, want[:, :n]), T
        assert skel.shape == (T,) + shape and np.array_equal(skel, want_skel[:T]), T


def test_closed_forms():
    def ints(h, w):
        return check(rectangle(h, w)[None].astype(np.uint16))[:, 0].tolist()
    assert ints(1, 1) == [1, 0, 0, 0, 0, 1, 2, 3, 1, 2, 3, 1]
    assert ints(2, 2)[0] == 1 and ints(2, 2)[5] == 2
    assert ints(3, 3)[0] == 1 and ints(3, 3)[6:] == [3, 4, 4, 3, 4, 4]
    assert ints(4, 4)[0] == 1 and ints(4, 4)[5] == 3
    assert ints(1, 5) == [5, 4, 0, 2, 0, 1, 2, 3, 1, 2, 7, 1]
    assert ints(2, 5)[:5] == [4, 3, 0, 2, 0]
    assert ints(3, 7)[:5] == [5, 4, 0, 2, 0] and (ints(3, 7)[8], ints(3, 7)[11]) == (4, 4)
    assert ints(8, 30)[:6] == [23, 22, 0, 2, 0, 5] and (ints(8, 30)[8], ints(8, 30)[11]) == (16, 16)
    rod = check(spherocylinder(30, 8)[None].astype(np.int32))[:, 0].tolist()
    assert rod[:6] == [23, 22, 0, 2, 0, 5] and {rod[8], rod[11]} == {13, 16}


def test_a_cell_that_fills_the_frame_and_cells_in_its_corners():
    H, W = 5, 65
    whole = np.ones((1, H, W), np.uint16)                       # touches all four borders: the nearest outside is row -1 / H
    assert check(whole)[:, 0].tolist() == [W - 4, W - 5, 0, 2, 0, 3, 2, 2, 9, 2, W - 3, 9]
    single = np.zeros((1, H, W), np.int32)
    places = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for l, (y, x) in enumerate(places, start=1):
        single[0, y, x] = l
    got = check(single, np.array([0, 4], np.int64))
    for l, (y, x) in enumerate(places):
        assert got[:, l].tolist() == [1, 0, 0, 0, 0, 1, y, x, 1, y, x, 1]


def test_word_and_row_boundaries():
    bar = np.zeros((1, 9, 210), np.uint16)
    bar[0, 3:6, 5:205] = 1                                      # 3 x 200: four words per row
    assert check(bar)[:, 0].tolist() == [198, 197, 0, 2, 0, 2, 4, 6, 4, 4, 203, 4]
    assert check(np.ascontiguousarray(bar.transpose(0, 2, 1)))[:, 0].tolist() == [198, 197, 0, 2, 0, 2, 6, 4, 4, 203, 4, 4]
    n = 300
    line = np.zeros((1, 320, 320), np.uint16)                   # 302 rows of 5 words: thinned in the workspace, not in LDS
    line[0, np.arange(n) + 7, np.arange(n) + 11] = 1
    got, skel = midline_of(line)
    assert got[:, 0].tolist() == [n, 0, n - 1, 2, 0, 1, 7, 11, 1, n + 6, n + 10, 1] and np.array_equal(skel, line)


def test_a_disc_of_a_hundred_rounds():
    yy, xx = np.mgrid[0:210, 0:210]
    disc = np.zeros((1, 210, 210), np.uint16)
    disc[0][(yy - 105) ** 2 + (xx - 105) ** 2 <= 100 ** 2] = 1  # 203 rows of 4 words: more rows than a group has lanes
    got = check(disc)
    assert got[5, 0] > 90 and got[0, 0] < 10


def test_neighbours_are_not_the_cell():
    lab = np.zeros((1, 20, 60), np.uint16)
    lab[0, 5:13, 4:20] = 1                                      # two rectangles that share an edge
    lab[0, 5:13, 20:50] = 2
    off = np.array([0, 2], np.int64)
    got, skel = midline_of(lab, off)
    for l in (1, 2):
        alone = np.where(lab == l, 1, 0).astype(np.uint16)
        a, s = midline_of(alone)
        assert np.array_equal(a[:, 0], got[:, l - 1]) and np.array_equal(s == 1, (skel == 1) & (lab == l))
    assert np.array_equal(got, mref.midline(lab, off)[0])


def test_a_ring_and_two_blobs_of_one_id():
    lab = np.zeros((1, 40, 70), np.uint16)
    lab[0, 2:6, 3:9] = 1                                        # one id in two pieces, 20 empty rows between them
    lab[0, 26:31, 50:66] = 1
    lab[0, 8:21, 20:41] = 2                                     # a ring
    lab[0, 11:18, 24:37] = 0
    got = check(lab, np.array([0, 2], np.int64))
    assert got[3, 0] == 4 and got[4, 0] == 0 and got[6:, 0].tolist() == [3, 5, 4, 28, 63, 9]
    assert got[3, 1] == 0 and got[0, 1] > 1 and got[4, 1] == 0 and not got[6:, 1].any()


def test_ids_outside_the_table_are_not_a_cell():
    lab = np.array(scene(33, 200)[0][:2], np.int32)
    k0 = int(lab[0].max())
    lab[0, 5:12, 40:90] = k0 + 3                                # beyond the table, amid the cells
    lab[0, 20:26, 100:160] = -7
    lab[1, 2:30, 60:64] = -2 ** 31
    lab[1][lab[1] == 2] = 0                                     # an absent id inside the table
    lab[1][lab[1] == 5] = 0
    off = np.array([0, k0, k0 + int(lab[1].max())], np.int64)
    got = check(lab, off)
    assert not got[:, k0 + 1].any() and not got[:, k0 + 4].any() and got[0, :k0].any()
    # the same frames under a shorter table: the ids it drops are not a cell any more, also as neighbours
    check(lab, np.array([0, k0 - 2, k0 - 2 + 3], np.int64))


# ---- other paths --------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes_with_and_without_the_skeleton():
    lab, off, bbox, want, want_skel = scene(70, 131)
    lab = lab.astype(np.uint16)
    (a, sa), (b, sb) = (midline_of(lab, off, bbox) for _ in range(2))
    assert a.tobytes() == b.tobytes() == want.tobytes() and sa.tobytes() == sb.tobytes() == want_skel.tobytes()
    bare, none = midline_of(lab, off, bbox, skeleton=False)
    assert none is None and bare.tobytes() == want.tobytes()


# ---- misuse -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing():
    from microbeseg_amd import _lib
    lib = _lib.load()
    lab, off, bbox, _, _ = scene(5, 65)
    lab = lab.astype(np.uint16)
    T, H, W = lab.shape
    refused = [dict(dtype_code=0), dict(dtype_code=3),                              # uint8 labels and an unknown code
               dict(dims=(-1, H, W)), dict(dims=(T, 0, W)), dict(dims=(T, H, -W)),
               dict(dims=(1, 512, 2 ** 22 - 1)), dict(dims=(1, 2 ** 16, 2 ** 15))]  # H * W == 2^31 - 512, and beyond
    for kw in refused:
        code, out, skel, status, ws = c_midline(lab, off, bbox, **kw)
        assert code == EINVAL and out.untouched() and skel.untouched() and status.untouched() and ws.untouched(), kw
    code, out, skel, status, ws = c_midline(lab, off, bbox, short=1)
    assert code == EWORKSPACE and out.untouched() and skel.untouched() and status.untouched() and ws.untouched()
    assert lib.mseg_cell_midline_workspace_bytes(-1, 0) == 0 and lib.mseg_cell_midline_workspace_bytes(10, -1) == 0
    assert lib.mseg_cell_midline_workspace_bytes(10, 50) >= 50 * 16
    code, out, skel, status, ws = c_midline(lab, np.zeros(5, np.int64), np.zeros((0, 4), np.int32))     # no cells: no kernel
    assert code == 0 and out.untouched() and ws.untouched() and status.host(np.int32)[0] == 0 and not skel.host(np.uint8).any()


def test_a_box_that_is_too_small_sets_status_bit_0():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab, off, bbox, want, want_skel = scene(33, 200)
    lab, off = lab.astype(np.uint16), np.array(off)
    n = int(off[-1])
    s = next(i for i in range(n // 2, n) if bbox[i, 2] - bbox[i, 0] >= 2)       # a cell in the middle of the table
    small = np.array(bbox)
    small[s, 2] -= 1                                            # its last pixel row is outside the box now
    code, out, skel, status, ws = c_midline(lab, off, small, words_from(small))
    assert code == 0 and status.host(np.int32)[0] == 1
    got = out.host(np.int64)                                    # the guard bands of all three are intact ...
    skel.host(np.uint8), ws.host(np.uint8)
    others = np.arange(n) != s                                  # ... and every other cell is what it was: its words were not touched
    assert np.array_equal(got[:, others], want[:, others]) and not np.array_equal(got[:, s], want[:, s])
    with pytest.raises(RuntimeError, match="outside the bounding box"):
        cells.midline_raw(_dev(lab), _lib.PIX_U16, off, small)
    ints, image = cells.midline_raw(_dev(lab), _lib.PIX_U16, off, np.array(bbox), skeleton=True)
    assert np.array_equal(ints, want) and image.dtype == np.uint8 and np.array_equal(image, want_skel)
    assert np.array_equal(cells.midline_raw(_dev(lab), _lib.PIX_U16, off, np.array(bbox)), want)


# ---- measure_cells(midline=True) ------------------------------------------------------------------------------------------------
def test_measure_cells_with_midline():
    from microbeseg_amd.inference import cells
    lab64, off, _, ints, _ = scene(70, 131)
    lab = lab64.astype(np.uint16)
    H, W = lab.shape[1:]
    img = np.random.default_rng(5).integers(0, 65536, (4, 1, H, W)).astype(np.uint16)
    df = cells.measure_cells(lab, img, midline=True)
    assert list(df.columns) == cells.columns([0], True, False, False, True) and len(df) > 100
    want = cells.table_from_sums(off, H, W, ref.measure(lab, off, img), channels=[0], links=ref.links(lab, off), midline=ints)
    pd.testing.assert_frame_equal(df[MIDLINE_COLUMNS], want[MIDLINE_COLUMNS], check_exact=True)
    assert df["midline_length"].isna().any() and df["midline_length"].notna().any()
    plain = cells.measure_cells(lab, img)
    assert list(plain.columns) == cells.columns([0], True) and cells.measure_cells(lab, img, midline=False).equals(plain)
    pd.testing.assert_frame_equal(df[list(plain.columns)], plain, check_exact=True)
    assert cells.measure_cells(lab.astype(np.int32), img, midline=True).to_csv().encode() == df.to_csv().encode()
    bare = cells.measure_cells(lab, link=False, midline=True)   # midline needs neither link nor hull
    assert list(bare.columns) == cells.columns([], False, False, False, True) and bare[MIDLINE_COLUMNS].equals(df[MIDLINE_COLUMNS])
    both = cells.measure_cells(lab, hull=True, midline=True)
    assert list(both.columns) == cells.columns([], True, False, True, True) and both[MIDLINE_COLUMNS].equals(df[MIDLINE_COLUMNS])
    hulled = cells.table_from_sums(off, H, W, ref.measure(lab, off), links=ref.links(lab, off), hull=hull_scene(70, 131)[3])
    pd.testing.assert_frame_equal(both[cells.HULL_COLUMNS], hulled[cells.HULL_COLUMNS], check_exact=True)


def test_infer_worker_passes_midline_on():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab = scene(33, 200)[0].astype(np.uint16)
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    assert worker.midline is False
    assert list(worker.cell_table(lab).columns) == cells.columns([], link=True)
    worker.midline = True
    df = worker.cell_table(lab)
    assert list(df.columns) == cells.columns([], True, False, False, True) and df.equals(cells.measure_cells(lab, midline=True))
