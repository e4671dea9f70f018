"""GPU (MI355X): drift-compensated linking (csrc/drift.hip, mseg_cell_links_shifted in csrc/cells.hip) through
the C ABI and through measure_cells, every value equal to the numpy restatement tests/drift_ref.py.  The expectations of the
end-to-end tests rest on properties of the input that tests/test_drift_host.py asserts on the CPU."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
import drift_ref as dref
from test_drift_host import FIX_OFFSETS, FIX_R, FIX_SHAPE, FIX_T, assert_one_track_per_stretch, fixture_stack
from test_gpu_cells import PIX, Guarded, _dev, c_links, random_small_labels

pytestmark = pytest.mark.gpu
EINVAL, EWORKSPACE = -1, -3
SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (70, 131), (33, 200)]
WIDE_R = {(5, 63): 70, (70, 131): 70}       # a search radius beyond W (and H): whole score rows are zero


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_drift(lab, off, R, short=0, dtype_code=None):
    """mseg_stack_drift through ctypes -> (return code, the guarded score buffer)"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    side = 2 * max(R, 0) + 1
    lab_d, off_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda()      # copies: the sources are read-only
    scores = Guarded((T - 1, side, side), torch.int32)
    nbytes = lib.mseg_stack_drift_workspace_bytes(T, H, W)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    code = lib.mseg_stack_drift(lab_d.data_ptr(), PIX[lab.dtype] if dtype_code is None else dtype_code, T, H, W,
                                off_d.data_ptr(), R, scores.ptr, ws.data_ptr(), nbytes - short, _stream())
    torch.cuda.synchronize()
    return code, scores


def c_links_shifted(lab, off, cap, shift):
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    lab_d, off_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda()      # copies: the sources are read-only
    shift_d = torch.from_numpy(np.ascontiguousarray(shift, np.int32)).cuda()
    pred, ovl, status = Guarded((n,), torch.int32), Guarded((n,), torch.int32), Guarded((T,), torch.int32)
    nbytes = lib.mseg_cell_links_workspace_bytes(T, n, cap)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    code = lib.mseg_cell_links_shifted(lab_d.data_ptr(), PIX[lab.dtype], T, H, W, off_d.data_ptr(), n, cap,
                                       shift_d.data_ptr(), pred.ptr, ovl.ptr, status.ptr, ws.data_ptr(), ws.numel(),
                                       _stream())
    torch.cuda.synchronize()
    assert code == 0, code
    return pred.host(np.int32), ovl.host(np.int32), status.host(np.int32)


@functools.lru_cache(maxsize=None)
def random_labels(H, W, T=4, seed=0):
    """small random rectangles, about a third of every frame covered, other rectangles in every frame -> (int64 labels
    [T, H, W], label_off); read only"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    lab = np.zeros((T, H, W), np.int64)
    for t in range(T):
        for k in range(1, max(1, H * W // 40) + 1):
            y, x = rng.integers(0, H), rng.integers(0, W)
            lab[t, y:y + rng.integers(1, 7), x:x + rng.integers(1, 10)] = k
    off = ref.frame_tables(lab)
    lab.setflags(write=False)
    off.setflags(write=False)
    return lab, off


@functools.lru_cache(maxsize=None)
def want_scores(H, W, T, R):
    lab, off = random_labels(H, W)
    return dref.scores(lab[:T], off[:T + 1], R)


# ---- mseg_stack_drift ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_scores_equal_the_restatement(shape, label_dtype):
    H, W = shape
    lab, off = random_labels(H, W)
    assert dref.foreground(lab, off).any()
    for T in (1, 2, 4):
        for R in [0, 1, 12] + ([WIDE_R[shape]] if shape in WIDE_R else []):
            code, scores = c_drift(lab[:T].astype(label_dtype), off[:T + 1], R)
            assert code == 0, (T, R, code)
            if T == 1:
                assert scores.untouched()
                continue
            got, want = scores.host(np.uint32), want_scores(H, W, T, R)
            assert got.shape == want.shape and np.array_equal(got, want), (T, R)
            if R > 12:                               # the shift leaves the frame: nothing can overlap
                beyond_y, beyond_x = np.abs(np.arange(-R, R + 1)) >= H, np.abs(np.arange(-R, R + 1)) >= W
                assert beyond_y.any() and not got[:, beyond_y].any() and not got[:, :, beyond_x].any()
                assert got.any()


def test_scores_of_empty_full_and_out_of_table_frames():
    H, W, R = 33, 200, 12
    base, _ = random_labels(H, W)
    lab = np.array(base, np.int32)
    lab[1] = 0                                       # no foreground
    lab[2] = 1                                       # all foreground
    k3 = int(lab[3].max())
    lab[3, 4:9, 50:130] = k3 + 5                     # beyond the frame's table
    lab[3, 20:25, 10:70] = -3                        # negative
    lab[3, 28:, 150:] = -2 ** 31
    off = np.concatenate([[0], np.cumsum([int(lab[0].max()), 0, 1, k3])]).astype(np.int64)
    code, scores = c_drift(lab, off, R)
    assert code == 0
    got, want = scores.host(np.uint32), dref.scores(lab, off, R)
    assert np.array_equal(got, want)
    assert not got[0].any() and not got[1].any() and got[2].any()
    fg3 = (lab[3] > 0) & (lab[3] <= k3)
    assert got[2, R, R] == fg3.sum() and fg3.sum() < (lab[3] != 0).sum()
    # the same frames with a table that holds nothing: no foreground anywhere
    code, scores = c_drift(lab, np.zeros(5, np.int64), R)
    assert code == 0 and not scores.host(np.uint32).any()


def test_scores_largest_radius_closed_form():
    H, W, R = 5, 65, 128
    lab = np.ones((2, H, W), np.uint16)              # two frames of foreground: the score is the overlap of two rectangles
    code, scores = c_drift(lab, np.array([0, 1, 2], np.int64), R)
    assert code == 0
    d = np.abs(np.arange(-R, R + 1))
    want = np.outer(np.maximum(H - d, 0), np.maximum(W - d, 0)).astype(np.uint32)
    assert np.array_equal(scores.host(np.uint32)[0], want)
    rl, roff = random_labels(H, W)
    code, scores = c_drift(rl[:2].astype(np.uint16), roff[:3], R)
    assert code == 0 and np.array_equal(scores.host(np.uint32), dref.scores(rl[:2], roff[:3], R))


def test_scores_argument_errors_touch_nothing():
    from microbeseg_amd import _lib
    lib = _lib.load()
    lab, off = random_labels(5, 65)
    lab = lab[:2].astype(np.uint16)
    for kw in ({"R": -1}, {"R": 129}, {"R": 4, "dtype_code": 0}, {"R": 4, "dtype_code": 3}):
        code, scores = c_drift(lab, off[:3], kw["R"], dtype_code=kw.get("dtype_code"))
        assert code == EINVAL and scores.untouched(), kw
    code, scores = c_drift(lab, off[:3], 4, short=1)
    assert code == EWORKSPACE and scores.untouched()
    assert lib.mseg_stack_drift_workspace_bytes(0, 5, 65) == 0 and lib.mseg_stack_drift_workspace_bytes(2, 0, 65) == 0
    assert lib.mseg_stack_drift_workspace_bytes(2, 5, -1) == 0
    assert lib.mseg_stack_drift_workspace_bytes(2, 46341, 46341) == 0          # H * W >= 2^31 - 512
    assert lib.mseg_stack_drift_workspace_bytes(2, 5, 65) >= 2 * 5 * 2 * 8


def writable_fixture():
    """copies of the shared fixture for calls that hand arrays to torch (which wants writable memory)"""
    lab, off, sc, shift = fixture_stack()
    return lab.copy(), off.copy(), sc, shift


def test_scores_two_calls_give_identical_bytes():
    lab, off, want, _ = writable_fixture()
    a, b = (c_drift(lab, off, FIX_R)[1].host(np.uint32) for _ in range(2))
    assert a.tobytes() == b.tobytes() == want.tobytes()


# ---- mseg_cell_links_shifted -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_links_shifted_equal_the_restatement(shape, label_dtype):
    H, W = shape
    base, off = random_labels(H, W)
    lab = base.astype(label_dtype)
    cap = 4096
    plain = c_links(lab, off, cap)
    assert not plain[2].any()
    for dy, dx in [(0, 0), (1, 0), (0, -1), (-7, 64), (3, -65), (H, 0), (0, W), (-H, 0), (0, -W), (2 ** 31 - 1, -2 ** 31)]:
        shift = np.array([(dy, dx)] * 4, np.int32)
        pred, ovl, status = c_links_shifted(lab, off, cap, shift)
        want_pred, want_ovl = dref.links_shifted(base, off, shift)
        assert not status.any(), (dy, dx)
        assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl), (dy, dx)
        if (dy, dx) == (0, 0):                       # the unshifted entry point, byte for byte
            assert all(a.tobytes() == b.tobytes() for a, b in zip((pred, ovl, status), plain))
            assert pred.any() or H * W == 1
        if abs(dy) >= H or abs(dx) >= W:
            assert not pred.any() and not ovl.any()
    # another shift for every pair; entry 0 is not read for a pairing
    shift = np.array([(17, -23), (1, 2), (-2, 0), (0, -3)], np.int32)
    pred, ovl, status = c_links_shifted(lab, off, cap, shift)
    want_pred, want_ovl = dref.links_shifted(base, off, shift)
    assert not status.any() and np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)


def test_links_shifted_ignore_ids_outside_the_tables():
    H, W = 33, 200
    base, off = random_labels(H, W)
    lab = np.array(base, np.int32)
    lab[0, 3:8, 20:90] = int(lab[0].max()) + 7
    lab[1, 10:15, 30:120] = -5
    lab[2, 20:30, 100:190] = int(lab[2].max()) + 1
    shift = np.array([(0, 0), (2, -3), (-4, 5), (1, 1)], np.int32)
    pred, ovl, status = c_links_shifted(lab, off, 4096, shift)
    want_pred, want_ovl = dref.links_shifted(np.where(lab < 0, 0, lab), off, shift)
    assert not status.any() and np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)


def test_links_shifted_table_overflow_and_the_wrappers_redo():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab = random_small_labels()
    off = ref.frame_tables(lab)
    zero = np.zeros((3, 2), np.int32)
    shift = np.array([(0, 0), (1, -2), (-3, 4)], np.int32)
    want_pred, want_ovl = dref.links_shifted(lab, off, shift)
    pred, ovl, status = c_links_shifted(lab, off, 16384, shift)          # more entries than pixels: cannot fill up
    assert not status.any() and np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
    # the smallest table fills up, and says so exactly as the unshifted entry point does
    _, _, status_plain = c_links(lab, off, 64)
    for s in (zero, shift):
        _, _, status = c_links_shifted(lab, off, 64, s)
        assert status[0] == 0 and status[1] != 0 and status[2] != 0
        if s is zero:
            assert status.tobytes() == status_plain.tobytes()
    lab_d = _dev(lab)
    pred, ovl = cells.link_raw(lab_d, _lib.PIX_U16, off, table_cap=64, shift=shift)
    assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
    pred, ovl = cells.link_raw(lab_d, _lib.PIX_U16, off, table_cap=64, shift=zero)
    assert all(np.array_equal(a, b) for a, b in zip((pred, ovl), ref.links(lab, off)))
    with pytest.raises(ValueError, match="shift"):
        cells.link_raw(lab_d, _lib.PIX_U16, off, shift=np.zeros((2, 2), np.int32))


def check_plain_table(df, want, raw, off):
    """test_gpu_cells.check_table for a stack of SMALL cells.  Many 2 - 4 px blobs have var_y == var_x exactly; there the
    orientation is +-pi/4 by the sign of the covariance, decided by an exact-equality test that the package makes on the
    integer sums and the restatement on rounded fp64 means, so the two can land on either side.  Those cells (named by
    the exact integers of the restatement, not by the code under test) are taken out of the orientation comparison, the
    only change against check_table; they stay in every other comparison."""
    from microbeseg_amd.inference import cells
    assert list(df.columns) == cells.columns([0], True) == [c for c in want.columns if c != "_skip"] and len(df) == len(want)
    n, sy, sx, syy, sxx, _ = ([int(v) for v in plane] for plane in raw["shape"])
    present = [i for i in range(int(off[-1])) if n[i] > 0]
    round_cell = np.array([n[i] * syy[i] - sy[i] ** 2 == n[i] * sxx[i] - sx[i] ** 2 for i in present])
    assert len(round_cell) == len(df) and round_cell.mean() < 0.10
    close = ["major_axis_length", "minor_axis_length", "std_ch0"]
    for col in df.columns:
        a, b = df[col].to_numpy(), want[col].to_numpy()
        if col == "orientation":
            keep = ~round_cell & ~want["_skip"].to_numpy(bool)
            np.testing.assert_allclose(a[keep], b[keep], rtol=1e-9, atol=1e-6)
        elif col in close:
            np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)
        else:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), col


# ---- measure_cells(drift=...) ---------------------------------------------------------------------------------------------------
def test_drift_raw_and_pick_on_the_fixture():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab, off, want, shift = writable_fixture()
    got = cells.drift_raw(_dev(lab), _lib.PIX_U16, off, FIX_R)
    assert got.dtype == np.uint32 and got.shape == (FIX_T - 1, 2 * FIX_R + 1, 2 * FIX_R + 1) and np.array_equal(got, want)
    assert cells.pick_drift(got).tolist() == shift.tolist() == [[0, 0]] + [list(o) for o in FIX_OFFSETS]
    assert cells.drift_raw(_dev(lab[:1]), _lib.PIX_U16, off[:2], 3).shape == (0, 7, 7)


def test_measure_cells_with_drift_recovers_the_offsets_and_keeps_the_tracks():
    from microbeseg_amd.inference import cells
    lab, off, _, shift = writable_fixture()
    img = np.random.default_rng(5).integers(0, 65536, (FIX_T, 1) + FIX_SHAPE).astype(np.uint16)
    df = cells.measure_cells(lab, img, drift=FIX_R)
    assert list(df.columns) == cells.columns([0], link=True, drift=True)
    total = np.cumsum(np.array([(0, 0)] + FIX_OFFSETS), axis=0)
    assert np.array_equal(df[["drift_y", "drift_x"]].to_numpy(), total[df["frame"].to_numpy()])
    want = cells.table_from_sums(off, *FIX_SHAPE, ref.measure(lab, off, img), channels=[0],
                                 links=dref.links_shifted(lab, off, shift), shift=shift)
    pd.testing.assert_frame_equal(df, want, check_exact=True)
    stretches = assert_one_track_per_stretch(df)
    # the flag is what does it: without it the same stack is the table of before (the restatement's), with broken tracks
    plain = cells.measure_cells(lab, img)
    check_plain_table(plain, ref.table(lab, img, channels=[0], link=True), ref.measure(lab, off, img), off)
    assert plain["track_id"].nunique() > 2 * stretches
    again = cells.measure_cells(lab.astype(np.int32), img, drift=FIX_R)
    assert again.to_csv().encode() == df.to_csv().encode()
    # a search radius that does not reach the jumps cannot find them
    assert not np.array_equal(cells.measure_cells(lab, drift=4)[["drift_y", "drift_x"]].to_numpy(),
                              total[df["frame"].to_numpy()])
    # drift = 0 searches nothing: the links of before, and the drift columns hold zeros
    zero = cells.measure_cells(lab, img, drift=0)
    assert not zero[["drift_y", "drift_x"]].to_numpy().any()
    pd.testing.assert_frame_equal(zero[list(plain.columns)], plain, check_exact=True)
    assert np.array_equal(zero["centroid_y_reg"].to_numpy(), zero["centroid_y"].to_numpy())


def test_infer_worker_passes_drift_on():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab, _, _, _ = writable_fixture()
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    assert worker.drift is None
    plain = worker.cell_table(lab)
    assert list(plain.columns) == cells.columns([], link=True)
    worker.drift = FIX_R
    df = worker.cell_table(lab)
    assert df.equals(cells.measure_cells(lab, drift=FIX_R)) and "drift_y" in df.columns
    assert df["track_id"].nunique() < plain["track_id"].nunique()
