"""GPU (MI355X): linking under a tile-wise displacement field (mseg_stack_flow in csrc/drift.hip, mseg_cell_links_field in
csrc/cells.hip) through the C ABI and through measure_cells, every value equal to the numpy restatement
tests/flow_ref.py.  The expectations of the end-to-end test rest on properties of the input that tests/test_flow_host.py
asserts on the CPU."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
import drift_ref as dref
import flow_ref as fref
from test_flow_host import FIX_FLOW, FIX_R, FIX_SHAPE, FIX_T, FIX_TILE, fixture_stack
from test_gpu_cells import PIX, Guarded, _dev, c_links, random_small_labels
from test_gpu_drift import c_drift, c_links_shifted, random_labels

pytestmark = pytest.mark.gpu
EINVAL, EWORKSPACE = -1, -3
# (H, W, tile): W no multiple of 64, H no multiple of the tile; 2 x 3 and 3 x 4 tiles of 64 px, 3 x 3 of 128, 2 x 3 of 256
CASES = [(70, 131, 64), (130, 200, 64), (260, 300, 128), (300, 520, 256)]
BASES = [(0, 0), (-5, 7), (3, -70), (-129, 64), (0, 4000)]          # the last moves everything out of the frame
T_MAX = 3


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_flow(lab, off, base, r, tile, short=0, dtype_code=None, null=()):
    """mseg_stack_flow through ctypes -> (return code, the guarded score buffer)"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    side = 2 * min(max(r, 0), 32) + 1
    ty, tx = fref.tiles(H, W, tile if tile in (64, 128, 256) else 64)
    lab_d, off_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda()      # copies: the sources are read-only
    base_d = torch.from_numpy(np.array(base, np.int32)).cuda()
    scores = Guarded((T - 1, ty, tx, side, side), torch.int32)
    nbytes = lib.mseg_stack_flow_workspace_bytes(T, H, W)
    assert nbytes > 0 and nbytes == lib.mseg_stack_drift_workspace_bytes(T, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ptr = {"labels": lab_d.data_ptr(), "label_off": off_d.data_ptr(), "base": base_d.data_ptr(), "scores": scores.ptr,
           "ws": ws.data_ptr()}
    for name in null:
        ptr[name] = None
    code = lib.mseg_stack_flow(ptr["labels"], PIX[lab.dtype] if dtype_code is None else dtype_code, T, H, W, ptr["label_off"],
                               tile, r, ptr["base"], ptr["scores"], ptr["ws"], nbytes - short, _stream())
    torch.cuda.synchronize()
    return code, scores


def c_links_field(lab, off, cap, field, tile, expect=0):
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    lab_d, off_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda()
    field_d = torch.from_numpy(np.ascontiguousarray(field, np.int32)).cuda()
    pred, ovl, status = Guarded((n,), torch.int32), Guarded((n,), torch.int32), Guarded((T,), torch.int32)
    nbytes = lib.mseg_cell_links_workspace_bytes(T, n, cap)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    code = lib.mseg_cell_links_field(lab_d.data_ptr(), PIX[lab.dtype], T, H, W, off_d.data_ptr(), n, cap, tile,
                                     field_d.data_ptr(), pred.ptr, ovl.ptr, status.ptr, ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert code == expect, code
    if expect:
        assert pred.untouched() and ovl.untouched() and status.untouched()
        return None
    return pred.host(np.int32), ovl.host(np.int32), status.host(np.int32)


def bases(base):
    """[T_MAX, 2]: row 0 is not read, the pairs get ``base`` and its mirror image"""
    return np.array([(77, -77), base, (-base[0], -base[1])], np.int32)


@functools.lru_cache(maxsize=None)
def want_scores(H, W, tile, r, base):
    lab, off = random_labels(H, W)
    out = fref.scores(lab[:T_MAX], off[:T_MAX + 1], bases(base), r, tile)
    out.setflags(write=False)
    return out


# ---- mseg_stack_flow ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("case", CASES)
def test_scores_equal_the_restatement(case, label_dtype):
    H, W, tile = case
    lab, off = random_labels(H, W)
    for base in BASES:
        for r in (0, 3, 8):
            want = want_scores(H, W, tile, r, base)
            for T in (1, 2, 3) if base == BASES[1] else (3,):
                code, scores = c_flow(lab[:T].astype(label_dtype), off[:T + 1], bases(base)[:T], r, tile)
                assert code == 0, (base, r, T, code)
                if T == 1:
                    assert scores.untouched()
                    continue
                got = scores.host(np.uint32)
                assert got.shape == want[:T - 1].shape and np.array_equal(got, want[:T - 1]), (base, r, T)
        assert want_scores(H, W, tile, 8, base).any() == (base != BASES[-1]) or base == BASES[3]     # -129 rows: H decides


def test_scores_largest_radius_on_the_smallest_frame():
    H, W, tile = CASES[0]
    lab, off = random_labels(H, W)
    code, scores = c_flow(lab[:2].astype(np.uint16), off[:3], bases((-5, 7))[:2], 32, tile)
    assert code == 0
    want = fref.scores(lab[:2], off[:3], bases((-5, 7))[:2], 32, tile)
    assert want.shape == (1, 2, 3, 65, 65) and np.array_equal(scores.host(np.uint32), want)


def test_scores_ids_beyond_the_table_and_negative_ids_are_background():
    H, W, tile = CASES[1]
    base_lab, off = random_labels(H, W)
    lab = np.array(base_lab[:T_MAX], np.int32)
    lab[1, 10:15, 30:120] = -5
    lab[2, 70:90, 100:190] = -2 ** 31
    low = np.array(off[:T_MAX + 1], np.int64)
    low[1:] -= np.arange(1, T_MAX + 1) * 40                   # every table ends 40 ids early
    code, scores = c_flow(lab, low, bases((-5, 7)), 3, tile)
    want = fref.scores(lab, low, bases((-5, 7)), 3, tile)
    assert code == 0 and np.array_equal(scores.host(np.uint32), want)
    assert want.sum() < want_scores(H, W, tile, 3, (-5, 7)).sum()
    code, scores = c_flow(lab, np.zeros(T_MAX + 1, np.int64), bases((-5, 7)), 3, tile)
    assert code == 0 and not scores.host(np.uint32).any()


def test_one_tile_at_base_zero_is_the_drift_surface_and_tiles_sum_to_it():
    H, W = CASES[0][:2]
    lab, off = random_labels(H, W)
    lab, off = lab[:T_MAX].astype(np.uint16), off[:T_MAX + 1]
    for r in (0, 8):
        code, scores = c_flow(lab, off, np.zeros((T_MAX, 2), np.int32), r, 256)          # 70 x 131 is one 256 px tile
        code_d, whole = c_drift(lab, off, r)
        assert code == 0 and code_d == 0
        assert scores.host(np.uint32).tobytes() == whole.host(np.uint32).tobytes()
    H, W, tile = CASES[1]
    lab, off = random_labels(H, W)
    lab, off = lab[:T_MAX].astype(np.uint16), off[:T_MAX + 1]
    r, R = 3, 12
    base = bases((-5, 7))
    got = c_flow(lab, off, base, r, tile)[1].host(np.uint32)
    whole = c_drift(lab, off, R)[1].host(np.uint32)
    for t in range(1, T_MAX):
        by, bx = (int(v) for v in base[t])
        assert np.array_equal(got[t - 1].sum(axis=(0, 1), dtype=np.int64),
                              whole[t - 1, by - r + R:by + r + R + 1, bx - r + R:bx + r + R + 1])


def test_scores_two_calls_give_identical_bytes():
    lab, off, shift, want, _ = fixture_stack()
    a, b = (c_flow(lab, off, shift, FIX_FLOW, FIX_TILE)[1].host(np.uint32) for _ in range(2))
    assert a.tobytes() == b.tobytes() == want.tobytes()


def test_scores_argument_errors_touch_nothing():
    from microbeseg_amd import _lib
    lib = _lib.load()
    H, W, tile = CASES[0]
    lab, off = random_labels(H, W)
    lab, off, base = lab[:2].astype(np.uint16), off[:3], bases((0, 0))[:2]
    for kw in ({"tile": 32}, {"tile": 100}, {"tile": 0}, {"r": -1}, {"r": 33}, {"dtype_code": 0}, {"dtype_code": 3},
               {"null": ("labels",)}, {"null": ("label_off",)}, {"null": ("base",)}, {"null": ("scores",)}, {"null": ("ws",)}):
        code, scores = c_flow(lab, off, base, kw.get("r", 3), kw.get("tile", tile), dtype_code=kw.get("dtype_code"),
                              null=kw.get("null", ()))
        assert code == EINVAL and scores.untouched(), kw
    code, scores = c_flow(lab, off, base, 3, tile, short=1)
    assert code == EWORKSPACE and scores.untouched()
    assert lib.mseg_stack_flow_workspace_bytes(0, 5, 65) == 0 and lib.mseg_stack_flow_workspace_bytes(2, 0, 65) == 0
    assert lib.mseg_stack_flow_workspace_bytes(2, 46341, 46341) == 0           # H * W >= 2^31 - 512


# ---- mseg_cell_links_field --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("case", CASES[:2])
def test_links_field_equal_the_restatement(case, label_dtype):
    H, W, _ = case
    base_lab, off = random_labels(H, W)
    lab = base_lab.astype(label_dtype)
    T, cap = lab.shape[0], 16384
    plain = c_links(lab, off, cap)
    rng = np.random.default_rng(H)
    for tile in (64, 128, 256):
        ty, tx = fref.tiles(H, W, tile)
        # a zero field: mseg_cell_links; a constant field: mseg_cell_links_shifted, byte for byte
        got = c_links_field(lab, off, cap, np.zeros((T, ty, tx, 2), np.int32), tile)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, plain)) and got[0].any()
        shift = np.array([(9, 9), (-7, 64), (3, -65), (1, 2)], np.int32)
        got = c_links_field(lab, off, cap, np.broadcast_to(shift[:, None, None, :], (T, ty, tx, 2)), tile)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, c_links_shifted(lab, off, cap, shift)))
        # random fields: small entries (most pixels keep a source) and entries up to +-140 (many leave the frame)
        for reach in (6, 140):
            field = rng.integers(-reach, reach + 1, (T, ty, tx, 2)).astype(np.int32)
            pred, ovl, status = c_links_field(lab, off, cap, field, tile)
            want_pred, want_ovl = fref.links_field(base_lab, off, field, tile)
            assert not status.any() and (want_pred.any() or reach > 6), (tile, reach)     # far entries may empty a frame
            assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl), (tile, reach)
    far = np.full((T,) + fref.tiles(H, W, 64) + (2,), 2 ** 31 - 1, np.int32)
    far[..., 1] = -2 ** 31
    pred, ovl, status = c_links_field(lab, off, cap, far, 64)
    assert not pred.any() and not ovl.any() and not status.any()
    for bad in (32, 100, 0):
        c_links_field(lab, off, cap, far, bad, expect=EINVAL)


def test_links_field_table_overflow_and_the_wrappers_redo():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab = random_small_labels()                                # 3 x 96 x 128, about 2000 cells per frame
    off = ref.frame_tables(lab)
    field = np.random.default_rng(8).integers(-4, 5, (3, 2, 2, 2)).astype(np.int32)
    want_pred, want_ovl = fref.links_field(lab, off, field, 64)
    pred, ovl, status = c_links_field(lab, off, 16384, field, 64)           # more entries than pixels: cannot fill up
    assert not status.any() and np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
    _, _, status = c_links_field(lab, off, 64, field, 64)                   # the smallest table fills up and says so
    assert status[0] == 0 and status[1] != 0 and status[2] != 0
    lab_d = _dev(lab)
    pred, ovl = cells.link_raw(lab_d, _lib.PIX_U16, off, table_cap=64, field=field, tile=64)
    assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
    with pytest.raises(ValueError, match="field"):
        cells.link_raw(lab_d, _lib.PIX_U16, off, field=field, tile=128)
    with pytest.raises(ValueError, match="field"):
        cells.link_raw(lab_d, _lib.PIX_U16, off, field=field)


# ---- measure_cells(flow=...) --------------------------------------------------------------------------------------------------------
def test_measure_cells_with_flow_reproduces_the_restatement_on_the_expanding_colony():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab, off, shift, sc, field = (np.array(a) for a in fixture_stack())
    got = cells.flow_raw(_dev(lab), _lib.PIX_U16, off, shift, FIX_FLOW, FIX_TILE)
    assert got.dtype == np.uint32 and np.array_equal(got, sc)
    assert np.array_equal(cells.pick_flow(got, shift), field)
    assert cells.flow_raw(_dev(lab[:1]), _lib.PIX_U16, off[:2], shift[:1], 3, 64).shape == (0, 3, 4, 7, 7)
    img = np.random.default_rng(5).integers(0, 65536, (FIX_T, 1) + FIX_SHAPE).astype(np.uint16)
    before = cells.measure_cells(lab, img, drift=FIX_R)
    df = cells.measure_cells(lab, img, drift=FIX_R, flow=FIX_FLOW, flow_tile=FIX_TILE)
    assert list(df.columns) == cells.columns([0], link=True, drift=True, flow=True)
    want_pred, want_ovl = fref.links_field(lab, off, field, FIX_TILE)
    present = np.asarray(ref.measure(lab, off)["shape"][0]) > 0
    assert np.array_equal(df["pred_label"].to_numpy(), want_pred[present])
    assert np.array_equal(df["overlap"].to_numpy(), want_ovl[present])
    want = cells.table_from_sums(off, *FIX_SHAPE, ref.measure(lab, off, img), channels=[0], links=(want_pred, want_ovl),
                                 shift=shift, field=field, tile=FIX_TILE)
    pd.testing.assert_frame_equal(df, want, check_exact=True)
    t = df["frame"].to_numpy()
    j = np.floor(df["centroid_y"].to_numpy()).astype(int) // FIX_TILE
    i = np.floor(df["centroid_x"].to_numpy()).astype(int) // FIX_TILE
    assert np.array_equal(df[["flow_y", "flow_x"]].to_numpy(), np.where((t > 0)[:, None], field[t, j, i], 0))
    # every column that is neither a link nor a flow column is the one of the table without flow; with flow = None the
    # table is today's
    same = [c for c in before.columns if c not in ("pred_label", "overlap", "track_id", "parent_track")]
    pd.testing.assert_frame_equal(df[same], before[same], check_exact=True)
    assert df["track_id"].nunique() < before["track_id"].nunique()
    none = cells.measure_cells(lab, img, drift=FIX_R, flow=None, flow_tile=128)
    assert none.to_csv().encode() == before.to_csv().encode()
    pd.testing.assert_frame_equal(before, cells.table_from_sums(off, *FIX_SHAPE, ref.measure(lab, off, img), channels=[0],
                                                                links=dref.links_shifted(lab, off, shift), shift=shift),
                                  check_exact=True)
    # the worker passes both settings on
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    worker.drift, worker.flow, worker.flow_tile = FIX_R, FIX_FLOW, FIX_TILE
    assert worker.cell_table(lab).equals(cells.measure_cells(lab, drift=FIX_R, flow=FIX_FLOW, flow_tile=FIX_TILE))
