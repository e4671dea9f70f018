"""GPU (MI355X): gap closing in cell tracks (mseg_cell_links_gap in csrc/cells.hip) through the C ABI and
through measure_cells, every value equal to the numpy restatement tests/gap_ref.py.  The expectations of the end-to-end tests
rest on properties of the inputs that tests/test_gap_host.py asserts on the CPU."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cells_ref as ref
import drift_ref as dref
import flow_ref as fref
import gap_ref as gref
from test_gap_host import BASE_SHAPE, base_stack, check_division_table, division_stack, moved_stack
from test_gpu_cells import PIX, Guarded, _dev, c_links, check_table, random_small_labels
from test_gpu_drift import c_links_shifted, random_labels
from test_gpu_flow import c_links_field

pytestmark = pytest.mark.gpu
EINVAL = -1
T_RAW = 6
SHAPES = [(61, 83), (96, 150)]           # W no multiple of 8: the row tail; 2 x 3 tiles of 64 px with partial tiles


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def c_links_gap(lab, off, cap, g, want, open_, shift=None, tile=0, expect=0):
    """mseg_cell_links_gap through ctypes -> (pred, overlap, status) from guarded buffers"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    lab_d, off_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda()      # copies: the sources are read-only
    want_d = torch.from_numpy(np.asarray(want, bool).astype(np.uint8)).cuda()
    open_d = torch.from_numpy(np.asarray(open_, bool).astype(np.uint8)).cuda()
    assert want_d.numel() == n and open_d.numel() == n
    shift_d = torch.from_numpy(np.ascontiguousarray(shift, np.int32)).cuda() if shift is not None else None
    pred, ovl, status = Guarded((n,), torch.int32), Guarded((n,), torch.int32), Guarded((T,), torch.int32)
    nbytes = lib.mseg_cell_links_workspace_bytes(T, n, cap)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    code = lib.mseg_cell_links_gap(lab_d.data_ptr(), PIX[lab.dtype], T, H, W, off_d.data_ptr(), n, cap, g, tile,
                                   shift_d.data_ptr() if shift_d is not None else None, want_d.data_ptr(), open_d.data_ptr(),
                                   pred.ptr, ovl.ptr, status.ptr, ws.data_ptr(), ws.numel(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert code == expect, code
    if expect:
        assert pred.untouched() and ovl.untouched() and status.untouched()
        return None
    return pred.host(np.int32), ovl.host(np.int32), status.host(np.int32)


@functools.lru_cache(maxsize=None)
def raw_case(H, W):
    """-> (labels int64 [6, H, W], label_off, want, open): about 30 % of the flags set; read only"""
    lab, off = random_labels(H, W, T_RAW)
    rng = np.random.default_rng(H * W)
    want, open_ = rng.random(int(off[-1])) < 0.3, rng.random(int(off[-1])) < 0.3
    want.setflags(write=False)
    open_.setflags(write=False)
    return lab, off, want, open_


def motions(H, W):
    """(shift, field, tile) triples: none; shifts within +-20, one row moving the whole frame outside; fields"""
    rng = np.random.default_rng(H + W)
    out = [(None, None, 0)]
    shift = rng.integers(-20, 21, (T_RAW, 2)).astype(np.int32)
    out.append((shift, None, 0))
    far = shift[::-1].copy()
    far[4] = (3, -W)                                                # no pixel of frame 4 has a source
    far[5] = (H, 0)
    out.append((far, None, 0))
    for tile, reach in ((64, 6), (64, 20), (128, 9)):
        ty, tx = fref.tiles(H, W, tile)
        out.append((None, rng.integers(-reach, reach + 1, (T_RAW, ty, tx, 2)).astype(np.int32), tile))
    return out


# ---- mseg_cell_links_gap against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_links_gap_equal_the_restatement(shape, label_dtype):
    H, W = shape
    base_lab, off, want, open_ = raw_case(H, W)
    lab = base_lab.astype(label_dtype)
    cap = 1 << (H * W).bit_length()                              # more entries than pixels: cannot fill up
    for g in (2, 3):
        for shift, field, tile in motions(H, W):
            moved = field if field is not None else shift
            pred, ovl, status = c_links_gap(lab, off, cap, g, want, open_, moved, tile)
            want_pred, want_ovl = gref.links_gap(base_lab, off, g, want, open_, shift, field, tile or None)
            assert not status.any()
            assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl), (g, tile, shift is None)
            assert not pred[~want].any() and not pred[:int(off[g])].any()
            if shift is None and field is None:
                assert want_pred.any()
            if shift is not None and shift[4][1] == -W:
                assert not pred[int(off[4]):].any() and pred[:int(off[4])].any()


@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", SHAPES)
def test_gap_one_with_all_flags_is_the_ordinary_call_bit_for_bit(shape, label_dtype):
    H, W = shape
    base_lab, off, _, _ = raw_case(H, W)
    lab, off = base_lab.astype(label_dtype), np.array(off)       # copies: the sources are read-only
    everyone = np.ones(int(off[-1]), bool)
    cap = 1 << (H * W).bit_length()
    shift, (_, field, tile) = motions(H, W)[1][0], motions(H, W)[3]
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    plain = c_links(lab, off, cap)
    assert plain[0].any() and same(c_links_gap(lab, off, cap, 1, everyone, everyone), plain)
    assert same(c_links_gap(lab, off, cap, 1, everyone, everyone, np.zeros((T_RAW, 2), np.int32)), plain)
    assert same(c_links_gap(lab, off, cap, 1, everyone, everyone, shift), c_links_shifted(lab, off, cap, shift))
    assert same(c_links_gap(lab, off, cap, 1, everyone, everyone, field, tile), c_links_field(lab, off, cap, field, tile))


def constructed():
    """T = 3, 6 x 21, frame 2 against frame 0 (gap 2); one case per row (pair).  -> (labels int32, label_off, want, open,
    {label of frame 2: (pred, overlap)})"""
    lab = np.zeros((3, 6, 21), np.int32)
    src, dst = lab[0], lab[2]
    # rows 0 - 1: the largest partner (source 1, 14 px) is not open: the second largest open one (source 2, 6 px against 4)
    dst[0:2, 0:12] = 1
    src[0:2, 0:7], src[0:2, 7:10], src[0:2, 10:12] = 1, 2, 3
    # row 2: an exact tie (4 px each) goes to the smaller label, which comes second in the row
    dst[2, 0:8] = 2
    src[2, 0:4], src[2, 4:8] = 5, 4
    # row 3: the wanted cell 3 starts at the last pixel of the first lane (x = 7) and goes on in the second; the cell before
    # it (4) is not wanted, though it lies on the same open source
    dst[3, 0:7], dst[3, 7:13] = 4, 3
    src[3, 5:13] = 6
    # row 4: a wanted cell that touches the last column (21 = 2 * 8 + 5: the row's tail lane)
    dst[4, 16:21] = 5
    src[4, 14:21] = 7
    # row 5: ids beyond their frame's table (frame 0 holds 7 cells, frame 2 holds 5): no cells, and no index into the flags;
    # cell 5 of frame 2 over such an id pairs with nothing there
    src[5, 0:11] = 9
    dst[5, 0:6] = 8
    dst[5, 8:11] = 5
    lab[1, 1:5, 2:19] = 1
    lab[1, 0, 0:21] = 2
    off = np.array([0, 7, 9, 14], np.int64)
    want, open_ = np.ones(14, bool), np.ones(14, bool)
    want[9 + 4 - 1] = False
    open_[1 - 1] = False
    return lab, off, want, open_, {1: (2, 6), 2: (4, 4), 3: (6, 6), 4: (0, 0), 5: (7, 5)}


@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
def test_links_gap_constructed_frames(label_dtype):
    base_lab, off, want, open_, expected = constructed()
    lab = base_lab.astype(label_dtype)
    want_pred, want_ovl = gref.links_gap(base_lab, off, 2, want, open_)
    assert {l: (int(want_pred[9 + l - 1]), int(want_ovl[9 + l - 1])) for l in expected} == expected
    for cap in (64, 256):
        pred, ovl, status = c_links_gap(lab, off, cap, 2, want, open_)
        assert not status.any() and np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
        assert not pred[:9].any()
        # the same under a zero shift and a zero field
        for moved, tile in ((np.zeros((3, 2), np.int32), 0), (np.zeros((3, 1, 1, 2), np.int32), 64)):
            again = c_links_gap(lab, off, cap, 2, want, open_, moved, tile)
            assert again[0].tobytes() == pred.tobytes() and again[1].tobytes() == ovl.tobytes()
    # with the largest partner open it wins; with the unwanted cell wanted it is linked
    everyone = np.ones(14, bool)
    pred, ovl, _ = c_links_gap(lab, off, 64, 2, everyone, everyone)
    assert (pred[9], ovl[9]) == (1, 14) and (pred[9 + 3], ovl[9 + 3]) == (6, 2)
    assert np.array_equal(pred, gref.links_gap(base_lab, off, 2, everyone, everyone)[0])


def test_links_gap_beyond_the_stack_gives_zeros_and_bad_arguments_are_refused():
    H, W = SHAPES[0]
    base_lab, off, want, open_ = raw_case(H, W)
    for T, g in ((3, 3), (3, 5), (1, 1), (2, 2)):
        lab = base_lab[:T].astype(np.uint16)
        n = int(off[T])
        pred, ovl, status = c_links_gap(lab, off[:T + 1], 64, g, want[:n], open_[:n])
        assert not pred.any() and not ovl.any() and not status.any(), (T, g)
    lab = base_lab.astype(np.uint16)
    shift = np.zeros((T_RAW, 2), np.int32)
    field = np.zeros((T_RAW,) + fref.tiles(H, W, 64) + (2,), np.int32)
    for g, moved, tile in ((0, None, 0), (6, None, 0), (-1, shift, 0), (2, None, 64), (2, None, 100), (2, field, 100),
                           (2, field, 32), (2, shift, 1)):
        c_links_gap(lab, off, 16384, g, want, open_, moved, tile, expect=EINVAL)
    assert c_links_gap(lab, off, 16384, 5, want, open_, field, 64) is not None


def test_links_gap_table_overflow_and_the_wrapper_redoes():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab = random_small_labels()                                # 3 x 96 x 128, about 2000 cells of 2 x 3 pixels per frame
    off = ref.frame_tables(lab)
    rng = np.random.default_rng(11)
    want, open_ = rng.random(int(off[-1])) < 0.3, rng.random(int(off[-1])) < 0.3
    assert want[int(off[2]):].sum() > 300 and open_[:int(off[1])].sum() > 300
    shift = np.array([(0, 0), (0, 0), (1, -2)], np.int32)
    for moved in (None, shift):
        want_pred, want_ovl = gref.links_gap(lab, off, 2, want, open_, moved)
        assert np.count_nonzero(want_pred) > 100
        pred, ovl, status = c_links_gap(lab, off, 16384, 2, want, open_, moved)      # more entries than pixels: cannot fill up
        assert not status.any() and np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
        _, _, status = c_links_gap(lab, off, 64, 2, want, open_, moved)              # the smallest table fills up and says so
        assert status[0] == 0 and status[1] == 0 and status[2] != 0
        pred, ovl = cells.link_gap_raw(_dev(lab), _lib.PIX_U16, off, 2, want, open_, shift=moved, table_cap=64)
        assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
        pred, ovl = cells.link_gap_raw(_dev(lab), _lib.PIX_U16, off, 2, want, open_, shift=moved)
        assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
    with pytest.raises(ValueError, match="field"):
        cells.link_gap_raw(_dev(lab), _lib.PIX_U16, off, 2, want, open_, field=np.zeros((3, 2, 2, 2), np.int32))
    with pytest.raises(ValueError, match="want"):
        cells.link_gap_raw(_dev(lab), _lib.PIX_U16, off, 2, want[:-1], open_)


# ---- measure_cells(gap=...) -----------------------------------------------------------------------------------------------------
def check_whole(df, want, drift=False, flow=False, gap=True):
    """the whole table against gap_ref.table: the columns of the plain table as test_gpu_cells checks them, every other
    column (drift, flow, pred_gap) exactly"""
    from microbeseg_amd.inference import cells
    cols = cells.columns([], True, drift, flow=flow, gap=gap)
    assert list(df.columns) == cols == [c for c in want.columns if c != "_skip"]
    plain = cells.columns([], True)
    check_table(df[plain], want[plain + ["_skip"]], [], True)
    for col in cols:
        if col not in plain:
            a, b = df[col].to_numpy(), want[col].to_numpy()
            assert a.dtype.kind == b.dtype.kind and np.array_equal(a, b), col


def test_measure_cells_closes_the_gaps_of_the_base_stack():
    from microbeseg_amd.inference import cells
    lab = np.array(base_stack())
    none = cells.measure_cells(lab)
    assert "pred_gap" not in none.columns and none["track_id"].nunique() == 5
    check_table(none, ref.table(lab), [], True)
    assert cells.measure_cells(lab, gap=None).to_csv() == none.to_csv()
    at = lambda df, t, l: df[(df["frame"] == t) & (df["label"] == l)].iloc[0]
    tables = {}
    for G, n_tracks in ((1, 4), (2, 3), (4, 3)):
        df = tables[G] = cells.measure_cells(lab, gap=G)
        check_whole(df, gref.table(lab, gap=G))
        assert df["track_id"].nunique() == n_tracks
        assert at(df, 3, 1)["pred_gap"] == 2 and at(df, 3, 1)["pred_label"] == 1
        assert at(df, 4, 3)["pred_gap"] == (3 if G >= 2 else 0)
        same = [c for c in none.columns if c not in ("pred_label", "overlap", "track_id", "parent_track")]
        assert df[same].equals(none[same])
    # int32 labels on the device, an image alongside: the link columns stay
    img = np.random.default_rng(3).integers(0, 256, (6, 1) + BASE_SHAPE).astype(np.uint8)
    df = cells.measure_cells(torch.from_numpy(lab.astype(np.int32)).cuda(), img, gap=2)
    assert list(df.columns) == cells.columns([0], True, gap=True)
    for col in ("pred_label", "overlap", "pred_gap", "track_id", "parent_track"):
        assert np.array_equal(df[col].to_numpy(), tables[2][col].to_numpy())
    # min_overlap decides over a closed gap as over an ordinary link: A shares 8 x 12 pixels across its gap
    assert at(cells.measure_cells(lab, gap=1, min_overlap=96), 3, 1)["pred_gap"] == 2
    high = cells.measure_cells(lab, gap=1, min_overlap=97)
    check_whole(high, gref.table(lab, gap=1, min_overlap=97))
    assert at(high, 3, 1)["pred_gap"] == 0


def test_measure_cells_continuing_cell_and_division_across_a_gap():
    from microbeseg_amd.inference import cells
    lab = np.array(division_stack())
    none, one = cells.measure_cells(lab), cells.measure_cells(lab, gap=1)
    check_division_table(none, one)
    check_whole(one, gref.table(lab, gap=1))


def test_measure_cells_closes_gaps_under_drift_and_flow():
    from microbeseg_amd.inference import cells
    still = cells.measure_cells(np.array(base_stack()), gap=2)
    lab, _ = moved_stack(base_stack(), (5, 6))
    off = ref.frame_tables(lab)
    shift = dref.pick(dref.scores(lab, off, 8))
    assert shift[1:].tolist() == [[5, 6]] * 5
    df = cells.measure_cells(lab, drift=8, gap=2)
    check_whole(df, gref.table(lab, gap=2, shift=shift), drift=True)
    for col in ("track_id", "parent_track", "pred_gap"):
        assert np.array_equal(df[col].to_numpy(), still[col].to_numpy()), col
    assert df["track_id"].nunique() == 3
    # two steps of (5, 6) outrun the 8 px cell height: without the composed shift nothing is joined
    assert cells.measure_cells(lab, gap=2)["pred_gap"].max() <= 1
    # the same under a field, on a 96 x 150 canvas (2 x 3 tiles of 64 px with partial tiles)
    wide = np.zeros((6, 96, 150), np.uint16)
    wide[:, 10:10 + lab.shape[1], 30:30 + lab.shape[2]] = lab
    off = ref.frame_tables(wide)
    shift = dref.pick(dref.scores(wide, off, 8))
    field = fref.pick(fref.scores(wide, off, shift, 4, 64), shift)
    df = cells.measure_cells(wide, drift=8, flow=4, gap=2)
    check_whole(df, gref.table(wide, gap=2, shift=shift, field=field, tile=64), drift=True, flow=True)
    for col in ("track_id", "parent_track", "pred_gap"):
        assert np.array_equal(df[col].to_numpy(), still[col].to_numpy()), col


@functools.lru_cache(maxsize=None)
def blinking_stack(seed=18):
    """T = 8, 96 x 128: 30 static ellipses that do not touch, cell k (id k + 1) blanked in every frame with probability 0.15
    -> (labels uint16, shown bool [8, 30]); read only.  With this seed the stretches of missed frames between two appearances
    of a cell are 1, 2, 3 and 4 frames long (18, 2, 1 and 1 of them), so gap = 1, 2 and 4 each close another set"""
    rng = np.random.default_rng(seed)
    T, H, W, n = 8, 96, 128, 30
    yy, xx = np.mgrid[:H, :W]
    placed = []
    for _ in range(5000):
        if len(placed) == n:
            break
        cy, cx, a, b, th = rng.uniform(6, H - 6), rng.uniform(6, W - 6), rng.uniform(3, 6), rng.uniform(2, 3), rng.uniform(0, np.pi)
        if all((cy - p[0]) ** 2 + (cx - p[1]) ** 2 > (a + p[2] + 2) ** 2 for p in placed):
            placed.append((cy, cx, a, b, th))
    assert len(placed) == n
    shown = rng.random((T, n)) >= 0.15
    lab = np.zeros((T, H, W), np.uint16)
    for k, (cy, cx, a, b, th) in enumerate(placed):
        u, v = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th), -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
        inside = (u / a) ** 2 + (v / b) ** 2 <= 1
        for t in range(T):
            if shown[t, k]:
                lab[t][inside] = k + 1
    lab.setflags(write=False)
    shown.setflags(write=False)
    return lab, shown


@pytest.mark.parametrize("G", [1, 2, 4])
def test_measure_cells_on_a_stack_of_blinking_cells(G):
    from microbeseg_amd.inference import cells
    lab, shown = blinking_stack()
    df = cells.measure_cells(np.array(lab), gap=G)
    check_whole(df, gref.table(lab, gap=G))
    # static cells overlap only themselves: every stretch of at most G missed frames between two appearances is closed onto
    # the cell's own earlier label, every longer one starts a new track
    rows = {(int(f), int(l)): (int(p), int(g), int(tr)) for f, l, p, g, tr in
            zip(df["frame"], df["label"], df["pred_label"], df["pred_gap"], df["track_id"])}
    stretches = np.concatenate([np.diff(np.nonzero(shown[:, k])[0]) - 1 for k in range(shown.shape[1])])
    assert [int((stretches == m).sum()) for m in (1, 2, 3, 4)] == [18, 2, 1, 1] and stretches.max() == 4
    closed = longer = 0
    for k in range(shown.shape[1]):
        frames = np.nonzero(shown[:, k])[0]
        assert all((int(t), k + 1) in rows for t in frames)
        for a, b in zip(frames[:-1], frames[1:]):
            pred, gap, track = rows[(int(b), k + 1)]
            if b - a - 1 <= G:
                assert (pred, gap) == (k + 1, b - a) and track == rows[(int(a), k + 1)][2], (k, a, b)
                closed += b - a > 1
            else:
                assert (pred, gap) == (0, 0) and track != rows[(int(a), k + 1)][2], (k, a, b)
                longer += 1
    assert (closed, longer) == {1: (18, 4), 2: (20, 2), 4: (22, 0)}[G]
    expected_tracks = sum(1 + int(np.count_nonzero(np.diff(np.nonzero(shown[:, k])[0]) - 1 > G)) for k in range(shown.shape[1])
                          if shown[:, k].any())
    assert df["track_id"].nunique() == expected_tracks and not df["parent_track"].any()


def test_the_worker_passes_gap_on():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab = np.array(base_stack())
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    assert worker.gap is None and worker.cell_table(lab).equals(cells.measure_cells(lab))
    worker.gap = 2
    got = worker.cell_table(lab)
    assert "pred_gap" in got.columns and got.equals(cells.measure_cells(lab, gap=2)) and got["track_id"].nunique() == 3
