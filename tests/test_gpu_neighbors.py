"""GPU (MI355X): the per-cell neighbourhood (csrc/neighbors.hip) through the C ABI, through neighbors_raw /
measure_cells / cell_contacts and through the command line, every integer equal to the restatement tests/neighbors_ref.py
(which test_neighbors_host.py checks on the CPU).  All comparisons are exact."""
import ctypes as C
import functools
import math

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
import hull_ref as href
import neighbors_ref as nref
from test_gpu_cells import PIX, Guarded, _dev
from test_hull_host import random_cells
from test_neighbors_host import CONTACT_COLUMNS, NEIGHBOR_COLUMNS

pytestmark = pytest.mark.gpu
EINVAL, EWORKSPACE = -1, -3
SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (33, 200), (70, 131)]
RADII = (1, 2, 8, 32)
TILE_H, TILE_W = 32, 64                 # NB_TH, NB_TW of csrc/neighbors.hip


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def c_neighbors(lab, off, R, cap=None, pair_cap=None, short=0, dtype_code=None, no_pairs=False):
    """mseg_cell_neighbors through ctypes -> (return code, guarded out [9, n], pairs [pair_cap, 5], n_pairs [1], status [T]);
    by default with a table that cannot fill up (the speckled cells of the scenes are all over their frames: almost every
    pair of them exists) and room for every possible pair"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    all_pairs = [int(k) * (int(k) - 1) // 2 for k in np.diff(off)]
    cap = max(64, 1 << max(all_pairs, default=0).bit_length()) if cap is None else cap
    pair_cap = max(sum(all_pairs), 1) if pair_cap is None else pair_cap
    lab_d, off_d = _dev(np.array(lab)), torch.from_numpy(np.array(off, np.int64)).cuda()
    out, pairs = Guarded((9, n), torch.int64), Guarded((pair_cap, 5), torch.int32)
    n_pairs, status = Guarded((1,), torch.int64), Guarded((T,), torch.int32)
    nbytes = lib.mseg_cell_neighbors_workspace_bytes(T, n, cap if cap >= 64 and cap & (cap - 1) == 0 else 64)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    code = lib.mseg_cell_neighbors(lab_d.data_ptr(), PIX[lab.dtype] if dtype_code is None else dtype_code, T, H, W,
                                   off_d.data_ptr(), n, R, cap, out.ptr, None if no_pairs else pairs.ptr,
                                   0 if no_pairs else pair_cap, n_pairs.ptr, status.ptr, ws.data_ptr(), nbytes - short,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code, out, pairs, n_pairs, status


def sort_rows(rows):
    rows = np.asarray(rows, np.int32).reshape(-1, 5)
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


def neighbors_of(lab, off, R, cap=None):
    """the valid outputs of one call: (int64 [9, n], the pair rows sorted)"""
    code, out, pairs, n_pairs, status = c_neighbors(lab, off, R, cap)
    assert code == 0 and not status.host(np.int32).any()
    m = int(n_pairs.host(np.int64)[0])
    assert m <= pairs.shape[0]
    return out.host(np.int64), sort_rows(pairs.host(np.int32)[:m])


@functools.lru_cache(maxsize=None)
def scene(H, W, R):
    """random rectangles plus speckle, 4 frames -> (int64 labels, label_off, reference planes, reference pair rows); read only"""
    lab = random_cells(H, W, T=4, seed=3)
    off = ref.frame_tables(lab)
    want, rows = nref.neighbors(lab, off, R)
    for a in (lab, off, want, rows):
        a.setflags(write=False)
    return lab, off, want, rows


# ---- against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_outputs_equal_the_restatement(shape, R, label_dtype):
    lab, off, want, rows = scene(*shape, R)
    assert want[1].any()
    if shape[1] >= 63:
        assert want[0].any() and want[2].any() and len(rows) > 0
    for T in (1, 4):
        n = int(off[T])
        got, got_rows = neighbors_of(lab[:T].astype(label_dtype), off[:T + 1], R)
        assert got.shape == (9, n) and np.array_equal(got, want[:, :n]), T
        assert np.array_equal(got_rows, rows[rows[:, 0] < T]), T


def test_ids_outside_the_table_are_not_a_cell():
    lab = np.array(scene(33, 200, 8)[0][:2], np.int32)
    k0 = int(lab[0].max())
    lab[0, 5:12, 40:90] = k0 + 3                                # beyond the table, amid the cells
    lab[0, 20:26, 100:160] = -7
    lab[1, 2:30, 60:64] = -2 ** 31
    lab[1][lab[1] == 2] = 0                                     # an absent id inside the table
    off = np.array([0, k0, k0 + int(lab[1].max())], np.int64)
    want, rows = nref.neighbors(lab, off, 8)
    assert not want[:, k0 + 1].any() and want[2].any()
    got, got_rows = neighbors_of(lab, off, 8)
    assert np.array_equal(got, want) and np.array_equal(got_rows, rows)
    short = np.array([0, k0 - 2, k0 - 2 + 3], np.int64)         # a shorter table: the ids it drops are background now
    want, rows = nref.neighbors(lab, short, 8)
    got, got_rows = neighbors_of(lab, short, 8)
    assert np.array_equal(got, want) and np.array_equal(got_rows, rows)


# ---- tile seams -----------------------------------------------------------------------------------------------------------------
def _block(frame, y, x, l):
    assert 0 <= y and y + 3 <= frame.shape[0] and 0 <= x and x + 3 <= frame.shape[1]
    frame[y:y + 3, x:x + 3] = l


@pytest.mark.parametrize("R", [1, 8, 32])
def test_pairs_across_tile_seams(R):
    """two 3 x 3 cells, 1 before 2 in raster order or not, with a gap of g background columns / rows: edges 3 and d2 1 for
    g == 0, else edges 0 and d2 (g + 1)^2, existing exactly when g + 1 <= R; diagonally (dy, dx) apart: d2 = dy^2 + dx^2"""
    H, W = 120, 230                                              # tiles of 32 x 64: seams at rows 32, 64, 96, columns 64, 128, 192
    assert H % TILE_H and W % TILE_W
    frames, expect = [], []

    def add(y1, x1, y2, x2, d2, edges):
        f = np.zeros((H, W), np.uint16)
        _block(f, y1, x1, 1)
        _block(f, y2, x2, 2)
        frames.append(f)
        expect.append([(1, 2, edges, d2)] if d2 <= R * R else [])

    for g in (R - 1, R):
        lo, hi, edges = g // 2, g - g // 2, 3 if g == 0 else 0
        for bx in range(TILE_W, W, TILE_W):                      # side by side across a vertical seam
            add(40, bx - lo - 3, 40, bx + hi, (g + 1) ** 2, edges)
        for by in range(TILE_H, H, TILE_H):                      # one above the other across a horizontal seam
            add(by - lo - 3, 70, by + hi, 70, (g + 1) ** 2, edges)
        add(H - 3, W - 6 - g, H - 3, W - 3, (g + 1) ** 2, edges)  # in the last rows, up to the last column
        add(H - 6 - g, W - 3, H - 3, W - 3, (g + 1) ** 2, edges)  # in the last columns, down to the last row
    for d in (math.isqrt(R * R // 2), math.isqrt(R * R // 2) + 1):
        if d < 2:
            d = 1                                                # R = 1: corner to corner, d2 = 2 > 1
        lo, hi = (d - 1) // 2, d - 1 - (d - 1) // 2
        for by in range(TILE_H, H, TILE_H):
            for bx in range(TILE_W, W, TILE_W):                  # across a tile corner, down-right and down-left
                add(by - lo - 3, bx - lo - 3, by + hi, bx + hi, 2 * d * d, 0)
                add(by - lo - 3, bx + hi, by + hi, bx - lo - 3, 2 * d * d, 0)
    lab = np.stack(frames)
    T = len(frames)
    off = 2 * np.arange(T + 1, dtype=np.int64)
    got, rows = neighbors_of(lab, off, R)
    assert any(expect) and not all(expect)
    for t in range(T):
        pair = [tuple(int(v) for v in r[1:]) for r in rows[rows[:, 0] == t]]
        assert pair == expect[t], (t, pair, expect[t])
        per = 12                                                 # the perimeter of a 3 x 3 cell, border edges included
        a, b = got[:, 2 * t].tolist(), got[:, 2 * t + 1].tolist()
        if expect[t]:
            _, _, e, d2 = expect[t][0]
            assert a[0] == b[0] == e and a[3:] == [int(e > 0), 1, 2, d2, 2 if e else 0, e], (t, a)
            assert b[3:] == [int(e > 0), 1, 1, d2, 1 if e else 0, e], (t, b)
        else:
            assert a[0] == b[0] == 0 and not any(a[3:]) and not any(b[3:]), (t, a, b)
        assert sum(a[:3]) == per and sum(b[:3]) == per


# ---- the table fills up, the rows do not fit ----------------------------------------------------------------------------------------
def test_full_table_sets_the_status_words_and_the_wrapper_redoes_the_frames():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab64, off, want, rows = scene(70, 131, 8)
    lab = lab64.astype(np.uint16)
    assert all((rows[:, 0] == t).sum() > 64 for t in range(4))  # every frame has more existing pairs than the table holds
    code, out, pairs, n_pairs, status = c_neighbors(lab, off, 8, cap=64)
    assert code == 0 and status.host(np.int32).all()
    out.host(np.int64), pairs.host(np.int32)                    # the guard bands are intact
    assert 0 < int(n_pairs.host(np.int64)[0]) <= 4 * 64
    ints, got_rows = cells.neighbors_raw(_dev(lab), _lib.PIX_U16, off, 8, table_cap=64)
    assert ints.dtype == np.int64 and got_rows.dtype == np.int32
    assert np.array_equal(ints, want) and np.array_equal(got_rows, rows)
    ints, got_rows = cells.neighbors_raw(_dev(lab), _lib.PIX_U16, off, 8)
    assert np.array_equal(ints, want) and np.array_equal(got_rows, rows)


def test_small_pair_cap_gives_the_full_count_and_writes_no_further_row():
    lab64, off, want, rows = scene(70, 131, 8)
    lab = lab64.astype(np.int32)
    for pair_cap in (10, 1):
        code, out, pairs, n_pairs, status = c_neighbors(lab, off, 8, pair_cap=pair_cap)
        assert code == 0 and not status.host(np.int32).any()
        assert int(n_pairs.host(np.int64)[0]) == len(rows) > pair_cap
        assert np.array_equal(out.host(np.int64), want)
        some = pairs.host(np.int32)                             # asserts the guard bands; every row written is a pair
        assert all(r.tolist() in rows.tolist() for r in some) and len({tuple(r) for r in some.tolist()}) == pair_cap
    code, out, pairs, n_pairs, status = c_neighbors(lab, off, 8, no_pairs=True)
    assert code == 0 and pairs.untouched() and int(n_pairs.host(np.int64)[0]) == len(rows)
    assert np.array_equal(out.host(np.int64), want)


def test_two_calls_give_identical_bytes():
    lab, off, want, rows = scene(70, 131, 8)
    (a, ra), (b, rb) = (neighbors_of(lab.astype(np.uint16), off, 8) for _ in range(2))
    assert a.tobytes() == b.tobytes() == want.tobytes() and ra.tobytes() == rb.tobytes() == rows.tobytes()


def test_argument_errors_touch_nothing():
    from microbeseg_amd import _lib
    lib = _lib.load()
    lab, off, _, _ = scene(5, 65, 8)
    lab = lab.astype(np.uint16)
    bad_calls = [dict(dtype_code=0), dict(dtype_code=3), dict(R=0), dict(R=33), dict(cap=96), dict(cap=32), dict(cap=0)]
    for kw in bad_calls:
        code, *bufs = c_neighbors(lab, off, kw.pop("R", 8), **kw)
        assert code == EINVAL and all(b.untouched() for b in bufs), kw
    code, *bufs = c_neighbors(lab, off, 8, short=1)
    assert code == EWORKSPACE and all(b.untouched() for b in bufs)
    n = int(off[-1])
    assert lib.mseg_cell_neighbors_workspace_bytes(4, n, 96) == 0 and lib.mseg_cell_neighbors_workspace_bytes(4, n, 32) == 0
    assert lib.mseg_cell_neighbors_workspace_bytes(0, n, 64) == 0 and lib.mseg_cell_neighbors_workspace_bytes(4, -1, 64) == 0
    assert lib.mseg_cell_neighbors_workspace_bytes(4, n, 2 ** 32) == 0
    assert lib.mseg_cell_neighbors_workspace_bytes(4, n, 1024) >= 4 * 1024 * 16 + 16 * n
    code, out, pairs, n_pairs, status = c_neighbors(lab, np.zeros(5, np.int64), 8)           # no cells: no launch
    assert code == 0 and out.untouched() and pairs.untouched()
    assert not status.host(np.int32).any() and n_pairs.host(np.int64)[0] == 0


# ---- measure_cells(neighbors=8), cell_contacts ------------------------------------------------------------------------------------
def test_measure_cells_with_neighbors():
    from microbeseg_amd.inference import cells
    lab64, off, ints, rows = scene(70, 131, 8)
    lab = lab64.astype(np.uint16)
    H, W = lab.shape[1:]
    img = np.random.default_rng(5).integers(0, 65536, (4, 1, H, W)).astype(np.uint16)
    df = cells.measure_cells(lab, img, neighbors=8)
    assert list(df.columns) == cells.columns([0], True, neighbors=True) and len(df) > 100
    want = cells.table_from_sums(off, H, W, ref.measure(lab, off, img), channels=[0], links=ref.links(lab, off),
                                 neighbors=ints)
    pd.testing.assert_frame_equal(df[NEIGHBOR_COLUMNS], want[NEIGHBOR_COLUMNS], check_exact=True)
    plain = cells.measure_cells(lab, img)
    assert list(plain.columns) == cells.columns([0], True)
    pd.testing.assert_frame_equal(df[list(plain.columns)], plain, check_exact=True)
    assert cells.measure_cells(lab.astype(np.int32), img, neighbors=8).to_csv().encode() == df.to_csv().encode()
    bare = cells.measure_cells(lab, link=False, neighbors=8)    # needs neither link, hull nor an image
    assert list(bare.columns) == cells.columns([], False, neighbors=True) and bare[NEIGHBOR_COLUMNS].equals(df[NEIGHBOR_COLUMNS])
    both = cells.measure_cells(lab, drift=2, hull=True, neighbors=8)
    assert list(both.columns) == cells.columns([], True, True, True, neighbors=True)
    assert both[NEIGHBOR_COLUMNS].equals(df[NEIGHBOR_COLUMNS])
    assert (both["contact_length"] + both["border_length"] <= both["perimeter"]).all()
    present = ref.measure(lab, off)["shape"][0] > 0
    assert np.array_equal(ints[:3].sum(axis=0)[present], both["perimeter"].to_numpy())
    assert np.array_equal(ints[:3].sum(axis=0), href.hull(lab, off)[0])
    with pytest.raises(ValueError, match="neighbors"):
        cells.measure_cells(lab, neighbors=33)


def test_cell_contacts():
    from microbeseg_amd.inference import cells
    lab64, off, _, rows = scene(70, 131, 8)
    for lab in (lab64.astype(np.uint16), lab64.astype(np.int32), torch.from_numpy(lab64.astype(np.int32)).cuda()):
        df = cells.cell_contacts(lab)                            # the default radius is 8
        assert list(df.columns) == CONTACT_COLUMNS and len(df) == len(rows)
        assert df[CONTACT_COLUMNS[:4]].to_numpy().tolist() == rows[:, :4].tolist()
        assert df["distance"].tolist() == [math.sqrt(int(v)) for v in rows[:, 4]]
    rows2 = scene(70, 131, 2)[3]
    df = cells.cell_contacts(lab64.astype(np.uint16), radius=2)
    assert df[CONTACT_COLUMNS[:4]].to_numpy().tolist() == rows2[:, :4].tolist() and len(rows2) < len(rows)
    with pytest.raises(ValueError, match="neighbors"):
        cells.cell_contacts(lab64.astype(np.uint16), radius=0)


def test_infer_worker_passes_neighbors_on():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    lab = scene(33, 200, 2)[0].astype(np.uint16)
    worker = InferWorker.__new__(InferWorker)
    worker.device = torch.device("cuda:0")
    assert worker.neighbors is None
    assert list(worker.cell_table(lab).columns) == cells.columns([], link=True)
    worker.neighbors = 2
    df = worker.cell_table(lab)
    assert list(df.columns) == cells.columns([], True, neighbors=True) and df.equals(cells.measure_cells(lab, neighbors=2))
    contacts = worker.contact_table(lab)
    assert contacts.equals(cells.cell_contacts(lab, 2)) and len(contacts) == len(scene(33, 200, 2)[3])


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_infer_script_neighbors_end_to_end(tmp_path):
    import subprocess
    import sys
    from microbeseg_amd.inference.cells import columns, measure_cells
    from microbeseg_amd.utils import synth, tiffio
    from test_cells_host import ROOT
    from test_gpu_analysis import _constant_distance_model
    model = _constant_distance_model(tmp_path / "distance_model_00")      # one cell per frame, whatever the input
    rng = np.random.Generator(np.random.PCG64(9))
    stack = np.stack([synth.synth_crop(rng, 128)["img"] for _ in range(2)])
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    tiffio.imwrite(str(imgs / "movie.tif"), stack)
    cmd = [sys.executable, str(ROOT / "infer_script_local.py"), "-i", str(imgs), "-m", str(model), "--cells"]
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    r = subprocess.run(cmd + ["-r", str(plain)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "neighbourhood" not in r.stdout
    r = subprocess.run(cmd + ["-r", str(flagged), "--neighbors"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Cell table: with the neighbourhood of every cell within 8 px" in r.stdout
    assert sorted(p.name for p in plain.iterdir()) == ["mask_movie_channel0.tif", "mask_movie_channel0_cells.csv"]
    assert sorted(p.name for p in flagged.iterdir()) == ["mask_movie_channel0.tif", "mask_movie_channel0_cells.csv",
                                                         "mask_movie_channel0_contacts.csv"]
    assert (plain / "mask_movie_channel0.tif").read_bytes() == (flagged / "mask_movie_channel0.tif").read_bytes()
    mask = tiffio.imread(str(plain / "mask_movie_channel0.tif"))
    assert (plain / "mask_movie_channel0_cells.csv").read_bytes() == measure_cells(mask, stack).to_csv(index=False).encode()
    read = lambda path: pd.read_csv(path, float_precision="round_trip")
    df, old = read(flagged / "mask_movie_channel0_cells.csv"), read(plain / "mask_movie_channel0_cells.csv")
    assert list(df.columns) == columns([0], True, neighbors=True) and list(old.columns) == columns([0], True)
    pd.testing.assert_frame_equal(df[list(old.columns)], old, check_exact=True)
    pd.testing.assert_frame_equal(df, measure_cells(mask, stack, neighbors=8), check_exact=True, check_dtype=False)
    assert df["n_neighbors"].tolist() == [0, 0] and df["nn_distance"].isna().all() and (df["contact_fraction"] == 0).all()
    contacts = read(flagged / "mask_movie_channel0_contacts.csv")
    assert list(contacts.columns) == CONTACT_COLUMNS and len(contacts) == 0
