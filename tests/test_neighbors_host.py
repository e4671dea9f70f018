"""CPU: the per-cell neighbourhood — the two restatements of tests/neighbors_ref.py against each other, against
the perimeter of tests/hull_ref.py and against closed forms, the boundary-pixel argument, the columns and their formulas, the
--neighbors flag and the declarations."""
import functools
import math
import pathlib
import re
import sys

import numpy as np
import pytest

import cells_ref as ref
import hull_ref as href
import neighbors_ref as nref
from test_hull_host import has_hole, is_disconnected, random_cells

ROOT = pathlib.Path(__file__).resolve().parents[1]
NEIGHBOR_COLUMNS = ["contact_length", "border_length", "contact_fraction", "n_touching", "n_neighbors", "nn_label",
                    "nn_distance", "nn_gap", "contact_label", "contact_max"]
CONTACT_COLUMNS = ["frame", "label_a", "label_b", "contact", "distance"]
RADII = (1, 2, 3, 8, 32)


# ---- the restatements -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_frames():
    """(frame, K) of 96 random frames up to 12 x 14 with > 150 cells between them; read only"""
    frames = []
    for seed in range(24):
        for H, W in ((12, 14), (9, 13), (7, 10), (12, 5)):
            frame = random_cells(H, W, seed=seed)[0]
            frame.setflags(write=False)
            frames.append((frame, int(frame.max())))
    return frames


@functools.lru_cache(maxsize=None)
def brute_of(i, R):
    frame, K = small_frames()[i]
    return nref.brute(frame, K, R)


def test_brute_and_windowed_agree_on_random_small_cells():
    frames = small_frames()
    cells = sum(len(np.unique(f[f > 0])) for f, _ in frames)
    assert cells >= 150
    apart = holed = 0
    for frame, K in frames:
        for l in np.unique(frame[frame > 0]):
            apart += is_disconnected(frame == l)
            holed += has_hole(frame == l)
    corner = gap = touching = 0
    for R in RADII:
        for i, (frame, K) in enumerate(frames):
            a, b = brute_of(i, R), nref.windowed(frame, K, R)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], (frame.shape, i, R)
            out, rows = a
            assert (out[3] <= out[4]).all() and all(r[3] <= R * R for r in rows)
            corner += sum(1 for r in rows if r[2] == 0 and r[3] == 2)
            gap += sum(1 for r in rows if r[2] == 0 and r[3] >= 4)
            touching += sum(1 for r in rows if r[2] > 0)
            if R == 1:
                assert all(r[3] == 1 and r[2] > 0 for r in rows)
    print(f"{cells} cells: {apart} disconnected, {holed} with a hole; pairs over all radii: {touching} share an edge, {corner} "
          f"meet at a corner only, {gap} lie across a gap")
    assert apart >= 5 and holed >= 5 and corner >= 5 and gap >= 5 and touching >= 5


def test_the_smallest_distance_is_attained_between_boundary_pixels():
    for R in RADII:
        for i, (frame, K) in enumerate(small_frames()):
            a, b = brute_of(i, R), nref.windowed(frame, K, R, boundary_only=True)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], (frame.shape, i, R)


def test_the_three_edge_kinds_sum_to_the_perimeter():
    for i, (frame, K) in enumerate(small_frames()):
        off = np.array([0, K], np.int64)
        out = brute_of(i, 3)[0]
        assert np.array_equal(out[0] + out[1] + out[2], href.hull(frame[None], off)[0]), i
    lab = random_cells(33, 60, T=2, seed=3)
    off = ref.frame_tables(lab)
    out = nref.neighbors(lab, off, 8)[0]
    assert np.array_equal(out[:3].sum(axis=0), href.hull(lab, off)[0]) and out[0].any() and out[1].any() and out[2].any()


def test_neighbors_stacks_frames_and_sorts_the_pairs():
    lab = random_cells(12, 14, T=3, seed=5)
    off = ref.frame_tables(lab)
    out, rows = nref.neighbors(lab, off, 3)
    assert out.shape == (9, off[-1]) and out.dtype == np.int64 and rows.dtype == np.int32 and rows.shape[1] == 5
    assert rows.tolist() == sorted(rows.tolist()) and set(rows[:, 0]) == {0, 1, 2} and (rows[:, 1] < rows[:, 2]).all()
    other = nref.neighbors(lab, off, 3, fn=nref.windowed)
    assert np.array_equal(out, other[0]) and np.array_equal(rows, other[1])
    for t in range(3):
        planes, pairs = nref.brute(lab[t], int(off[t + 1] - off[t]), 3)
        assert np.array_equal(out[:, off[t]:off[t + 1]], planes)
        assert rows[rows[:, 0] == t][:, 1:].tolist() == [list(r) for r in pairs]


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
FNS = [nref.brute, nref.windowed]


@pytest.mark.parametrize("fn", FNS)
def test_rectangles_side_by_side_and_across_a_gap(fn):
    for h, w in ((3, 4), (1, 1), (5, 2)):
        for g in (0, 1, 2, 3, 4):
            frame = np.zeros((h + 3, 2 * w + g + 2), np.int64)
            frame[1:1 + h, 1:1 + w] = 1
            frame[1:1 + h, 1 + w + g:1 + 2 * w + g] = 2
            for R in (1, 2, 3, 4, 8):
                out, rows = fn(frame, 2, R)
                per = 2 * (h + w)
                if g == 0:
                    assert rows == [(1, 2, h, 1)]
                    assert out[:, 0].tolist() == [h, 0, per - h, 1, 1, 2, 1, 2, h]
                    assert out[:, 1].tolist() == [h, 0, per - h, 1, 1, 1, 1, 1, h]
                elif g + 1 <= R:
                    assert rows == [(1, 2, 0, (g + 1) ** 2)]
                    assert out[:, 0].tolist() == [0, 0, per, 0, 1, 2, (g + 1) ** 2, 0, 0]
                else:
                    assert rows == [] and out[:, 0].tolist() == [0, 0, per, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("fn", FNS)
def test_rectangles_meeting_at_a_corner(fn):
    frame = np.zeros((7, 9), np.int64)
    frame[1:3, 1:4] = 1
    frame[3:6, 4:8] = 2
    assert fn(frame, 2, 1)[1] == [] and not fn(frame, 2, 1)[0][[0, 3, 4, 5, 6, 7, 8]].any()
    for R in (2, 3, 32):
        out, rows = fn(frame, 2, R)
        assert rows == [(1, 2, 0, 2)]
        assert out[:, 0].tolist() == [0, 0, 10, 0, 1, 2, 2, 0, 0] and out[:, 1].tolist() == [0, 0, 14, 0, 1, 1, 2, 0, 0]


@pytest.mark.parametrize("fn", FNS)
def test_a_cell_filling_the_frame_and_a_ring_around_a_disc(fn):
    for H, W in ((1, 1), (4, 7), (12, 3)):
        out, rows = fn(np.ones((H, W), np.int64), 1, 32)
        assert rows == [] and out[:, 0].tolist() == [0, 2 * (H + W), 0, 0, 0, 0, 0, 0, 0]
    frame = np.zeros((11, 11), np.int64)
    frame[1:10, 1:10] = 1                       # a ring, one pixel of background inside it, a 3 x 3 disc in the middle
    frame[3:8, 3:8] = 0
    frame[4:7, 4:7] = 2
    for R in (1, 2, 8):
        out, rows = fn(frame, 2, R)
        assert out[:3, 0].tolist() == [0, 0, 36 + 20] and out[:3, 1].tolist() == [0, 0, 12]
        assert rows == ([] if R == 1 else [(1, 2, 0, 4)])
    frame[3:8, 3:8] = 2                         # the disc fills the hole: every edge of the hole is a contact
    out, rows = fn(frame, 2, 1)
    assert rows == [(1, 2, 20, 1)] and out[:, 0].tolist() == [20, 0, 36, 1, 1, 2, 1, 2, 20]
    assert out[:, 1].tolist() == [20, 0, 0, 1, 1, 1, 1, 1, 20]
    frame[0:11, 0:11][frame == 0] = 1           # the ring reaches the frame's border
    out, _ = fn(frame, 2, 1)
    assert out[:3, 0].tolist() == [20, 44, 0]


@pytest.mark.parametrize("fn", FNS)
def test_ids_outside_the_table_negative_ids_and_absent_ids_are_not_a_cell(fn):
    frame = np.zeros((6, 9), np.int64)
    frame[1:3, 1:4] = 1
    frame[1:3, 4:6] = 7                         # beyond a table of 3, pressed against cell 1
    frame[3:5, 1:4] = -4                        # negative, below cell 1
    frame[3:5, 5:8] = 3                         # id 2 is absent
    out, rows = fn(frame, 3, 8)
    assert out.shape == (9, 3) and not out[:, 1].any()
    assert rows == [(1, 3, 0, 5)]
    assert out[:, 0].tolist() == [0, 0, 10, 0, 1, 3, 5, 0, 0] and out[:, 2].tolist() == [0, 0, 10, 0, 1, 1, 5, 0, 0]
    out7, rows7 = fn(frame, 7, 8)               # a table that holds 7: now a cell, and the nearest one
    assert (1, 7, 2, 1) in rows7 and out7[:, 0].tolist() == [2, 0, 8, 1, 2, 7, 1, 7, 2]
    assert fn(frame, 2, 8)[1] == [] and fn(frame, 2, 8)[0].shape == (9, 2)


@pytest.mark.parametrize("fn", FNS)
def test_ties_go_to_the_smaller_label(fn):
    frame = np.zeros((7, 9), np.int64)
    frame[2:5, 3:6] = 3                         # 3 x 3 in the middle; cells 4 and 2 share 3 edges with it, 1 and 5 are 2 away
    frame[2:5, 6:9] = 4
    frame[2:5, 0:3] = 2
    frame[0, 3:6] = 5
    frame[6, 3:6] = 1
    out, rows = fn(frame, 5, 2)
    assert out[:, 2].tolist() == [6, 0, 6, 2, 4, 2, 1, 2, 3]
    assert (1, 3, 0, 4) in rows and (3, 5, 0, 4) in rows
    frame[2:5, 0:3] = 0
    frame[2:5, 6:9] = 0                         # nothing touches any more: the nearest of 1 and 5 (both 2 away) is 1
    out, _ = fn(frame, 5, 2)
    assert out[:, 2].tolist() == [0, 0, 12, 0, 2, 1, 4, 0, 0]


# ---- columns ----------------------------------------------------------------------------------------------------------------------
def test_neighbor_columns():
    from microbeseg_amd.inference import cells
    assert cells.NEIGHBOR_COLUMNS == NEIGHBOR_COLUMNS and cells.CONTACT_COLUMNS == CONTACT_COLUMNS
    assert cells.MAX_NEIGHBOR_RADIUS == 32
    for args in (([1], True, True), ([], False, False), ([0, 2], True, False, True, True, (5, 50))):
        assert cells.columns(*args, neighbors=True) == cells.columns(*args) + NEIGHBOR_COLUMNS
        assert cells.columns(*args, neighbors=False) == cells.columns(*args)
    assert cells.columns() == cells.SHAPE_COLUMNS + cells.LINK_COLUMNS and "n_touching" not in cells.columns([1], True, True)
    assert cells.columns([1], True, False, True, True, (50,), True)[-10:] == NEIGHBOR_COLUMNS
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.neighbors is None and callable(InferWorker.contact_table)


def test_check_neighbors():
    from microbeseg_amd.inference.cells import check_neighbors
    assert check_neighbors(None) is None and check_neighbors(1) == 1 and check_neighbors(32) == 32
    assert check_neighbors(np.int64(8)) == 8 and type(check_neighbors(np.int64(8))) is int and check_neighbors(8.0) == 8
    for bad in (0, 33, -1, 2.5, True, "8", [8]):
        with pytest.raises(ValueError, match="neighbors"):
            check_neighbors(bad)


def test_float_columns_follow_the_formulas():
    from microbeseg_amd.inference import cells
    lab = random_cells(12, 14, T=3, seed=2)
    lab[2] = 0
    lab[2, 2:4, 2:5] = 1                        # a frame with one cell alone
    off = ref.frame_tables(lab)
    raw = ref.measure(lab, off)
    ints, pairs = nref.neighbors(lab, off, 2)
    plain = cells.table_from_sums(off, 12, 14, raw, links=ref.links(lab, off))
    df = cells.table_from_sums(off, 12, 14, raw, links=ref.links(lab, off), neighbors=ints)
    assert list(df.columns) == cells.columns([], True, neighbors=True) and len(df) == len(plain) > 5
    assert df[list(plain.columns)].equals(plain)
    assert cells.table_from_sums(off, 12, 14, raw, neighbors=ints).columns.tolist() == cells.columns([], False, neighbors=True)
    both = cells.table_from_sums(off, 12, 14, raw, hull=href.hull(lab, off), neighbors=ints)
    assert both.columns.tolist() == cells.columns([], False, False, True, neighbors=True)
    assert (both["contact_length"] + both["border_length"] <= both["perimeter"]).all()
    slots = [int(off[t]) + l - 1 for t, l in zip(df["frame"], df["label"])]
    alone = 0
    for row, s in zip(df.itertuples(index=False), slots):
        c, b, f, nt, nn, lbl, d2, cl, ce = (int(v) for v in ints[:, s])
        assert (row.contact_length, row.border_length, row.n_touching, row.n_neighbors) == (c, b, nt, nn)
        assert row.contact_fraction == c / (c + b + f) and 0 <= row.contact_fraction <= 1
        assert (row.nn_label, row.contact_label, row.contact_max) == (lbl, cl, ce)
        if lbl:
            assert row.nn_distance == math.sqrt(d2) and row.nn_gap == math.sqrt(d2) - 1 and row.nn_gap >= 0
        else:
            assert math.isnan(row.nn_distance) and math.isnan(row.nn_gap) and nn == 0 and cl == 0 and ce == 0
            alone += 1
    assert alone >= 1 and df["nn_label"].any()
    for name in ("contact_length", "border_length", "n_touching", "n_neighbors", "nn_label", "contact_label", "contact_max"):
        assert df[name].dtype.kind == "i", name
    for name in ("contact_fraction", "nn_distance", "nn_gap"):
        assert df[name].dtype.kind == "f", name
    contacts = cells.contacts_from_pairs(pairs)
    assert list(contacts.columns) == CONTACT_COLUMNS and len(contacts) == len(pairs) > 3
    assert contacts[CONTACT_COLUMNS[:4]].to_numpy().tolist() == pairs[:, :4].tolist()
    assert contacts["distance"].tolist() == [math.sqrt(int(v)) for v in pairs[:, 4]]
    empty = cells.contacts_from_pairs(np.zeros((0, 5), np.int32))
    assert list(empty.columns) == CONTACT_COLUMNS and len(empty) == 0 and empty["distance"].dtype.kind == "f"


# ---- command line -----------------------------------------------------------------------------------------------------------------
BASE = ["-i", "x", "-m", "y"]


def _parser():
    sys.path.insert(0, str(ROOT))
    import infer_script_local as script
    return script.build_parser()


def test_cli_neighbors():
    parser = _parser()
    assert parser.parse_args(BASE).neighbors is None and parser.parse_args(BASE + ["--cells"]).neighbors is None
    assert parser.parse_args(BASE + ["--cells", "--neighbors"]).neighbors == 8
    assert parser.parse_args(BASE + ["--neighbors", "--cells", "--hull"]).neighbors == 8
    assert parser.parse_args(BASE + ["--cells", "--neighbors", "1"]).neighbors == 1
    assert parser.parse_args(BASE + ["--cells", "--neighbors", "32"]).neighbors == 32
    action, = [a for a in parser._actions if "--neighbors" in a.option_strings]
    assert action.help.startswith("[extension]")


def test_cli_neighbors_without_cells_is_refused_with_a_message(capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + ["--neighbors"])
    assert exit_.value.code == 2 and "--neighbors" in capsys.readouterr().err


@pytest.mark.parametrize("bad", ["0", "33", "-1"])
def test_cli_neighbors_outside_the_range_is_refused(bad, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + ["--cells", "--neighbors", bad])
    assert exit_.value.code == 2 and "--neighbors" in capsys.readouterr().err


# ---- declarations -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    build = (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()
    assert "neighbors.hip" in build and (ROOT / "microbeseg_amd" / "csrc" / "neighbors.hip").is_file()
    source = (ROOT / "microbeseg_amd" / "csrc" / "neighbors.hip").read_text()
    for name in ("mseg_cell_neighbors", "mseg_cell_neighbors_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
        decl = re.search(rf"\b{name}\(([^;]*?)\);", header, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert re.search(rf'extern "C" \w+ {name}\(', source), name
