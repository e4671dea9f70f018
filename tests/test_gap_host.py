"""CPU: gap closing in cell tracks — tracks over gaps, the composed motion, the numpy restatement
tests/gap_ref.py on the stacks the GPU tests run on the device, arguments, columns and the declarations."""
import functools
import pathlib
import re

import numpy as np
import pytest

import cells_ref as ref
import gap_ref as gref

ROOT = pathlib.Path(__file__).resolve().parents[1]

# the base stack of the GPU tests: T = 6, 48 x 64, three rectangles
BASE_T, BASE_SHAPE = 6, (48, 64)


@functools.lru_cache(maxsize=None)
def base_stack():
    """A (label 1): 8 x 14 at row 4, column 6 + t, absent in frame 2; B (label 2): a steady neighbour; C (label 3): absent
    in frames 2 and 3.  -> uint16 [6, 48, 64], read only"""
    lab = np.zeros((BASE_T,) + BASE_SHAPE, np.uint16)
    for t in range(BASE_T):
        if t != 2:
            lab[t, 4:12, 6 + t:20 + t] = 1
        lab[t, 20:30, 30:44] = 2
        if t not in (2, 3):
            lab[t, 36:44, 8:24] = 3
    lab.setflags(write=False)
    return lab


def moved_stack(lab, step, margin=0):
    """the stack on a larger canvas, frame t moved by t * step -> (uint16 stack, the per-pair shifts int32 [T, 2])"""
    T, H, W = lab.shape
    out = np.zeros((T, H + margin + (T - 1) * step[0], W + margin + (T - 1) * step[1]), np.uint16)
    for t in range(T):
        out[t, t * step[0]:t * step[0] + H, t * step[1]:t * step[1] + W] = lab[t]
    shift = np.tile(np.array(step, np.int32), (T, 1))
    shift[0] = 0
    return out, shift


def division_stack():
    """T = 4, 40 x 64, rows 8 .. 15 and 28 .. 33 (no cell is square: every orientation is defined).  E (columns 10 .. 29) and
    F (columns 26 .. 33, lower row) exist in frames 0 and 1 only.  M (lower row) covers columns 34 .. 49 in frames 0 and 1
    and shrinks to columns 42 .. 49 in frames 2 and 3: it continues.  Frame 3 has three new cells: P (columns 10 .. 18) and Q (columns 21 .. 29) over E, and R (lower row, columns
    30 .. 41), which lies on 8 columns of M as it was in frame 1, on 4 columns of F, and on nothing in frame 2."""
    lab = np.zeros((4, 40, 64), np.uint16)
    for t in (0, 1):
        lab[t, 8:16, 10:30] = 1          # E
        lab[t, 28:34, 26:34] = 2         # F
        lab[t, 28:34, 34:50] = 3         # M
    lab[2, 28:34, 42:50] = 1             # M
    lab[3, 8:16, 10:19] = 1              # P
    lab[3, 8:16, 21:30] = 2              # Q
    lab[3, 28:34, 30:42] = 3             # R
    lab[3, 28:34, 42:50] = 4             # M
    lab.setflags(write=False)
    return lab


def check_division_table(none, one):
    """what the division stack's tables hold without gap closing and with gap = 1"""
    at = lambda df, t, l: df[(df["frame"] == t) & (df["label"] == l)].iloc[0]
    assert none["track_id"].nunique() == 6 and one["track_id"].nunique() == 5
    for label in (1, 2, 3):
        assert at(none, 3, label)["pred_label"] == 0 and at(none, 3, label)["parent_track"] == 0
    e_track, f_track, m_track = (at(one, 0, l)["track_id"] for l in (1, 2, 3))
    for label in (1, 2):                                              # P and Q: both on E, a division across the gap
        row = at(one, 3, label)
        assert (row["pred_label"], row["pred_gap"], row["overlap"], row["parent_track"]) == (1, 2, 8 * 9, e_track)
    assert len({at(one, 3, 1)["track_id"], at(one, 3, 2)["track_id"], e_track, f_track, m_track}) == 5
    row = at(one, 3, 3)                                               # R: mostly on M, which continued; F ended and gets it
    assert (row["pred_label"], row["pred_gap"], row["overlap"], row["track_id"], row["parent_track"]) == (2, 2, 6 * 4, f_track, 0)
    row = at(one, 3, 4)
    assert (row["pred_label"], row["pred_gap"], row["track_id"]) == (1, 1, m_track)


# ---- tracks ---------------------------------------------------------------------------------------------------------------------
TRACK_CASES = {
    # frame, label, pred, overlap, gap
    "plain chain": ([0, 1, 2], [1, 1, 1], [0, 1, 1], [0, 9, 9], [0, 1, 1]),
    "one gap": ([0, 0, 1, 2, 2], [1, 2, 2, 1, 2], [0, 0, 2, 1, 2], [0, 0, 5, 7, 5], [0, 0, 1, 2, 1]),
    "division across a gap": ([0, 2, 2], [1, 1, 2], [0, 1, 1], [0, 4, 6], [0, 2, 2]),
    "named at gap 1 and gap 2 by different cells": ([0, 1, 2], [1, 1, 1], [0, 1, 1], [0, 8, 3], [0, 1, 2]),
    "gap 3 and a dropped link": ([0, 1, 3, 3], [1, 1, 1, 2], [0, 1, 1, 1], [0, 1, 9, 9], [0, 1, 3, 2]),
    "the named cell does not exist": ([0, 2], [1, 1], [0, 2], [0, 5], [0, 2]),
}


@pytest.mark.parametrize("name", sorted(TRACK_CASES))
def test_assemble_tracks_over_gaps_equals_the_restatement(name):
    from microbeseg_amd.inference import cells
    frame, label, pred, overlap, gap = TRACK_CASES[name]
    for min_overlap in (1, 2):
        got = cells.assemble_tracks(frame, label, pred, overlap, min_overlap, gap)
        want = gref.tracks(frame, label, pred, overlap, min_overlap, gap)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, min_overlap)
        # without gaps: today's result, which cells_ref.tracks states
        got = cells.assemble_tracks(frame, label, pred, overlap, min_overlap)
        same = cells.assemble_tracks(frame, label, pred, overlap, min_overlap, gap=None)
        ones = cells.assemble_tracks(frame, label, pred, overlap, min_overlap, gap=np.ones(len(frame), np.int64))
        want = ref.tracks(frame, label, pred, overlap, min_overlap)
        for other in (same, ones, want, gref.tracks(frame, label, pred, overlap, min_overlap)):
            assert np.array_equal(got[0], other[0]) and np.array_equal(got[1], other[1]), (name, min_overlap)


def test_assemble_tracks_rules_over_gaps():
    from microbeseg_amd.inference import cells
    frame, label, pred, overlap, gap = TRACK_CASES["division across a gap"]
    track, parent = cells.assemble_tracks(frame, label, pred, overlap, 1, gap)
    assert track.tolist() == [1, 2, 3] and parent.tolist() == [0, 1, 1]
    frame, label, pred, overlap, gap = TRACK_CASES["named at gap 1 and gap 2 by different cells"]
    track, parent = cells.assemble_tracks(frame, label, pred, overlap, 1, gap)
    assert track.tolist() == [1, 2, 3] and parent.tolist() == [0, 1, 1]           # two successors: a division
    frame, label, pred, overlap, gap = TRACK_CASES["one gap"]
    track, parent = cells.assemble_tracks(frame, label, pred, overlap, 1, gap)
    assert track.tolist() == [1, 2, 2, 1, 2] and parent.tolist() == [0] * 5      # one successor hands on, whatever the gap


# ---- composed motion ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 2, 3, 5, 9])
def test_compose_motion_equals_the_restatement(g):
    from microbeseg_amd.inference import cells
    rng = np.random.default_rng(g)
    for shape in ((7, 2), (7, 2, 3, 2), (1, 2), (2, 1, 1, 2)):
        moved = rng.integers(-40, 41, shape).astype(np.int32)
        got, want = cells.compose_motion(moved, g), gref.compose(moved, g)
        assert got.dtype == np.int32 and got.shape == moved.shape and np.array_equal(got, want), (shape, g)
        assert not got[:g].any()
    shift = np.array([(99, 99), (1, 2), (3, 4), (5, 6)], np.int32)               # row 0 is never part of a sum
    assert cells.compose_motion(shift, 2).tolist() == [[0, 0], [0, 0], [4, 6], [8, 10]]
    assert cells.compose_motion(shift, 3).tolist() == [[0, 0], [0, 0], [0, 0], [9, 12]]
    assert np.array_equal(cells.compose_motion(shift, 1)[1:], shift[1:])
    with pytest.raises(ValueError):
        cells.compose_motion(np.zeros((4, 3), np.int32), 2)


# ---- the restatement on the stacks of the GPU tests ------------------------------------------------------------------------------------
def test_base_stack_on_the_restatement():
    """5 tracks without gap closing, 4 with gap = 1 (A is joined over frame 2), 3 with gap = 2 (C over frames 2 and 3)"""
    lab = base_stack()
    none = gref.table(lab)
    one = gref.table(lab, gap=1)
    two = gref.table(lab, gap=2)
    assert "pred_gap" not in none.columns and none.drop(columns="_skip").equals(ref.table(lab).drop(columns="_skip"))
    assert [df["track_id"].nunique() for df in (none, one, two)] == [5, 4, 3]
    at = lambda df, t, l: df[(df["frame"] == t) & (df["label"] == l)].iloc[0]
    assert at(one, 3, 1)["pred_gap"] == 2 and at(one, 3, 1)["pred_label"] == 1 and at(one, 3, 1)["overlap"] == 8 * 12
    assert at(one, 4, 3)["pred_gap"] == 0 and at(two, 4, 3)["pred_gap"] == 3 and at(two, 4, 3)["overlap"] == 8 * 16
    assert at(two, 3, 1)["pred_gap"] == 2
    assert sorted(one["pred_gap"].unique()) == [0, 1, 2] and sorted(two["pred_gap"].unique()) == [0, 1, 2, 3]
    assert at(two, 5, 1)["track_id"] == at(two, 0, 1)["track_id"] and at(two, 5, 3)["track_id"] == at(two, 0, 3)["track_id"]
    assert not two["parent_track"].any()


def test_division_stack_on_the_restatement():
    lab = division_stack()
    check_division_table(gref.table(lab), gref.table(lab, gap=1))
    # R's largest partner two frames back is M: with every cell flagged the plain rule takes it
    off = ref.frame_tables(lab)
    everyone = np.ones(int(off[-1]), bool)
    pred, ovl = gref.links_gap(lab, off, 2, everyone, everyone)
    assert pred[int(off[3]) + 2] == 3 and ovl[int(off[3]) + 2] == 6 * 8


def test_moved_base_stack_needs_the_composed_shift():
    """the base stack moved by (5, 6) px per frame: two steps are (10, 12), beyond the 8 px cell height, so gap closing at the
    same (y, x) joins nothing, and under the composed shift the tracks are those of the unmoved stack"""
    lab, shift = moved_stack(base_stack(), (5, 6))
    still = gref.table(base_stack(), gap=2)
    plain = gref.table(lab, gap=2)
    moved = gref.table(lab, gap=2, shift=shift)
    assert plain["pred_gap"].max() <= 1 or plain["track_id"].nunique() > 3
    for col in ("track_id", "parent_track", "pred_gap", "pred_label", "overlap"):
        assert np.array_equal(moved[col].to_numpy(), still[col].to_numpy()), col


# ---- arguments and columns -------------------------------------------------------------------------------------------------------------
def test_gap_arguments_are_checked_before_the_device_is_touched():
    from microbeseg_amd.inference import cells
    from microbeseg_amd.inference.infer import InferWorker
    assert cells.MAX_GAP == 4 and cells.check_gap(None) is None
    for ok in (1, 2, 3, 4, np.int64(4), np.int32(1)):
        assert cells.check_gap(ok) == int(ok) and type(cells.check_gap(ok)) is int
    for bad in (0, 5, -1, True, False, 1.0, 1.5, "2", b"2", (1,), [2]):
        with pytest.raises(ValueError, match="gap"):
            cells.check_gap(bad)
    lab = np.zeros((2, 4, 4), np.uint16)
    with pytest.raises(ValueError, match="link"):
        cells.measure_cells(lab, gap=1, link=False)
    for bad in (0, 5, 1.5, "1", True):
        with pytest.raises(ValueError, match="gap"):
            cells.measure_cells(lab, gap=bad)
    assert InferWorker.gap is None


def test_gap_columns():
    from microbeseg_amd.inference import cells
    link = cells.columns([1], link=True)
    assert cells.columns([1], link=True, gap=True) == link + ["pred_gap"]
    assert cells.columns([1], link=True, drift=True, gap=True) == cells.columns([1], link=True, drift=True) + ["pred_gap"]
    assert cells.columns([1], link=True, drift=True, flow=True, gap=True) == \
        cells.columns([1], link=True, drift=True, flow=True) + ["pred_gap"]
    for drift, flow, before in ((False, False, "parent_track"), (True, False, "centroid_x_reg"), (True, True, "flow_x")):
        plain = cells.columns([0], True, drift, True, True, (50,), True, True, flow)
        full = cells.columns([0], True, drift, True, True, (50,), True, True, flow, gap=True)
        assert full.index("pred_gap") == full.index(before) + 1 and full.index("pred_gap") + 1 == full.index("perimeter")
        assert [c for c in full if c != "pred_gap"] == plain
        assert cells.columns([0], True, drift, True, True, (50,), True, True, flow, gap=False) == plain
    with pytest.raises(ValueError, match="link"):
        cells.columns([], link=False, gap=True)


def test_table_from_sums_with_gaps():
    from microbeseg_amd.inference import cells
    lab = base_stack()
    off = ref.frame_tables(lab)
    raw = ref.measure(lab, off)
    pred, ovl, pred_gap = gref.close_gaps(lab, off, *ref.links(lab, off), 1, 2)
    df = cells.table_from_sums(off, *BASE_SHAPE, raw, links=(pred, ovl), gaps=pred_gap)
    want = gref.table(lab, gap=2)
    assert list(df.columns) == cells.columns([], link=True, gap=True)
    for col in ("frame", "label", "area", "pred_label", "overlap", "pred_gap", "track_id", "parent_track"):
        assert np.array_equal(df[col].to_numpy(), want[col].to_numpy()), col
    assert df["pred_gap"].dtype.kind == "i"
    plain = cells.table_from_sums(off, *BASE_SHAPE, raw, links=ref.links(lab, off))
    assert "pred_gap" not in plain.columns and plain["track_id"].nunique() == 5 and df["track_id"].nunique() == 3
    same = [c for c in plain.columns if c not in ("pred_label", "overlap", "track_id", "parent_track")]
    assert plain[same].equals(df[same])


# ---- declarations ------------------------------------------------------------------------------------------------------------------
def test_new_symbol_declared_and_bound():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    name = "mseg_cell_links_gap"
    assert name in _lib.SIGNATURES
    decl = re.search(rf"\b{name}\(([^;]*?)\);", header, re.S)
    assert decl
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == 19
    source = (ROOT / "microbeseg_amd" / "csrc" / "cells.hip").read_text()
    assert re.search(rf'extern "C" \w+ {name}\(', source)
