"""CPU: drift-compensated linking — the pick rule, the identities of the numpy restatement
tests/drift_ref.py, the well-posedness of the stack the GPU tests use, tracks and columns under a shift, the --drift flag
and the declarations."""
import functools
import pathlib
import re
import sys

import numpy as np
import pytest

import cells_ref as ref
import drift_ref as dref

ROOT = pathlib.Path(__file__).resolve().parents[1]

# the stack of the GPU tests: 70 x 131, 4 frames, 60 canvas cells, three jumps of 9 - 12 px per axis, searched at R = 12
FIX_SHAPE, FIX_T, FIX_CELLS, FIX_R = (70, 131), 4, 60, 12
FIX_OFFSETS = [(9, -11), (-3, 12), (12, 12)]
FIX_SEED = 1


@functools.lru_cache(maxsize=None)
def fixture_stack():
    """-> (labels uint16 [4, 70, 131], label_off, reference scores at R = 12, reference shifts); computed once, read only"""
    lab, _ = dref.drifting_stack(FIX_SHAPE[0], FIX_SHAPE[1], FIX_T, FIX_CELLS, FIX_OFFSETS, FIX_SEED)
    off = ref.frame_tables(lab)
    sc = dref.scores(lab, off, FIX_R)
    for a in (lab, off, sc):
        a.setflags(write=False)
    return lab, off, sc, dref.pick(sc)


def in_both(lab, t):
    """canvas ids with at least one pixel in frame t - 1 and in frame t"""
    return sorted((set(np.unique(lab[t])) & set(np.unique(lab[t - 1]))) - {0})


def assert_one_track_per_stretch(df):
    """a canvas cell (= its label here) keeps one track_id over every unbroken stretch of frames it is in view, no two
    stretches share a track, and nothing divides; -> the number of stretches"""
    stretches = 0
    for c, rows in df.groupby("label"):
        frames, tracks = rows["frame"].to_numpy(), rows["track_id"].to_numpy()
        new_stretch = np.concatenate([[True], np.diff(frames) != 1])
        assert np.array_equal(np.concatenate([[True], np.diff(tracks) != 0]), new_stretch), c
        stretches += int(new_stretch.sum())
    assert df.groupby("track_id")["label"].nunique().max() == 1
    assert df["track_id"].nunique() == stretches and not df["parent_track"].any()
    return stretches


# ---- pick ---------------------------------------------------------------------------------------------------------------------
def _surface(R, entries):
    s = np.zeros((1, 2 * R + 1, 2 * R + 1), np.uint32)
    for (dy, dx), v in entries.items():
        s[0, dy + R, dx + R] = v
    return s


@pytest.mark.parametrize("pick", ["package", "restatement"])
def test_pick_rule(pick):
    from microbeseg_amd.inference import cells
    fn = cells.pick_drift if pick == "package" else dref.pick
    one = lambda R, entries: fn(_surface(R, entries))[1].tolist()
    assert one(3, {(2, -3): 9, (0, 0): 8, (-1, 1): 8}) == [2, -3]                  # a unique peak
    assert one(3, {(0, 0): 7, (1, 0): 7, (-3, -3): 7}) == [0, 0]                   # a shift that ties (0, 0) never wins
    assert one(3, {(1, 2): 5, (-1, 2): 5, (2, -1): 5, (2, 1): 5, (-1, -2): 5, (-2, 1): 5}) == [-2, 1]   # equal norm: dy first
    assert one(3, {(-1, 2): 5, (-1, -2): 5}) == [-1, -2]                           # ... then the smaller dx
    assert one(3, {(3, 3): 5, (0, 1): 5, (0, -1): 5, (1, 0): 5}) == [0, -1]        # the smallest norm before either
    assert one(3, {}) == [0, 0]                                                     # nothing overlaps anywhere
    assert one(0, {(0, 0): 4}) == [0, 0] and one(0, {}) == [0, 0]                  # R = 0
    out = fn(np.concatenate([_surface(2, {(1, 1): 3}), _surface(2, {}), _surface(2, {(-2, 0): 1})]))
    assert out.dtype == np.int32 and out.tolist() == [[0, 0], [1, 1], [0, 0], [-2, 0]]
    assert fn(np.zeros((0, 5, 5), np.uint32)).tolist() == [[0, 0]]                 # a single frame


def test_pick_equals_restatement_on_random_surfaces():
    from microbeseg_amd.inference import cells
    rng = np.random.default_rng(3)
    sc = rng.integers(0, 4, (40, 7, 7)).astype(np.uint32)        # few distinct values: ties everywhere
    sc[5] = 0
    assert np.array_equal(cells.pick_drift(sc), dref.pick(sc))


# ---- identities of the restatement ---------------------------------------------------------------------------------------------
def test_reference_identities():
    lab, off, sc, _ = fixture_stack()
    fg = dref.foreground(lab, off)
    for t in range(1, FIX_T):
        assert sc[t - 1, FIX_R, FIX_R] == np.count_nonzero(fg[t] & fg[t - 1])
    zero = np.zeros((FIX_T, 2), np.int32)
    for a, b in zip(dref.links_shifted(lab, off, zero), ref.links(lab, off)):
        assert np.array_equal(a, b)
    for wide in ((0, FIX_SHAPE[1]), (0, -FIX_SHAPE[1]), (FIX_SHAPE[0], 0), (5, 1000)):
        pred, ovl = dref.links_shifted(lab, off, np.array([wide] * FIX_T, np.int32))
        assert not pred.any() and not ovl.any()
    # ids beyond a frame's table are background for the scores
    low = np.array(off, np.int64)
    low[1:] -= np.arange(1, FIX_T + 1) * 3
    assert dref.foreground(lab, low).sum() < fg.sum()
    # scores by slicing = scores by moving the frame
    rng = np.random.default_rng(0)
    for dy, dx in rng.integers(-FIX_R, FIX_R + 1, (8, 2)):
        assert sc[0, dy + FIX_R, dx + FIX_R] == np.count_nonzero(fg[1] & dref.moved(fg[0], dy, dx))


# ---- the stack of the GPU tests is well posed ------------------------------------------------------------------------------------
def test_fixture_peaks_are_unique_and_plain_linking_fails_on_it():
    lab, off, sc, shift = fixture_stack()
    assert lab.shape == (FIX_T,) + FIX_SHAPE
    for t, (dy, dx) in enumerate(FIX_OFFSETS, start=1):
        surface = sc[t - 1].astype(np.int64)
        assert (surface == surface.max()).sum() == 1, "the peak is unique"
        assert np.unravel_index(surface.argmax(), surface.shape) == (dy + FIX_R, dx + FIX_R)
        runner_up = np.sort(surface.ravel())[-2]
        print(f"pair {t}: peak {surface.max()} at {(dy, dx)}, runner-up {runner_up}")
    assert shift.tolist() == [[0, 0]] + [list(o) for o in FIX_OFFSETS]
    plain, _ = ref.links(lab, off)
    moved, _ = dref.links_shifted(lab, off, shift)
    n_both = right_plain = right_moved = 0
    for t in range(1, FIX_T):
        for c in in_both(lab, t):
            n_both += 1
            right_plain += int(plain[int(off[t]) + c - 1] == c)
            right_moved += int(moved[int(off[t]) + c - 1] == c)
    print(f"{n_both} cells present in both frames of a pair: plain linking right for {right_plain}, shifted for {right_moved}")
    assert n_both > 60
    assert right_plain < 0.10 * n_both
    assert right_moved == n_both


def test_tracks_follow_the_canvas_cells_under_the_shift():
    from microbeseg_amd.inference import cells
    lab, off, _, shift = fixture_stack()
    raw = ref.measure(lab, off)
    df = cells.table_from_sums(off, *FIX_SHAPE, raw, links=dref.links_shifted(lab, off, shift), shift=shift)
    assert_one_track_per_stretch(df)
    broken = cells.table_from_sums(off, *FIX_SHAPE, raw, links=ref.links(lab, off))
    assert broken["track_id"].nunique() > 2 * df["track_id"].nunique()       # without the shift nearly every cell starts anew


# ---- columns ----------------------------------------------------------------------------------------------------------------------
def test_drift_columns():
    from microbeseg_amd.inference import cells
    assert cells.columns([1], link=True, drift=True) == cells.columns([1], link=True) + \
        ["drift_y", "drift_x", "centroid_y_reg", "centroid_x_reg"]
    assert cells.columns([1]) == cells.columns([1], True, False) and "drift_y" not in cells.columns([1])
    with pytest.raises(ValueError, match="link"):
        cells.columns([], link=False, drift=True)
    lab, off, _, shift = fixture_stack()
    raw = ref.measure(lab, off)
    links = dref.links_shifted(lab, off, shift)
    df = cells.table_from_sums(off, *FIX_SHAPE, raw, links=links, shift=shift)
    assert list(df.columns) == cells.columns([], link=True, drift=True)
    total = np.cumsum(np.array([(0, 0)] + FIX_OFFSETS), axis=0)
    frame = df["frame"].to_numpy()
    assert df["drift_y"].dtype.kind == "i" and df["drift_x"].dtype.kind == "i"
    assert np.array_equal(df["drift_y"].to_numpy(), total[frame, 0])
    assert np.array_equal(df["drift_x"].to_numpy(), total[frame, 1])
    assert np.array_equal(df["centroid_y_reg"].to_numpy(), df["centroid_y"].to_numpy() - total[frame, 0])
    assert np.array_equal(df["centroid_x_reg"].to_numpy(), df["centroid_x"].to_numpy() - total[frame, 1])
    # a cell that is whole in two frames keeps its registered centroid (up to the rounding of sum / n - shift)
    inner = df[~df["touches_border"]]
    spread = inner.groupby("label")[["centroid_y_reg", "centroid_x_reg"]].agg(lambda v: v.max() - v.min())
    assert len(spread) > 20 and float(spread.to_numpy().max()) < 1e-9
    # row 0 of the shifts is ignored; without shift the table is the one from before
    other = shift.copy()
    other[0] = (5, 5)
    assert cells.table_from_sums(off, *FIX_SHAPE, raw, links=links, shift=other).equals(df)
    plain = cells.table_from_sums(off, *FIX_SHAPE, raw, links=links)
    assert list(plain.columns) == cells.columns([], link=True) and plain.equals(df[list(plain.columns)])


def test_drift_argument_is_checked_before_the_device_is_touched():
    from microbeseg_amd.inference import cells
    lab = np.zeros((2, 4, 4), np.uint16)
    for bad in (-1, 129, 2.5, "3", True):
        with pytest.raises((ValueError, TypeError)):
            cells.measure_cells(lab, drift=bad)
    with pytest.raises(ValueError, match="link"):
        cells.measure_cells(lab, link=False, drift=4)
    assert cells.check_drift(None) is None and cells.check_drift(0) == 0 and cells.check_drift(np.int64(128)) == 128
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.drift is None


# ---- command line -------------------------------------------------------------------------------------------------------------------
BASE = ["-i", "x", "-m", "y"]


def _parser():
    sys.path.insert(0, str(ROOT))
    import infer_script_local as script
    return script.build_parser()


def test_cli_drift_values():
    parser = _parser()
    assert parser.parse_args(BASE).drift is None and parser.parse_args(BASE + ["--cells"]).drift is None
    assert parser.parse_args(BASE + ["--cells", "--drift"]).drift == 32
    assert parser.parse_args(BASE + ["--cells", "--drift", "8"]).drift == 8
    assert parser.parse_args(BASE + ["--drift", "0", "--cells"]).drift == 0
    assert parser.parse_args(BASE + ["--cells", "--drift", "128"]).drift == 128
    action, = [a for a in parser._actions if "--drift" in a.option_strings]
    assert action.help.startswith("[extension]") and action.nargs == "?" and action.const == 32 and action.type is int


@pytest.mark.parametrize("extra", [["--drift"], ["--drift", "8"], ["--cells", "--drift", "129"], ["--cells", "--drift", "-1"],
                                   ["--cells", "--drift", "1.5"]])
def test_cli_drift_is_refused_with_a_message(extra, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + extra)
    assert exit_.value.code == 2 and "--drift" in capsys.readouterr().err


# ---- declarations ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    build = (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()
    assert "drift.hip" in build and (ROOT / "microbeseg_amd" / "csrc" / "drift.hip").is_file()
    for name in ("mseg_stack_drift", "mseg_stack_drift_workspace_bytes", "mseg_cell_links_shifted"):
        assert name in _lib.SIGNATURES, name
        decl = re.search(rf"\b{name}\(([^;]*?)\);", header, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    source = (ROOT / "microbeseg_amd" / "csrc" / "drift.hip").read_text() + \
        (ROOT / "microbeseg_amd" / "csrc" / "cells.hip").read_text()
    for name in ("mseg_stack_drift", "mseg_stack_drift_workspace_bytes", "mseg_cell_links_shifted"):
        assert re.search(rf'extern "C" \w+ {name}\(', source), name
