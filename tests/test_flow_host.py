"""CPU: linking under a tile-wise displacement field — the pick rule, the identities of the numpy
restatement tests/flow_ref.py, the stack that shows what the field is for (the GPU tests run the same stack on the device),
arguments, columns and the declarations."""
import functools
import pathlib
import re

import numpy as np
import pytest

import cells_ref as ref
import drift_ref as dref
import flow_ref as fref

ROOT = pathlib.Path(__file__).resolve().parents[1]

# the expanding colony of the GPU tests: 192 x 256, 4 frames, 40 rods, 8 % linear expansion per frame and three stage jumps
# of up to 6 px per axis; drift searched at R = 12, the field at r = 8 in 64 px tiles
FIX_SHAPE, FIX_T, FIX_CELLS, FIX_GROWTH = (192, 256), 4, 40, 0.08
FIX_OFFSETS = [(-1, -5), (6, 6), (0, -3)]
FIX_SEED = 5
FIX_R, FIX_FLOW, FIX_TILE = 12, 8, 64


@functools.lru_cache(maxsize=None)
def fixture_stack():
    """-> (labels uint16 [4, 192, 256], label_off, global shifts, tile scores, field); computed once, read only"""
    lab = fref.expanding_stack(*FIX_SHAPE, FIX_T, FIX_CELLS, FIX_GROWTH, FIX_OFFSETS, FIX_SEED)
    off = ref.frame_tables(lab)
    shift = dref.pick(dref.scores(lab, off, FIX_R))
    sc = fref.scores(lab, off, shift, FIX_FLOW, FIX_TILE)
    field = fref.pick(sc, shift)
    for a in (lab, off, shift, sc, field):
        a.setflags(write=False)
    return lab, off, shift, sc, field


def right_predecessors(lab, off, pred):
    """-> (cells present in frames t - 1 and t, over all pairs; those of them whose pred is their own id)"""
    n_both = right = 0
    for t in range(1, lab.shape[0]):
        for c in sorted((set(np.unique(lab[t])) & set(np.unique(lab[t - 1]))) - {0}):
            n_both += 1
            right += int(pred[int(off[t]) + c - 1] == c)
    return n_both, right


# ---- pick -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 3])
def test_pick_flow_equals_the_restatement_on_random_surfaces(r):
    from microbeseg_amd.inference import cells
    rng = np.random.default_rng(r)
    sc = rng.integers(0, 4, (5, 3, 4, 2 * r + 1, 2 * r + 1)).astype(np.uint32)       # few distinct values: ties everywhere
    sc[1, 2] = 0                                                                    # a row of empty tiles
    sc[3] = 0                                                                       # an empty pair
    base = rng.integers(-200, 200, (6, 2)).astype(np.int32)
    got, want = cells.pick_flow(sc, base), fref.pick(sc, base)
    assert got.dtype == np.int32 and got.shape == (6, 3, 4, 2) and np.array_equal(got, want)
    assert not got[0].any()
    assert np.array_equal(got[2, 2], np.broadcast_to(base[2], (4, 2)))             # empty tiles fall back to the base
    assert np.array_equal(got[4], np.broadcast_to(base[4], (3, 4, 2)))
    assert np.abs(got[1:] - base[1:, None, None]).max() <= r


def test_pick_flow_rule():
    from microbeseg_amd.inference import cells
    for fn in (cells.pick_flow, fref.pick):
        sc = np.zeros((1, 1, 2, 7, 7), np.uint32)
        sc[0, 0, 0, 3 + 1, 3 + 2] = sc[0, 0, 0, 3 - 1, 3 + 2] = sc[0, 0, 0, 3 + 2, 3 - 1] = sc[0, 0, 0, 3 - 2, 3 + 1] = 5
        sc[0, 0, 1, 3, 3] = sc[0, 0, 1, 3 + 1, 3] = 7                                # a deviation that ties (0, 0) never wins
        out = fn(sc, np.array([(9, 9), (10, -20)], np.int32))
        assert out[1].tolist() == [[[10 - 2, -20 + 1], [10, -20]]]                  # equal norm: the smaller ey first
        assert fn(np.zeros((0, 2, 2, 3, 3), np.uint32), np.zeros((1, 2), np.int32)).shape == (1, 2, 2, 2)    # one frame
    with pytest.raises(ValueError, match="scores"):
        cells.pick_flow(np.zeros((1, 2, 2, 3, 4), np.uint32), np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match="base"):
        cells.pick_flow(np.zeros((1, 2, 2, 3, 3), np.uint32), np.zeros((3, 2), np.int32))


# ---- identities of the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [64, 128])
def test_tile_surfaces_sum_to_the_drift_surface(tile):
    H, W, T, r, R = 70, 131, 3, 3, 12                    # neither size is a multiple of the tile
    lab = fref.expanding_stack(H, W, T, 12, 0.05, [(2, -3), (-1, 4)], 2)
    off = ref.frame_tables(lab)
    whole = dref.scores(lab, off, R)
    base = np.array([(100, 100), (2, -3), (-9, 7)], np.int32)        # row 0 is not read; |base| + r <= R
    sc = fref.scores(lab, off, base, r, tile)
    assert sc.shape == (T - 1,) + fref.tiles(H, W, tile) + (2 * r + 1, 2 * r + 1) and sc.any()
    for t in range(1, T):
        by, bx = (int(v) for v in base[t])
        want = whole[t - 1, by - r + R:by + r + R + 1, bx - r + R:bx + r + R + 1]
        assert np.array_equal(sc[t - 1].sum(axis=(0, 1), dtype=np.int64), want)


def test_links_under_a_constant_field_are_the_shifted_links():
    lab, off, shift, _, _ = fixture_stack()
    ty, tx = fref.tiles(*FIX_SHAPE, FIX_TILE)
    const = np.broadcast_to(shift[:, None, None, :], (FIX_T, ty, tx, 2))
    for a, b in zip(fref.links_field(lab, off, const, FIX_TILE), dref.links_shifted(lab, off, shift)):
        assert np.array_equal(a, b)
    far = np.full((FIX_T, ty, tx, 2), 1000, np.int32)
    assert not fref.links_field(lab, off, far, FIX_TILE)[0].any()


# ---- the test that shows the feature --------------------------------------------------------------------------------------------
def test_the_field_links_an_expanding_colony_that_one_shift_per_pair_cannot():
    """40 rods expand by 8 % per frame about the centre of a 192 x 256 frame, under stage jumps of up to 6 px.  On the
    restatement alone: of the 117 cells present in both frames of a pair, plain overlap linking finds the right predecessor
    for 32, linking under the global shift of the pair (R = 12) for 48 (41 %), linking under the field picked from the 64 px
    tile surfaces at r = 8 for 116 (99 %)."""
    lab, off, shift, sc, field = fixture_stack()
    assert lab.shape == (FIX_T,) + FIX_SHAPE and int(lab.max()) == FIX_CELLS
    assert sc.shape == (FIX_T - 1, 3, 4, 2 * FIX_FLOW + 1, 2 * FIX_FLOW + 1)
    n_both, right_plain = right_predecessors(lab, off, ref.links(lab, off)[0])
    _, right_global = right_predecessors(lab, off, dref.links_shifted(lab, off, shift)[0])
    _, right_field = right_predecessors(lab, off, fref.links_field(lab, off, field, FIX_TILE)[0])
    print(f"{n_both} cells present in both frames of a pair: right predecessor for {right_plain} (plain), {right_global} "
          f"(global shift), {right_field} (field)")
    assert n_both > 100
    assert right_global < 0.80 * n_both
    assert right_field >= 0.95 * n_both
    assert (n_both, right_plain, right_global, right_field) == (117, 32, 48, 116)       # the docstring's counts
    # the field differs from tile to tile and stays within r of the global shift
    assert len({tuple(v) for v in field[1].reshape(-1, 2).tolist()}) > 4
    assert np.abs(field[1:] - shift[1:, None, None]).max() <= FIX_FLOW


def test_flow_columns_hold_the_field_value_of_the_centroid_tile():
    from microbeseg_amd.inference import cells
    lab, off, shift, _, field = fixture_stack()
    raw = ref.measure(lab, off)
    links = fref.links_field(lab, off, field, FIX_TILE)
    df = cells.table_from_sums(off, *FIX_SHAPE, raw, links=links, shift=shift, field=field, tile=FIX_TILE)
    assert list(df.columns) == cells.columns([], link=True, drift=True, flow=True)
    t = df["frame"].to_numpy()
    j = np.floor(df["centroid_y"].to_numpy()).astype(int) // FIX_TILE
    i = np.floor(df["centroid_x"].to_numpy()).astype(int) // FIX_TILE
    want = np.where((t > 0)[:, None], np.asarray(field)[t, j, i], 0)
    assert df["flow_y"].dtype.kind == "i" and df["flow_x"].dtype.kind == "i"
    assert np.array_equal(df[["flow_y", "flow_x"]].to_numpy(), want) and want.any()
    # every other column is the one of the table without the field
    plain = cells.table_from_sums(off, *FIX_SHAPE, raw, links=links, shift=shift)
    assert plain.equals(df[list(plain.columns)])
    with pytest.raises(ValueError, match="shift"):
        cells.table_from_sums(off, *FIX_SHAPE, raw, links=links, field=field, tile=FIX_TILE)


# ---- arguments and columns ---------------------------------------------------------------------------------------------------------
def test_flow_arguments_are_checked_before_the_device_is_touched():
    from microbeseg_amd.inference import cells
    lab = np.zeros((2, 4, 4), np.uint16)
    with pytest.raises(ValueError, match="drift"):
        cells.measure_cells(lab, flow=8)
    for bad in (-1, 33, 2.5, "3", True):
        with pytest.raises((ValueError, TypeError)):
            cells.measure_cells(lab, drift=4, flow=bad)
    for bad in (32, 100, 0, 64.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            cells.measure_cells(lab, drift=4, flow=8, flow_tile=bad)
    assert cells.check_flow(None) == (None, 64) and cells.check_flow(0, 128) == (0, 128)
    assert cells.check_flow(np.int64(32), np.int64(256)) == (32, 256)
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.flow is None and InferWorker.flow_tile == 64


def test_flow_columns():
    from microbeseg_amd.inference import cells
    assert cells.columns([1], link=True, drift=True, flow=True) == cells.columns([1], link=True) + \
        ["drift_y", "drift_x", "centroid_y_reg", "centroid_x_reg", "flow_y", "flow_x"]
    full = cells.columns([0], True, True, True, True, (50,), True, True, flow=True)
    assert full.index("flow_x") + 1 == full.index("perimeter") and full.index("flow_y") == full.index("centroid_x_reg") + 1
    assert [c for c in full if c not in ("flow_y", "flow_x")] == cells.columns([0], True, True, True, True, (50,), True, True)
    with pytest.raises(ValueError, match="drift"):
        cells.columns([], link=True, flow=True)


# ---- declarations ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    names = ("mseg_stack_flow", "mseg_stack_flow_workspace_bytes", "mseg_cell_links_field")
    for name in names:
        assert name in _lib.SIGNATURES, name
        decl = re.search(rf"\b{name}\(([^;]*?)\);", header, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    source = (ROOT / "microbeseg_amd" / "csrc" / "drift.hip").read_text() + \
        (ROOT / "microbeseg_amd" / "csrc" / "cells.hip").read_text()
    for name in names:
        assert re.search(rf'extern "C" \w+ {name}\(', source), name
