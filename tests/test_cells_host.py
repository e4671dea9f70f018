"""CPU: the numpy restatement of the per-cell table (tests/cells_ref.py) against scikit-image's own regionprops values
(tests/golden/cells_regionprops.npz, tools/gen_golden_cells.py), the track assembly on hand-made link tables, the new
command-line flags and the declaration of the new entry points."""
import pathlib
import re
import sys

import numpy as np
import pandas as pd
import pytest

import cells_ref as ref

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "cells_regionprops.npz"
CASES = ["ellipses", "touching", "small", "border"]
MAX_SKIPPED = 0.10        # share of a case's cells whose orientation may be undefined


def load_case(name):
    z = np.load(GOLDEN)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}


def check_against_library(df, g, skip):
    """df: one row per cell in label order (columns of measure_cells, channel 0 measured); g: the library's values.
    Integers, centroid, mean, min and max bit-equal; axes rtol 1e-9 / atol 1e-6 px; orientation the same in radians
    except for the cells in ``skip`` (undefined angle), which may be at most 10 % of the case."""
    assert np.array_equal(df["label"].to_numpy(np.int64), g["ids"])
    assert np.array_equal(df["area"].to_numpy(np.int64), g["area"])
    assert np.array_equal(df["centroid_y"].to_numpy(np.float64), g["centroid"][:, 0])
    assert np.array_equal(df["centroid_x"].to_numpy(np.float64), g["centroid"][:, 1])
    bbox = df[["bbox_min_row", "bbox_min_col", "bbox_max_row", "bbox_max_col"]].to_numpy(np.int64)
    assert np.array_equal(bbox, g["bbox"])
    assert np.array_equal(df["mean_ch0"].to_numpy(np.float64), g["mean"])
    assert np.array_equal(df["min_ch0"].to_numpy(np.int64), g["min"])
    assert np.array_equal(df["max_ch0"].to_numpy(np.int64), g["max"])
    np.testing.assert_allclose(df["major_axis_length"].to_numpy(np.float64), g["major"], rtol=1e-9, atol=1e-6)
    np.testing.assert_allclose(df["minor_axis_length"].to_numpy(np.float64), g["minor"], rtol=1e-9, atol=1e-6)
    skip = np.asarray(skip, bool)
    assert skip.mean() <= MAX_SKIPPED, f"{skip.sum()} of {len(skip)} cells without a defined orientation"
    np.testing.assert_allclose(df["orientation"].to_numpy(np.float64)[~skip], g["orientation"][~skip], rtol=1e-9, atol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_regionprops(name):
    g = load_case(name)
    df = ref.table(g["label"][None], g["img"][None, None], channels=[0], link=False)
    check_against_library(df, g, df["_skip"])


def test_fixture_holds_the_stated_cases():
    small, border = load_case("small"), load_case("border")
    assert (small["area"] == 1).sum() >= 3 and (small["area"] == 4).sum() >= 1
    H, W = border["label"].shape
    bb = border["bbox"]
    assert ((bb[:, 0] == 0) | (bb[:, 1] == 0) | (bb[:, 2] == H) | (bb[:, 3] == W)).any()
    lab = load_case("touching")["label"].astype(np.int64)
    right = (lab[:, :-1] != lab[:, 1:]) & (lab[:, :-1] > 0) & (lab[:, 1:] > 0)
    assert right.any()
    assert GOLDEN.stat().st_size < 400 * 1024


# ---- assemble_tracks ---------------------------------------------------------------------------------------------------
def _tracks(rows, min_overlap=1):
    from microbeseg_amd.inference.cells import assemble_tracks
    frame, label, pred, overlap = (np.array(c) for c in zip(*rows))
    got = assemble_tracks(frame, label, pred, overlap, min_overlap)
    want = ref.tracks(frame, label, pred, overlap, min_overlap)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got[0].tolist(), got[1].tolist()


def test_tracks_continuation_appearance_disappearance():
    #        frame label pred overlap
    rows = [(0, 1, 0, 0), (0, 2, 0, 0),
            (1, 1, 1, 9), (1, 3, 0, 0),          # 1 continues, 2 disappears, label 3 appears
            (2, 1, 1, 7), (2, 2, 3, 5)]
    track, parent = _tracks(rows)
    assert track == [1, 2, 1, 3, 1, 3] and parent == [0] * 6


def test_tracks_division_into_two_and_three():
    rows = [(0, 1, 0, 0), (0, 2, 0, 0),
            (1, 1, 1, 4), (1, 2, 1, 5), (1, 3, 2, 3), (1, 4, 2, 3), (1, 5, 2, 2),
            (2, 1, 2, 5)]                         # a daughter goes on: keeps its track and its parent
    track, parent = _tracks(rows)
    assert track == [1, 2, 3, 4, 5, 6, 7, 4]
    assert parent == [0, 0, 1, 1, 2, 2, 2, 1]


def test_tracks_merge_loser_ends():
    rows = [(0, 1, 0, 0), (0, 2, 0, 0),
            (1, 1, 1, 8),                         # cells 1 and 2 merged; the link names 1, so track 2 ends
            (2, 1, 1, 8)]
    track, parent = _tracks(rows)
    assert track == [1, 2, 1, 1] and parent == [0, 0, 0, 0]


def test_tracks_min_overlap_cut_and_id_order():
    rows = [(0, 2, 0, 0), (0, 5, 0, 0),           # ids follow first appearance, not the labels
            (1, 1, 5, 2), (1, 2, 2, 6)]
    assert _tracks(rows) == ([1, 2, 2, 1], [0, 0, 0, 0])
    track, parent = _tracks(rows, min_overlap=3)  # the 2-pixel link is cut: a new track instead of a continuation
    assert track == [1, 2, 3, 1] and parent == [0, 0, 0, 0]
    # a cut link no longer counts as a successor: the remaining daughter inherits instead of dividing
    rows = [(0, 1, 0, 0), (1, 1, 1, 9), (1, 2, 1, 1)]
    assert _tracks(rows) == ([1, 2, 3], [0, 1, 1])
    assert _tracks(rows, min_overlap=2) == ([1, 1, 2], [0, 0, 0])


def test_tracks_empty_table():
    from microbeseg_amd.inference.cells import assemble_tracks
    track, parent = assemble_tracks([], [], [], [], 1)
    assert len(track) == 0 and len(parent) == 0


# ---- command line, table layout, declarations ------------------------------------------------------------------------------
def _script():
    sys.path.insert(0, str(ROOT))
    import infer_script_local
    return infer_script_local


def test_cli_accepts_the_new_flags():
    script = _script()
    args = script.build_parser().parse_args(["-i", "x", "-m", "y", "--cells", "--measure_channels", "0", "2",
                                             "--min_overlap", "5"])
    assert args.cells and args.measure_channels == [0, 2] and args.min_overlap == 5
    args = script.build_parser().parse_args(["-i", "x", "-m", "y", "-c", "1"])
    assert not args.cells and args.measure_channels is None and args.min_overlap == 1
    help_text = script.build_parser().format_help()
    assert "no motion model" in " ".join(help_text.split()) and "no gap closing" in " ".join(help_text.split())
    assert script.measured_channels(args, np.zeros((2, 3, 4, 5))) == [1]
    assert script.measured_channels(args, np.zeros((7, 4, 5))) == [0]


def test_select_channels_views_and_missing_channel():
    script = _script()
    rng = np.random.default_rng(0)
    tchw = rng.integers(0, 65536, (4, 5, 6, 7)).astype(np.uint16)
    hwc = rng.integers(0, 256, (6, 7, 3)).astype(np.uint8)
    chw = rng.integers(0, 256, (3, 6, 7)).astype(np.uint8)
    thw = rng.integers(0, 256, (4, 6, 7)).astype(np.uint8)
    for img, chans in ((tchw, [1]), (tchw, [0, 2, 4]), (tchw, [1, 2]), (hwc, [2]), (hwc, [0, 1, 2]), (chw, [1]),
                       (thw, [0]), (thw[0], [0])):
        view = script.select_channels(img, chans, "a.tif")
        assert np.shares_memory(view, img), "a view, not a copy"
        for i, c in enumerate(chans):
            want = script.select_frames(img, c, "a.tif")
            assert np.array_equal(view[:, i], want)
    for img, chans in ((tchw, [5]), (hwc, [3]), (chw, [0, 3]), (thw, [1]), (tchw, [-1])):
        with pytest.raises(ValueError, match="channel"):
            script.select_channels(img, chans, "a.tif")
    assert script.select_channels(np.zeros((1, 1, 1, 1, 1)), [0], "a.tif") is None


def test_table_columns_in_the_stated_order(tmp_path):
    from microbeseg_amd.inference import cells
    want = ['frame', 'label', 'area', 'centroid_y', 'centroid_x', 'bbox_min_row', 'bbox_min_col', 'bbox_max_row',
            'bbox_max_col', 'major_axis_length', 'minor_axis_length', 'orientation', 'touches_border',
            'mean_ch1', 'std_ch1', 'min_ch1', 'max_ch1', 'sum_ch1', 'bg_mean_ch1',
            'mean_ch3', 'std_ch3', 'min_ch3', 'max_ch3', 'sum_ch3', 'bg_mean_ch3',
            'pred_label', 'overlap', 'track_id', 'parent_track']
    assert cells.columns([1, 3], link=True) == want
    assert cells.columns([], link=False) == want[:13]
    # the host half of measure_cells on the integer sums of the restatement: same columns, written and read back
    g = load_case("small")
    lab, img = g["label"][None], g["img"][None, None]
    off = ref.frame_tables(lab)
    raw = ref.measure(lab, off, img)
    pred, ovl = ref.links(lab, off)
    df = cells.table_from_sums(off, lab.shape[1], lab.shape[2], raw, channels=[0], links=(pred, ovl))
    assert list(df.columns) == cells.columns([0], link=True)
    check_against_library(df, g, ref.table(lab, link=False)["_skip"])
    cells.write_cells(df, tmp_path / "cells.csv")
    back = pd.read_csv(tmp_path / "cells.csv", float_precision="round_trip")
    assert list(back.columns) == list(df.columns) and len(back) == len(df)
    for col in df.columns:
        assert np.array_equal(back[col].to_numpy(), df[col].to_numpy(), equal_nan=df[col].dtype.kind == "f"), col


def test_new_symbols_declared_and_bound():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    for name in ("mseg_cell_measure", "mseg_cell_links", "mseg_cell_links_workspace_bytes"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES
    build = (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()
    assert "cells.hip" in build and (ROOT / "microbeseg_amd" / "csrc" / "cells.hip").is_file()
    # argument counts of the declarations and the ctypes table agree
    for name in ("mseg_cell_measure", "mseg_cell_links", "mseg_cell_links_workspace_bytes"):
        decl = re.search(rf"\b{name}\(([^;]*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
