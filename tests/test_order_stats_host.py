"""CPU: per-cell percentiles — the restatement tests/order_stats_ref.py against np.percentile, the rank and
value formulas of inference/cells.py, the percentile rule, the columns, the --percentiles flag, table_from_sums on hand-made
integers, and the declarations."""
import math
import pathlib
import re
import sys

import numpy as np
import pytest

import cells_ref as ref
import order_stats_ref as oref

ROOT = pathlib.Path(__file__).resolve().parents[1]
PS = (0, 1, 5, 25, 50, 75, 95, 99, 100)


def random_samples():
    """sorted samples of 1 .. 400 values: uint8, uint16, and a narrow uint16 range that straddles 255 / 256"""
    rng = np.random.default_rng(5)
    for i in range(300):
        n = int(rng.integers(1, 401)) if i % 7 else (1, 2, 3, 399, 400)[i % 5]
        kind = i % 3
        if kind == 0:
            v = rng.integers(0, 256, n).astype(np.uint8)
        elif kind == 1:
            v = rng.integers(0, 65536, n).astype(np.uint16)
        else:
            v = rng.integers(250, 262, n).astype(np.uint16)
        yield np.sort(v)


# ---- the restatement against numpy -------------------------------------------------------------------------------------------
def test_restatement_against_numpy_percentile():
    # values <= 65535 and three fp64 operations: rounding differences stay below 1e-10; 1e-9 leaves room for another numpy
    worst = 0.0
    for v in random_samples():
        for P in PS:
            got, want = oref.percentile(v, P), float(np.percentile(v, P))
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-9, (len(v), v.dtype, P, got, want)
    print(f"largest difference to np.percentile: {worst:.3e}")


def test_package_formulas_against_numpy_and_the_restatement():
    from microbeseg_amd.inference import cells
    for v in random_samples():
        ranks, g = cells.percentile_ranks(len(v), PS)
        assert ranks.shape == (2 * len(PS),) and g.shape == (len(PS),) and ranks.dtype == np.int64
        got = cells.percentile_value(v[ranks[0::2]], v[ranks[1::2]], g)
        for i, P in enumerate(PS):
            k, k1, gg = oref.percentile_ranks(len(v), P)
            assert (int(ranks[2 * i]), int(ranks[2 * i + 1]), float(g[i])) == (k, k1, gg)
            assert float(got[i]) == oref.percentile(v, P)
            assert abs(float(got[i]) - float(np.percentile(v, P))) <= 1e-9


def test_odd_count_median_is_the_middle_integer():
    rng = np.random.default_rng(6)
    for n in (1, 3, 5, 7, 99, 399):
        v = np.sort(rng.integers(0, 65536, n).astype(np.uint16))
        assert oref.percentile(v, 50) == float(v[n // 2])
        k, k1, g = oref.percentile_ranks(n, 50)
        assert (k, g) == (n // 2, 0.0)


# ---- percentile_ranks ---------------------------------------------------------------------------------------------------------
def test_percentile_ranks():
    from microbeseg_amd.inference import cells
    counts = np.array([0, 1, 2, 3, 4, 10, 101, 400, 2 ** 22, 2 ** 31 - 600], np.int64)
    ps = tuple(range(0, 101, 5))[:8] + (100,)
    for chunk in (ps[:8], (99, 100, 1, 50)):
        ranks, g = cells.percentile_ranks(counts, chunk)
        assert ranks.shape == (2 * len(chunk), len(counts)) and g.shape == (len(chunk), len(counts))
        top = np.maximum(counts - 1, 0)
        assert (ranks >= 0).all() and (ranks <= top).all() and (g >= 0).all() and (g < 1).all()
        assert (ranks[:, 0] == 0).all() and (ranks[:, 1] == 0).all() and (g[:, :2] == 0).all()      # counts 0 and 1
        for i, P in enumerate(chunk):
            assert (ranks[2 * i] <= ranks[2 * i + 1]).all() and (ranks[2 * i + 1] - ranks[2 * i] <= 1).all()
            if P == 0:
                assert (ranks[2 * i] == 0).all() and (g[i] == 0).all()
            if P == 100:
                assert (ranks[2 * i] == top).all() and (ranks[2 * i + 1] == top).all() and (g[i] == 0).all()
    for P in PS:
        r, g = cells.percentile_ranks(1, (P,))
        assert r.tolist() == [0, 0] and g.tolist() == [0.0]
    v = np.arange(10, 20)
    r, g = cells.percentile_ranks(10, (0, 100))
    assert v[r].tolist() == [10, 11, 19, 19]
    assert cells.percentile_value(v[r[0::2]], v[r[1::2]], g).tolist() == [10.0, 19.0]


def test_percentile_value_rule():
    from microbeseg_amd.inference import cells
    assert float(cells.percentile_value(10, 20, 0.25)) == 12.5
    assert float(cells.percentile_value(10, 20, 0.75)) == 17.5
    assert float(cells.percentile_value(0, 65535, 0.5)) == 65535 - 65535 * 0.5
    assert float(cells.percentile_value(7, 7, 0.3)) == 7.0


# ---- check_percentiles --------------------------------------------------------------------------------------------------------
def test_check_percentiles():
    from microbeseg_amd.inference.cells import check_percentiles
    assert check_percentiles(None) == () and check_percentiles(()) == () and check_percentiles([]) == ()
    assert check_percentiles((5, 50, 95)) == (5, 50, 95)
    assert check_percentiles([95, 5]) == (95, 5)                                   # the order given
    assert check_percentiles([0, 100]) == (0, 100)
    assert check_percentiles(np.array([50])) == (50,) and type(check_percentiles(np.array([50]))[0]) is int
    assert check_percentiles((50.0,)) == (50,)
    assert check_percentiles(range(8)) == tuple(range(8))
    for bad in ((101,), (-1,), (50, 50), tuple(range(9)), (2.5,), (True,), ("50",), 50, "50", (None,), (float("nan"),)):
        with pytest.raises(ValueError):
            check_percentiles(bad)


# ---- columns --------------------------------------------------------------------------------------------------------------------
SHAPE = ['frame', 'label', 'area', 'centroid_y', 'centroid_x', 'bbox_min_row', 'bbox_min_col', 'bbox_max_row', 'bbox_max_col',
         'major_axis_length', 'minor_axis_length', 'orientation', 'touches_border']
LINK = ['pred_label', 'overlap', 'track_id', 'parent_track']
MIDLINE = ['skeleton_pixels', 'skeleton_length', 'skeleton_ends', 'skeleton_branches', 'midline_length', 'midline_width',
           'midline_y0', 'midline_x0', 'midline_y1', 'midline_x1']


def _ch(c):
    return [f'mean_ch{c}', f'std_ch{c}', f'min_ch{c}', f'max_ch{c}', f'sum_ch{c}', f'bg_mean_ch{c}']


def test_columns():
    from microbeseg_amd.inference import cells
    assert cells.columns([0, 2], True, percentiles=(95, 5)) == SHAPE + _ch(0) + _ch(2) + LINK + [
        'p95_ch0', 'p5_ch0', 'p95_ch2', 'p5_ch2', 'bg_p95_ch0', 'bg_p5_ch0', 'bg_p95_ch2', 'bg_p5_ch2']
    assert cells.columns([1], False, False, False, True, (50,)) == SHAPE + _ch(1) + MIDLINE + ['p50_ch1', 'bg_p50_ch1']
    # without percentiles: the present lists
    assert cells.columns([0, 2], True) == SHAPE + _ch(0) + _ch(2) + LINK
    assert cells.columns([1], False, False, False, True) == SHAPE + _ch(1) + MIDLINE
    assert cells.columns([1], False, False, False, True, ()) == SHAPE + _ch(1) + MIDLINE
    assert cells.columns() == SHAPE + LINK
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.percentiles is None


# ---- command line -----------------------------------------------------------------------------------------------------------------
BASE = ["-i", "x", "-m", "y"]


def _parser():
    sys.path.insert(0, str(ROOT))
    import infer_script_local as script
    return script.build_parser()


def test_cli_percentiles():
    parser = _parser()
    assert parser.parse_args(BASE).percentiles is None and parser.parse_args(BASE + ["--cells"]).percentiles is None
    assert parser.parse_args(BASE + ["--cells", "--percentiles"]).percentiles == [50]
    assert parser.parse_args(BASE + ["--cells", "--percentiles", "5", "50", "95"]).percentiles == [5, 50, 95]
    ns = parser.parse_args(BASE + ["--percentiles", "95", "5", "--cells", "--hull"])
    assert ns.percentiles == [95, 5] and ns.hull is True and ns.midline is False
    action, = [a for a in parser._actions if "--percentiles" in a.option_strings]
    assert action.help.startswith("[extension]")


@pytest.mark.parametrize("extra", [["--percentiles"], ["--percentiles", "50"],
                                   ["--cells", "--percentiles", "101"], ["--cells", "--percentiles", "-1"],
                                   ["--cells", "--percentiles", "5", "5"],
                                   ["--cells", "--percentiles"] + [str(v) for v in range(9)],
                                   ["--cells", "--percentiles", "2.5"]])
def test_cli_percentiles_refused_with_a_message(extra, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + extra)
    assert exit_.value.code == 2 and "--percentiles" in capsys.readouterr().err


# ---- table_from_sums on hand-made integers ----------------------------------------------------------------------------------------
def test_table_from_sums_with_order_stats():
    from microbeseg_amd.inference import cells
    # T = 2, 4 x 6.  Frame 0: cell 1 = 4 pixels, cell 2 = 5 pixels, 15 background pixels; frame 1: one cell covering the
    # whole frame: no background
    lab = np.zeros((2, 4, 6), np.int64)
    lab[0, 0, 0:4] = 1
    lab[0, 2, 0:5] = 2
    lab[1] = 1
    img = np.zeros((2, 1, 4, 6), np.uint16)
    img[0, 0, 0, 0:4] = [10, 40, 20, 30]
    img[0, 0, 2, 0:5] = [500, 100, 300, 200, 400]
    img[0, 0][lab[0] == 0] = np.arange(15) * 2
    img[1, 0] = np.arange(24).reshape(4, 6) * 1000
    off = ref.frame_tables(lab)
    assert off.tolist() == [0, 2, 3]
    raw = ref.measure(lab, off, img)
    pct = (50, 25, 100)
    # the ranks by hand: n = 4: h = 1.5, 0.75, 3; n = 5: h = 2, 1, 4; n = 24: h = 11.5, 5.75, 23; background n = 15: 7, 3.5, 14
    ranks = np.array([[1, 2, 11], [2, 3, 12], [0, 1, 5], [1, 2, 6], [3, 4, 23], [3, 4, 23]], np.int64)
    bg_ranks = np.array([[7, 0], [8, 0], [3, 0], [4, 0], [14, 0], [14, 0]], np.int64)
    got_ranks, _ = cells.percentile_ranks(raw["shape"][0].astype(np.int64), pct)
    assert np.array_equal(got_ranks, ranks)
    assert np.array_equal(cells.percentile_ranks(raw["bg_sums"][0, :, 0].astype(np.int64), pct)[0], bg_ranks)
    values, bg_values, status = oref.order_stats(lab, off, img, raw["bbox"], ranks, bg_ranks)
    assert status == 0
    assert values[:, 0, :].tolist() == [[20, 300, 11000], [30, 400, 12000], [10, 200, 5000], [20, 300, 6000],
                                        [40, 500, 23000], [40, 500, 23000]]
    assert bg_values[:, :, 0].tolist() == [[14, 0], [16, 0], [6, 0], [8, 0], [28, 0], [28, 0]]
    plain = cells.table_from_sums(off, 4, 6, raw, [0])
    df = cells.table_from_sums(off, 4, 6, raw, [0], order_stats=(pct, values, bg_values))
    assert list(df.columns) == list(plain.columns) + ['p50_ch0', 'p25_ch0', 'p100_ch0', 'bg_p50_ch0', 'bg_p25_ch0', 'bg_p100_ch0']
    assert df[list(plain.columns)].equals(plain)
    assert cells.table_from_sums(off, 4, 6, raw, [0], order_stats=None).equals(plain)
    assert df['p50_ch0'].tolist() == [25.0, 300.0, 11500.0]
    assert df['p25_ch0'].tolist() == [17.5, 200.0, 5750.0]
    assert df['p100_ch0'].tolist() == [40.0, 500.0, 23000.0]
    assert df['bg_p50_ch0'].tolist()[:2] == [14.0, 14.0] and math.isnan(df['bg_p50_ch0'][2])
    assert df['bg_p25_ch0'].tolist()[:2] == [7.0, 7.0] and math.isnan(df['bg_p25_ch0'][2])
    assert df['bg_p100_ch0'].tolist()[:2] == [28.0, 28.0] and math.isnan(df['bg_p100_ch0'][2])
    for c in df.columns[-6:]:
        assert df[c].dtype == np.float64, c
        want = oref.percentile_columns(lab, img, [0], pct)[c]
        assert np.array_equal(df[c].to_numpy(), np.array(want), equal_nan=True), c
    for c, P in (('p50_ch0', 50), ('p25_ch0', 25), ('p100_ch0', 100)):
        assert df[c].tolist() == [float(np.percentile(img[t, 0][lab[t] == l], P)) for t, l in ((0, 1), (0, 2), (1, 1))]
    with pytest.raises(ValueError):
        cells.table_from_sums(off, 4, 6, ref.measure(lab, off), [], order_stats=(pct, values, bg_values))


def test_restatement_rules():
    """absent cells, ids beyond the table, ranks out of range, pixels outside the given box"""
    lab = np.zeros((1, 5, 7), np.int32)
    lab[0, 1, 1:4] = 1
    lab[0, 3, 2:6] = 3                                            # id 2 is absent
    lab[0, 0, 0] = 9                                              # beyond the table of 3: neither cell nor background
    lab[0, 4, 6] = -4
    img = (np.arange(35).reshape(1, 1, 5, 7) + 100).astype(np.uint8)
    off = np.array([0, 3], np.int64)
    bbox = np.array([[1, 1, 2, 4], [0, 0, 0, 0], [3, 2, 4, 6]], np.int32)
    ranks = np.array([[0, 77, 3], [2, -5, 0]], np.int64)
    n_bg = 35 - 3 - 4 - 2
    values, bg_values, status = oref.order_stats(lab, off, img, bbox, ranks, np.array([[0], [n_bg - 1]]))
    assert status == 0 and values[:, 0].tolist() == [[108, 0, 126], [110, 0, 123]]
    assert bg_values[:, 0, 0].tolist() == [101, 133]              # 100 (the id 9) and 134 (the id -4) are not background
    assert oref.order_stats(lab, off, img, bbox, np.array([[3, 0, 0]]), np.array([[0]]))[2] == 1           # rank == area
    assert oref.order_stats(lab, off, img, bbox, np.array([[0, 0, 0]]), np.array([[n_bg]]))[2] == 1
    bbox[2] = [3, 2, 4, 5]                                        # one column short: 3 pixels found
    values, _, status = oref.order_stats(lab, off, img, bbox, np.array([[3, 0, 3]]), np.array([[0]]))
    assert status == 1 and values[0, 0].tolist() == [0, 0, 0]


# ---- declarations -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_bound_and_exported():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    build = (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()
    assert "order_stats.hip" in build and (ROOT / "microbeseg_amd" / "csrc" / "order_stats.hip").is_file()
    source = (ROOT / "microbeseg_amd" / "csrc" / "order_stats.hip").read_text()
    lib = _lib.load()
    for name in ("mseg_cell_order_stats", "mseg_cell_order_stats_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
        decl = re.search(rf"\b{name}\(([^;]*?)\);", header, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert re.search(rf'extern "C" \w+ {name}\(', source), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    # the size function is host code: O(T C R 256) words, nothing per cell, 0 for bad arguments
    size = lib.mseg_cell_order_stats_workspace_bytes
    assert size(4, 1000, 3, 16) == size(4, 0, 3, 16) == size(4, 10 ** 9, 3, 16) >= 4 * 4 * 3 * (256 + 16 * 256)
    assert size(4, 10, 3, 16) < 2 * 4 * 4 * 3 * (256 + 16 * 256 + 64)
    for bad in ((0, 10, 1, 1), (-1, 10, 1, 1), (1, -1, 1, 1), (1, 10, 0, 1), (1, 10, 1, 0), (1, 10, 1, 17)):
        assert size(*bad) == 0, bad
