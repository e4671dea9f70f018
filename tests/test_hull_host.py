"""CPU: per-cell outline measures — the two restatements of tests/hull_ref.py against each other and against
closed forms, the columns and their formulas, the --hull flag and the declarations."""
import functools
import math
import pathlib
import re
import sys

import numpy as np
import pytest

import cells_ref as ref
import hull_ref as href

ROOT = pathlib.Path(__file__).resolve().parents[1]
HULL_COLUMNS = ["perimeter", "convex_area", "solidity", "feret_max", "feret_min", "feret_angle", "feret_y0", "feret_x0",
                "feret_y1", "feret_x1"]


def random_cells(H, W, T=1, seed=0, speckle=0.15):
    """random rectangles, then ``speckle`` of the pixels redrawn among background and the frame's ids: ragged, disconnected
    and holed cells -> int64 labels [T, H, W]"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    lab = np.zeros((T, H, W), np.int64)
    for t in range(T):
        K = max(1, H * W // 40)
        for k in range(1, K + 1):
            y, x = rng.integers(0, H), rng.integers(0, W)
            lab[t, y:y + rng.integers(1, 7), x:x + rng.integers(1, 10)] = k
        flip = rng.random((H, W)) < speckle
        lab[t][flip] = rng.integers(0, K + 1, int(flip.sum()))
    return lab


def components(mask, diagonal):
    """connected components of a small boolean mask by flood fill -> list of pixel sets"""
    todo, parts = {(int(y), int(x)) for y, x in np.argwhere(mask)}, []
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if diagonal else [])
    while todo:
        stack, part = [todo.pop()], set()
        while stack:
            p = stack.pop()
            part.add(p)
            for dy, dx in steps:
                q = (p[0] + dy, p[1] + dx)
                if q in todo:
                    todo.remove(q)
                    stack.append(q)
        parts.append(part)
    return parts


def is_disconnected(mask):
    """the union of closed pixel squares falls apart (pixels that share only a corner still touch)"""
    return len(components(mask, diagonal=True)) > 1


def has_hole(mask):
    """some piece of the complement does not reach the outside"""
    outside = np.pad(~mask, 1, constant_values=True)
    return len(components(outside, diagonal=False)) > 1


def spherocylinder(length, width, tilt, H=48, W=48):
    """pixels whose centre lies within width / 2 of a segment of length - width through the frame's centre, ``tilt`` radians
    from the row axis -> uint16 [1, H, W]"""
    yy, xx = np.mgrid[0:H, 0:W] + 0.5
    dy, dx = yy - H / 2, xx - W / 2
    along = np.clip(dy * math.cos(tilt) + dx * math.sin(tilt), -(length - width) / 2, (length - width) / 2)
    dist2 = (dy - along * math.cos(tilt)) ** 2 + (dx - along * math.sin(tilt)) ** 2
    return (dist2 <= (width / 2) ** 2).astype(np.uint16)[None]


# ---- the restatements -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_cells():
    """(frame, id) of > 150 random small cells on frames up to 12 x 14"""
    cells = []
    for seed in range(24):
        for H, W in ((12, 14), (9, 13), (7, 10), (12, 5)):
            frame = random_cells(H, W, seed=seed)[0]
            frame.setflags(write=False)
            cells += [(frame, int(l)) for l in np.unique(frame) if l > 0]
    return cells


def test_brute_and_andrew_agree_on_random_small_cells():
    cells = small_cells()
    assert len(cells) >= 150
    apart = holed = 0
    for frame, l in cells:
        a, b = href.brute(frame, l), href.andrew(frame, l)
        assert a == b, (frame.shape, l, a, b)
        mask = frame == l
        assert a[0] >= 4 and a[1] >= 4 and a[2] >= 2 * int(mask.sum()) and a[3] >= 2 and a[8] >= 1 and a[9] >= 1
        assert (a[4], a[5]) < (a[6], a[7]) and (a[6] - a[4]) ** 2 + (a[7] - a[5]) ** 2 == a[3]
        apart += is_disconnected(mask)
        holed += has_hole(mask)
    print(f"{len(cells)} cells: {apart} disconnected, {holed} with a hole")
    assert apart >= 5 and holed >= 5


def test_hull_skips_ids_outside_the_table_and_absent_ids():
    frame = np.zeros((1, 6, 9), np.int64)
    frame[0, 1:3, 1:4] = 1
    frame[0, 3:5, 5:8] = 3                      # id 2 is absent
    frame[0, 0, 8] = 7                          # beyond a table of 3
    frame[0, 5, 0] = -4
    out = href.hull(frame, np.array([0, 3], np.int64))
    assert out.shape == (10, 3) and out.dtype == np.int64 and not out[:, 1].any()
    assert out[:, 0].tolist() == [10, 4, 12, 13, 1, 1, 3, 4, 2, 1]
    assert out[:, 2].tolist() == [10, 4, 12, 13, 3, 5, 5, 8, 2, 1]
    assert href.hull(frame, np.array([0, 2], np.int64)).shape == (10, 2)


@pytest.mark.parametrize("fn", [href.brute, href.andrew])
def test_closed_forms(fn):
    for h, w, y0, x0 in [(1, 1, 0, 0), (1, 1, 4, 7), (3, 5, 2, 1), (5, 3, 0, 0), (4, 4, 1, 6), (1, 8, 3, 0), (6, 1, 0, 9)]:
        frame = np.zeros((8, 12), np.int64)
        frame[y0:y0 + h, x0:x0 + w] = 2
        assert fn(frame, 2) == [2 * (h + w), 4, 2 * h * w, h * h + w * w, y0, x0, y0 + h, x0 + w, min(h, w), 1]
        assert fn(frame, 1) == [0] * 10
    one = np.zeros((3, 3), np.int64)
    one[1, 1] = 1
    assert fn(one, 1) == [4, 4, 2, 2, 1, 1, 2, 2, 1, 1]
    for n in (2, 3, 9):
        line = np.zeros((n + 2, n + 3), np.int64)
        line[np.arange(n) + 1, np.arange(n) + 2] = 1
        got = fn(line, 1)
        assert got[:4] == [4 * n, 6, 4 * n - 2, 2 * n * n] and got[4:8] == [1, 2, n + 1, n + 2] and got[8:] == [2, 2]
    ring = np.zeros((7, 7), np.int64)
    ring[1:6, 1:6] = 1
    ring[2:5, 2:5] = 0                          # the perimeter counts the hole, the hull does not see it
    assert fn(ring, 1) == [20 + 12, 4, 50, 50, 1, 1, 6, 6, 5, 1]
    two = np.zeros((9, 6), np.int64)            # two blobs of one id, empty rows between them
    two[0:2, 0:2] = 1
    two[6:8, 3:5] = 1
    assert fn(two, 1)[:4] == [16, 6, 44, 64 + 25] and fn(two, 1)[4:8] == [0, 0, 8, 5]


# ---- columns ----------------------------------------------------------------------------------------------------------------------
def test_hull_columns():
    from microbeseg_amd.inference import cells
    assert cells.HULL_COLUMNS == HULL_COLUMNS
    for args in (([1], True, True), ([], False, False), ([0, 2], True, False)):
        assert cells.columns(*args, hull=True) == cells.columns(*args) + HULL_COLUMNS
        assert cells.columns(*args, True) == cells.columns(*args, hull=True)
    assert cells.columns() == cells.SHAPE_COLUMNS + cells.LINK_COLUMNS and "perimeter" not in cells.columns([1], True, True)
    assert cells.columns([1], True, True, False) == cells.columns([1], True, True)
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.hull is False


def test_float_columns_follow_the_formulas():
    from microbeseg_amd.inference import cells
    lab = random_cells(12, 14, T=3, seed=2)
    off = ref.frame_tables(lab)
    raw, ints = ref.measure(lab, off), href.hull(lab, off)
    plain = cells.table_from_sums(off, 12, 14, raw, links=ref.links(lab, off))
    df = cells.table_from_sums(off, 12, 14, raw, links=ref.links(lab, off), hull=ints)
    assert list(df.columns) == cells.columns([], True, False, True) and len(df) == len(plain) > 10
    assert df[list(plain.columns)].equals(plain)
    assert cells.table_from_sums(off, 12, 14, raw, hull=ints).columns.tolist() == cells.columns([], False, False, True)
    slots = [int(off[t]) + l - 1 for t, l in zip(df["frame"], df["label"])]
    for row, s in zip(df.itertuples(index=False), slots):
        per, _, area2, feret2, ay, ax, by, bx, num, den2 = (int(v) for v in ints[:, s])
        assert row.perimeter == per and row.convex_area == area2 / 2 and row.solidity == row.area / (area2 / 2)
        assert row.feret_max == math.sqrt(feret2) and row.feret_min == num / math.sqrt(den2)
        assert row.feret_angle == math.atan2(bx - ax, by - ay) and -math.pi / 2 < row.feret_angle <= math.pi / 2
        assert (row.feret_y0, row.feret_x0, row.feret_y1, row.feret_x1) == (ay, ax, by, bx)
        assert 0 < row.solidity <= 1 and row.feret_min <= row.feret_max
    assert df["perimeter"].dtype.kind == "i" and df["feret_y0"].dtype.kind == "i" and df["feret_max"].dtype.kind == "f"


@pytest.mark.parametrize("tilt", [0.5, -0.5, 1.2, -1.2])
def test_feret_angle_follows_the_orientation_of_a_tilted_rod(tilt):
    from microbeseg_amd.inference import cells
    lab = spherocylinder(30, 8, tilt)
    off = ref.frame_tables(lab)
    df = cells.table_from_sums(off, *lab.shape[1:], ref.measure(lab, off), hull=href.hull(lab, off))
    row = df.iloc[0]
    print(f"tilt {tilt}: orientation {row.orientation:.4f}, feret_angle {row.feret_angle:.4f}, major {row.major_axis_length:.2f}, "
          f"feret_max {row.feret_max:.2f}, minor {row.minor_axis_length:.2f}, feret_min {row.feret_min:.2f}")
    assert np.sign(row.feret_angle) == np.sign(row.orientation) == np.sign(tilt)
    assert abs(row.feret_angle - row.orientation) < 0.1
    assert 29 < row.feret_max < 32 and 7 < row.feret_min < 9.5


# ---- command line -----------------------------------------------------------------------------------------------------------------
BASE = ["-i", "x", "-m", "y"]


def _parser():
    sys.path.insert(0, str(ROOT))
    import infer_script_local as script
    return script.build_parser()


def test_cli_hull():
    parser = _parser()
    assert parser.parse_args(BASE).hull is False and parser.parse_args(BASE + ["--cells"]).hull is False
    assert parser.parse_args(BASE + ["--cells", "--hull"]).hull is True
    assert parser.parse_args(BASE + ["--hull", "--cells", "--drift", "8"]).hull is True
    action, = [a for a in parser._actions if "--hull" in a.option_strings]
    assert action.help.startswith("[extension]")


def test_cli_hull_without_cells_is_refused_with_a_message(capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + ["--hull"])
    assert exit_.value.code == 2 and "--hull" in capsys.readouterr().err


# ---- declarations -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    from microbeseg_amd import _lib
    header = (ROOT / "include" / "mseg_hip.h").read_text()
    build = (ROOT / "microbeseg_amd" / "csrc" / "build.sh").read_text()
    assert "hull.hip" in build and (ROOT / "microbeseg_amd" / "csrc" / "hull.hip").is_file()
    source = (ROOT / "microbeseg_amd" / "csrc" / "hull.hip").read_text()
    for name in ("mseg_cell_hull", "mseg_cell_hull_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
        decl = re.search(rf"\b{name}\(([^;]*?)\);", header, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert re.search(rf'extern "C" \w+ {name}\(', source), name
