"""TEST INFRASTRUCTURE ONLY — structured worst-case instance masks for the label creation (csrc/labels.hip,
label_boundary_kernel of csrc/augment.hip).  Pure numpy; every coordinate is written out.  Each builder returns
(name, mask uint16 (H, W), search_radius); frames are at most 64 x 64.

What each family is for (the decision point of the kernels that it puts on the line):
  half_even        centroids at exactly x.5 in y and x, both parities      rint() in lb_window_kernel
  frame_* / tromino_*  cells on every edge and in every corner             y0 / y1 / x0 / x1 clipped by the frame
  long_bar, split_* cells cut by / absent from their own window            the window test of lb_edt_kernel
  edge_<side>_<in|out>  the only neighbour on the last column / row of the window, or just past it
  partial_neighbour nearest pixel of the neighbour lies outside the window
  comb_same_rows / comb_rows_away / comb_transposed / comb_mirrored   >= 12 alternating runs between a pixel and the other cell   lb_gap_other, `lim`
  ties_345(_flipped)  other cells at (0,5) (3,4) (4,3) (5,0), and (1,5)+(3,4), (2,5)+(4,3): lb_isqrt_ceil at and off squares
  gap_g<g>_l<L>_t<T>  two facing rectangles: every area class of the artefact test, kept and removed; minor axis < and >= 3
  diagonal_gap(_mirrored)  a gap component that is one piece under 8-connectivity only, joined down-right / down-left
  ring_gap         an annular gap around an 8 x 8 cell
  near_<edge>      closable gaps 0, 1, 2, 3 pixels from the frame
  seven_ids        more than six ids in one disk(3); only the last one met closes the pixel    tried[6]
  tiny_*           H or W below 7, H == 1, W == 1
  ids_extreme      ids 1 and 65535, touching
  whole_window     contract only (no background pixel in the window): both maps are 0
"""
import numpy as np


def _frame(H, W):
    return np.zeros((H, W), np.uint16)


def _rect(m, y0, y1, x0, x1, k):
    """rows y0..y1-1, columns x0..x1-1"""
    assert 0 <= y0 < y1 <= m.shape[0] and 0 <= x0 < x1 <= m.shape[1], (y0, y1, x0, x1, m.shape)
    m[y0:y1, x0:x1] = k


# ---- 1a. centroid and frame ------------------------------------------------------------------------------------------------------
def half_even():
    """two-pixel-thick bars: the centroid is at .5 across the bar, and (even length) at .5 along it.  sr = 3 cuts every
    bar along its length, so moving the window by one pixel moves a column / row of the cell in or out of it."""
    m = _frame(40, 48)
    _rect(m, 4, 6, 3, 11, 1)       # cy 4.5 -> 4   cx 6.5 -> 6
    _rect(m, 5, 7, 20, 28, 2)      # cy 5.5 -> 6   cx 23.5 -> 24
    _rect(m, 14, 24, 4, 6, 3)      # cy 18.5 -> 18 cx 4.5 -> 4
    _rect(m, 15, 25, 15, 17, 4)    # cy 19.5 -> 20 cx 15.5 -> 16
    _rect(m, 11, 13, 30, 42, 5)    # cy 11.5 -> 12 cx 35.5 -> 36
    _rect(m, 32, 34, 22, 34, 6)    # cy 32.5 -> 32 cx 27.5 -> 28
    return "half_even", m, 3


def _frame_blocks():
    m = _frame(24, 28)
    _rect(m, 0, 4, 0, 4, 1)
    _rect(m, 0, 4, 24, 28, 2)
    _rect(m, 20, 24, 0, 4, 3)
    _rect(m, 20, 24, 24, 28, 4)
    _rect(m, 0, 4, 10, 14, 5)      # touching pair on the top edge
    _rect(m, 0, 4, 14, 18, 6)
    _rect(m, 20, 24, 9, 14, 7)     # bottom edge, a two-pixel gap
    _rect(m, 20, 24, 16, 20, 8)
    _rect(m, 8, 12, 0, 3, 9)       # touching pair on the left edge
    _rect(m, 12, 16, 0, 3, 10)
    _rect(m, 9, 15, 25, 28, 11)    # right edge
    _rect(m, 9, 14, 11, 16, 12)    # centre
    return m


def frame_whole():
    return "frame_whole", _frame_blocks(), 100     # sr larger than the frame: every window is the frame


def frame_sr3():
    return "frame_sr3", _frame_blocks(), 3


def _trominoes():
    """L-trominoes: three pixels, so a window of 2 x 2 (sr = 1) still holds a pixel that is not the cell"""
    m = _frame(12, 14)
    cells = (((0, 1), (1, 0), (1, 1)), ((0, 12), (1, 12), (1, 13)), ((10, 1), (11, 0), (11, 1)), ((11, 13), (10, 13), (11, 12)),
             ((0, 6), (1, 6), (0, 7)), ((11, 6), (10, 6), (11, 7)), ((5, 0), (6, 0), (5, 1)), ((5, 13), (6, 13), (5, 12)),
             ((5, 6), (6, 6), (5, 7)),
             ((0, 8), (1, 8), (1, 9)))             # touches the top-edge tromino
    for k, px in enumerate(cells, 1):              # corners (without the corner pixel itself where sr = 1 would see nothing else)
        for y, x in px:
            m[y, x] = k
    return m


def tromino_sr1():
    return "tromino_sr1", _trominoes(), 1


def tromino_sr2():
    return "tromino_sr2", _trominoes(), 2


# ---- 1b. search window -----------------------------------------------------------------------------------------------------------
def long_bar():
    """a bar of 22 columns with sr = 4 (window of 8), a neighbour bar two rows below it"""
    m = _frame(20, 32)
    _rect(m, 6, 9, 4, 26, 1)
    _rect(m, 11, 13, 2, 30, 2)
    return "long_bar", m, 4


def split_empty_window():
    """cell 1 in two equal pieces 20 columns apart: its window lies between them and holds none of its pixels"""
    m = _frame(16, 40)
    _rect(m, 5, 8, 4, 7, 1)
    _rect(m, 5, 8, 30, 33, 1)
    _rect(m, 5, 9, 16, 21, 2)      # another cell sits where the window of cell 1 is
    return "split_empty_window", m, 4


def split_partial_window():
    """cell 1 in a large and a small piece: the window holds a part of the large piece only"""
    m = _frame(16, 40)
    _rect(m, 4, 8, 4, 14, 1)       # 40 pixels, columns 4..13
    _rect(m, 4, 6, 30, 32, 1)      # 4 pixels
    _rect(m, 10, 12, 8, 16, 2)
    return "split_partial_window", m, 4


def window_edge(side, inside):
    """cell 1 = 5 x 5 around (12, 12), sr = 6: window rows / columns [6, 18).  The only other cell is a one-pixel-wide bar on
    the first / last row / column of the window (inside) or one step past it."""
    m = _frame(24, 24)
    _rect(m, 10, 15, 10, 15, 1)
    pos = {"x1": 17 if inside else 18, "x0": 6 if inside else 5, "y1": 17 if inside else 18, "y0": 6 if inside else 5}[side]
    if side[0] == "x":
        _rect(m, 9, 16, pos, pos + 1, 2)
    else:
        _rect(m, pos, pos + 1, 9, 16, 2)
    return f"edge_{side}_{'in' if inside else 'out'}", m, 6


def partial_neighbour():
    """cell 1 = 5 x 5 around (12, 12), sr = 4: window [8, 16).  Cell 2 is an L: its column 16 (just outside) is the nearest part
    for the right half of cell 1, its arm on row 8 (the first window row) is what the window sees."""
    m = _frame(24, 24)
    _rect(m, 10, 15, 10, 15, 1)
    _rect(m, 8, 15, 16, 17, 2)
    _rect(m, 8, 9, 13, 17, 2)
    return "partial_neighbour", m, 4


COMB_PROBES = ((49, 24), (50, 24), (51, 24))


def _comb(m):
    """cell 1 = a 48 x 48 block with 14 teeth below it: rows 49..51 read 1,0,1,0,... from column 10 to 36.  The block makes the
    cell's largest distance 24, so the denominator of the neighbour map is 27 and a neighbour distance of 14 (the probes:
    13 runs away from the other cell) stays above the cut of the rescaling: 1 - 14 / 27 = 0.48 > 0.39."""
    _rect(m, 1, 49, 1, 49, 1)
    for x in range(10, 37, 2):
        _rect(m, 49, 52, x, x + 1, 1)


def comb_same_rows():
    """the other cell stands in the tooth rows behind the last tooth: found at dy = 0 across 13 runs, and the tooth rows at
    dy = 1, 2 are then walked under the bound `lim`"""
    m = _frame(64, 64)
    _comb(m)
    _rect(m, 49, 52, 38, 41, 2)
    return "comb_same_rows", m, 40


def comb_rows_away():
    """the other cell stands below the teeth: the tooth rows are walked to the window's end without a find, and the answer
    comes from a row with dy > 0"""
    m = _frame(64, 64)
    _comb(m)
    _rect(m, 54, 56, 38, 41, 2)
    return "comb_rows_away", m, 40


def comb_transposed():
    """comb_rows_away transposed: the teeth are crossed by the row sweep (dy), not by the run walk"""
    return "comb_transposed", np.ascontiguousarray(comb_rows_away()[1].T), 40


TIES_PROBES = ((12, 12), (12, 34), (34, 12), (34, 34))


def ties_345():
    """11 x 11 cells whose corner pixel p (TIES_PROBES) has single-pixel cells at p + (0,5), (3,4), (4,3), (5,0): four ways
    to 25; at p + (1,5) and (3,4): 26 is found first, 25 needs g = 4 under lim = ceil(sqrt(17)) = 5;
    at p + (2,5) and (4,3): 29 first, 25 needs g = 3 under lim = ceil(sqrt(13)) = 4.  The cells are large enough (largest
    cell distance 6, so the denominator is 9) for p to stay above the cut of the rescaling: 1 - 5 / 9 = 0.44 > 0.39."""
    m = _frame(44, 44)
    k = 10
    for n, ((py, px), offs) in enumerate(zip(TIES_PROBES, (((0, 5), (3, 4), (4, 3), (5, 0)),
                                                           ((1, 5), (3, 4)),
                                                           ((2, 5), (4, 3)),
                                                           ((5, 0), (4, 3), (0, 5))))):
        _rect(m, py - 10, py + 1, px - 10, px + 1, n + 1)
        for dy, dx in offs:
            m[py + dy, px + dx] = k
            k += 1
    return "ties_345", m, 12


def ties_345_flipped():
    """ties_345 turned by 180 degrees: the other cells lie to the left and above, so the left-hand walk and the rows above
    meet the same bounds"""
    return "ties_345_flipped", np.ascontiguousarray(ties_345()[1][::-1, ::-1]), 12


def comb_mirrored():
    """comb_same_rows flipped left to right: the 13 runs are crossed by the left-hand walk"""
    return "comb_mirrored", np.ascontiguousarray(comb_same_rows()[1][:, ::-1]), 40


# ---- 1c. gaps and the per-cell closing -------------------------------------------------------------------------------------------
def gap_pair(g, L, T):
    """two rectangles of length L and thickness T, g background rows between them"""
    m = _frame(2 * T + g + 10, L + 10)
    _rect(m, 5, 5 + T, 5, 5 + L, 1)
    _rect(m, 5 + T + g, 5 + 2 * T + g, 5, 5 + L, 2)
    return f"gap_g{g}_l{L}_t{T}", m, 20


# (g, L, T): chosen so that every area class (<= 20, <= 30, <= 50, > 50) is met with a kept and with a removed gap and the
# minor axis lies on both sides of 3 — asserted by tests/test_labels_structured_host.py
GAP_PAIRS = ((1, 8, 3), (2, 4, 2), (2, 12, 2), (3, 8, 6),                  # area <= 20 (2, 12, 2: exactly 20)
             (2, 14, 3), (2, 14, 2), (2, 17, 2), (4, 8, 6),                 # area <= 30 (2, 17, 2: exactly 30)
             (2, 22, 2), (3, 14, 6), (3, 14, 8), (2, 27, 2),                # area <= 50 (2, 27, 2: exactly 50)
             (2, 30, 3), (2, 30, 2), (3, 30, 8), (6, 14, 3))                # area > 50


def diagonal_gap():
    """six rectangles in 24 x 32; their gaps form a component whose parts touch only diagonally"""
    m = _frame(24, 32)
    for k, (y0, y1, x0, x1) in enumerate(DIAGONAL_RECTS, 1):
        _rect(m, y0, y1, x0, x1, k)
    return "diagonal_gap", m, 12


def diagonal_gap_mirrored():
    """the same frame flipped left to right: the diagonal join runs the other way"""
    return "diagonal_gap_mirrored", np.ascontiguousarray(diagonal_gap()[1][:, ::-1]), 12


# found once by a seeded search over random six-rectangle frames (numpy default_rng(5), 42nd draw); stored, not searched
DIAGONAL_RECTS = ((10, 17, 17, 24), (1, 8, 18, 23), (8, 14, 8, 12), (9, 12, 1, 7), (1, 5, 4, 10), (20, 24, 26, 30))


def ring_gap():
    """an 8 x 8 cell inside an annular cell, 3 background pixels between them: one gap that surrounds the inner cell"""
    m = _frame(30, 30)
    _rect(m, 4, 26, 4, 26, 2)
    _rect(m, 8, 22, 8, 22, 0)
    _rect(m, 11, 19, 11, 19, 1)
    return "ring_gap", m, 14


def near_frame(edge):
    """pairs of cells 5 wide and 6 high, one background column between them, 0, 1, 2 and 3 rows from the top of the frame, and
    one pair further in; the other edges by flipping / transposing.  The facing sides are long enough for the gap to be kept
    (rim sum 8 >= 5), so it shows in the neighbour map exactly where the closing lets it live."""
    m = _frame(20, 64)
    k = 1
    for d, x in ((0, 1), (1, 18), (2, 35), (3, 52)):
        _rect(m, d, d + 6, x, x + 5, k)
        _rect(m, d, d + 6, x + 6, x + 11, k + 1)
        k += 2
    _rect(m, 12, 18, 8, 13, k)
    _rect(m, 12, 18, 14, 19, k + 1)
    m = {"top": m, "bottom": m[::-1], "left": m.T, "right": m.T[:, ::-1]}[edge]
    return f"near_{edge}", np.ascontiguousarray(m), 8


def seven_ids():
    """background pixel p = (12, 12).  Eight single-pixel cells above it inside disk(3) come first in raster order and close
    nothing; the ninth id met, at p + (0, -3), is a U whose arms (columns 9 and 15) close p."""
    m = _frame(26, 25)
    _rect(m, 5, 18, 9, 10, 9)
    _rect(m, 5, 18, 15, 16, 9)
    _rect(m, 16, 18, 9, 16, 9)
    for k, (dy, dx) in enumerate(((-3, 0), (-2, -2), (-2, 0), (-2, 2), (-1, -2), (-1, -1), (-1, 1), (-1, 2)), 1):
        m[12 + dy, 12 + dx] = k
    return "seven_ids", m, 10


# ---- 1d. frames, ids, whole-window cell ------------------------------------------------------------------------------------------
def tiny(H, W):
    m = _frame(H, W)
    sr = 2
    if (H, W) == (1, 9):
        m[0] = [0, 1, 1, 0, 2, 2, 3, 0, 4]
    elif (H, W) == (9, 1):
        m[:, 0] = [0, 1, 1, 0, 2, 2, 3, 0, 4]
    elif (H, W) == (3, 3):
        m[:] = [[1, 1, 0], [0, 2, 2], [3, 0, 2]]
    elif (H, W) == (6, 20):
        _rect(m, 0, 3, 0, 4, 1)
        _rect(m, 1, 5, 6, 9, 2)
        _rect(m, 1, 5, 9, 12, 3)
        _rect(m, 3, 6, 15, 20, 4)
        sr = 3
    elif (H, W) == (7, 7):
        _rect(m, 0, 7, 0, 3, 1)
        _rect(m, 0, 7, 4, 7, 2)
        m[3, 3] = 3                                # the only pixel 3 away from every edge
        sr = 3
    else:
        assert (H, W) == (1, 1)                    # one background pixel, no cell
    return f"tiny_{H}x{W}", m, sr


def ids_extreme():
    m = _frame(16, 20)
    _rect(m, 4, 10, 3, 9, 1)
    _rect(m, 4, 10, 9, 15, 65535)
    _rect(m, 12, 14, 5, 13, 2)
    return "ids_extreme", m, 6


def whole_window():
    """CONTRACT ONLY (not compared with the oracle): no pixel of the window lies outside the cell"""
    return "whole_window", np.full((16, 16), 1, np.uint16), 4


def small_shapes():
    """single pixels, two-pixel cells and a diagonal line, for the moment formulas (a single pixel has major axis 0)"""
    m = _frame(16, 24)
    m[2, 2] = 1
    m[2, 20] = 2
    m[13, 3] = 3
    m[6, 5] = m[6, 6] = 4
    m[9, 12] = m[10, 12] = 5
    m[12, 17] = m[13, 18] = 6
    for i in range(9):
        m[3 + i, 8 + i] = 7
    return "small_shapes", m, 5


def all_cases():
    """every fixture that is compared with the oracle, in a fixed order"""
    out = [half_even(), frame_whole(), frame_sr3(), tromino_sr1(), tromino_sr2(), long_bar(), split_empty_window(),
           split_partial_window()]
    for side in ("x1", "x0", "y1", "y0"):
        out += [window_edge(side, True), window_edge(side, False)]
    out += [partial_neighbour(), comb_same_rows(), comb_rows_away(), comb_transposed(), comb_mirrored(), ties_345(),
            ties_345_flipped()]
    out += [gap_pair(*p) for p in GAP_PAIRS]
    out += [diagonal_gap(), diagonal_gap_mirrored(), ring_gap()]
    out += [near_frame(e) for e in ("top", "bottom", "left", "right")]
    out += [seven_ids()]
    out += [tiny(*s) for s in ((1, 1), (1, 9), (9, 1), (3, 3), (6, 20), (7, 7))]
    out += [ids_extreme(), small_shapes()]
    for _, m, _ in out:
        m.setflags(write=False)
    return out


CASES = {name: (mask, sr) for name, mask, sr in all_cases()}
