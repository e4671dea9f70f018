"""CPU: the per-cell intensity profile on the host: the numpy restatement tests/profile_ref.py against
independent forms, and the host half of inference/cells.py: the rule of --profile, the integer direction, the summary columns
from hand-made integer tables, the column names, the command-line flag."""
import math

import numpy as np
import pytest

import profile_ref as pref
from microbeseg_amd.inference import cells

UNIT = 16384


def rectangle(H=9, W=21, r0=2, c0=3, h=5, w=13, seed=0):
    """one frame, one axis-aligned rectangle of label 1, a uint16 image of two channels"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((1, H, W), np.int64)
    lab[0, r0:r0 + h, c0:c0 + w] = 1
    img = rng.integers(0, 65536, (1, 2, H, W)).astype(np.uint16)
    return lab, np.array([0, 1], np.int64), img, np.array([[r0, c0, r0 + h, c0 + w]], np.int32)


# ---- the restatement against independent forms ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 4, 5, 13, 32])
def test_rectangle_along_the_columns_is_reduceat_over_column_sums(N):
    lab, off, img, bbox = rectangle()
    r0, c0, r1, c1 = (int(v) for v in bbox[0])
    w = c1 - c0
    count, sums, extent = pref.profile(lab, off, img, bbox, [[0, UNIT]], N)
    assert extent[:, 0].tolist() == [UNIT * c0, UNIT * (c1 - 1)]
    # q - qmin = 16384 k, qmax - qmin + 1 = 16384 (w - 1) + 1: a hair below k N / (w - 1), so ceil(k N / (w - 1)) - 1 for k > 0
    col_bin = [0] + [(k * N - 1) // (w - 1) for k in range(1, w)]
    assert col_bin == [(UNIT * k * N) // (UNIT * (w - 1) + 1) for k in range(w)] and col_bin[-1] == N - 1
    starts = [col_bin.index(b) for b in sorted(set(col_bin))]
    for c in range(2):
        cols = img[0, c, r0:r1, c0:c1].astype(np.int64).sum(axis=0)
        want = np.zeros(N, np.int64)
        want[sorted(set(col_bin))] = np.add.reduceat(cols, starts)
        assert sums[c, :, 0].astype(np.int64).tolist() == want.tolist()
    assert count[:, 0].tolist() == [(r1 - r0) * col_bin.count(b) for b in range(N)]


@pytest.mark.parametrize("N", [2, 3, 5, 32])
def test_rectangle_along_the_rows_is_reduceat_over_row_sums(N):
    lab, off, img, bbox = rectangle()
    r0, c0, r1, c1 = (int(v) for v in bbox[0])
    h = r1 - r0
    count, sums, extent = pref.profile(lab, off, img, bbox, [[UNIT, 0]], N)
    assert extent[:, 0].tolist() == [UNIT * r0, UNIT * (r1 - 1)]
    row_bin = [0] + [(k * N - 1) // (h - 1) for k in range(1, h)]
    assert row_bin == [(UNIT * k * N) // (UNIT * (h - 1) + 1) for k in range(h)]
    starts = [row_bin.index(b) for b in sorted(set(row_bin))]
    for c in range(2):
        rows = img[0, c, r0:r1, c0:c1].astype(np.int64).sum(axis=1)
        want = np.zeros(N, np.int64)
        want[sorted(set(row_bin))] = np.add.reduceat(rows, starts)
        assert sums[c, :, 0].astype(np.int64).tolist() == want.tolist()
    assert count[:, 0].tolist() == [(c1 - c0) * row_bin.count(b) for b in range(N)]
    assert count[N - 1, 0] > 0 and count[0, 0] > 0


def test_one_pixel_cell_goes_to_bin_0():
    lab = np.zeros((1, 4, 6), np.int64)
    lab[0, 2, 5] = 1
    img = np.full((1, 1, 4, 6), 77, np.uint8)
    count, sums, extent = pref.profile(lab, np.array([0, 1]), img, [[2, 5, 3, 6]], [[11585, -11585]], 8)
    assert count[:, 0].tolist() == [1] + [0] * 7 and sums[0, :, 0].tolist() == [77] + [0] * 7
    assert extent[:, 0].tolist() == [11585 * 2 - 11585 * 5] * 2


def test_direction_zero_puts_everything_in_bin_0():
    lab, off, img, bbox = rectangle()
    count, sums, extent = pref.profile(lab, off, img, bbox, [[0, 0]], 16)
    assert count[:, 0].tolist() == [65] + [0] * 15 and extent.tolist() == [[0], [0]]
    assert int(sums[1, 0, 0]) == int(img[0, 1, 2:7, 3:16].astype(np.int64).sum())


def test_ten_pixel_diagonal_in_32_bins():
    lab = np.zeros((1, 12, 12), np.int64)
    for i in range(10):
        lab[0, 1 + i, 1 + i] = 1
    img = np.arange(144, dtype=np.uint16).reshape(1, 1, 12, 12)
    count, sums, _ = pref.profile(lab, np.array([0, 1]), img, [[1, 1, 11, 11]], [[11585, 11585]], 32)
    got = count[:, 0].tolist()
    assert got[:8] == [1, 0, 0, 1, 0, 0, 0, 1] and sum(got) == 10 and got.count(0) == 22 and got[31] == 1
    assert got == [1 if b in [(23170 * i * 32) // (23170 * 9 + 1) for i in range(10)] else 0 for b in range(32)]
    assert sums[0, 0, 0] == 13 and sums[0, 31, 0] == 130


@pytest.mark.parametrize("d", [(UNIT, 0), (0, UNIT), (11585, 11585), (11585, -11585), (-3, 16000), (UNIT, -UNIT)])
@pytest.mark.parametrize("N", [2, 7, 32])
def test_last_pixel_lands_in_the_last_bin_and_negative_ux_works(d, N):
    rng = np.random.default_rng(5)
    lab = (rng.random((1, 17, 23)) < 0.3).astype(np.int64)
    img = rng.integers(0, 256, (1, 1, 17, 23)).astype(np.uint8)
    count, sums, extent = pref.profile(lab, np.array([0, 1]), img, [[0, 0, 17, 23]], [d], N)
    y, x = np.nonzero(lab[0])
    q = d[0] * y + d[1] * x
    assert extent[:, 0].tolist() == [q.min(), q.max()] and q.max() > q.min()
    assert count[0, 0] >= 1 and count[N - 1, 0] >= 1 and count[:, 0].sum() == len(y)
    assert int(sums[0, :, 0].sum()) == int(img[0, 0][lab[0] == 1].astype(np.int64).sum())
    # pixel by pixel in Python integers
    want = np.zeros(N, np.int64)
    for v in q.tolist():
        want[(v - int(q.min())) * N // (int(q.max()) - int(q.min()) + 1)] += 1
    assert count[:, 0].tolist() == want.tolist()
    assert ((q.max() - q.min()) * N) // (q.max() - q.min() + 1) == N - 1      # the pixel(s) at qmax are in the last bin


def test_other_cells_background_and_foreign_ids_do_not_count():
    lab = np.zeros((1, 6, 8), np.int64)
    lab[0, 1:5, 1:7] = (np.indices((4, 6)).sum(axis=0) % 2) + 1   # a checkerboard of 1 and 2 in one box
    lab[0, 2, 3], lab[0, 3, 3] = 9, -4
    img = np.full((1, 1, 6, 8), 10, np.uint8)
    count, sums, _ = pref.profile(lab, np.array([0, 2]), img, [[1, 1, 5, 7]] * 2, [[0, UNIT]] * 2, 4)
    assert count.sum(axis=0).tolist() == [int((lab == 1).sum()), int((lab == 2).sum())] == [11, 11]
    assert (sums[0].astype(np.int64) == 10 * count).all()


def test_short_and_absent_boxes():
    lab, off, img, bbox = rectangle()
    short = bbox.copy()
    short[0, 3] -= 2
    assert pref.profile(lab, off, img, short, [[0, UNIT]], 8)[0].sum() == 5 * 11
    out = pref.profile(lab, off, img, np.zeros((1, 4)), [[0, UNIT]], 8)
    assert not out[0].any() and not out[1].any() and not out[2].any()
    far = pref.profile(lab, off, img, [[-5, -9, 400, 10 ** 6]], [[0, UNIT]], 8)       # clipped to the frame
    assert np.array_equal(far[0], pref.profile(lab, off, img, bbox, [[0, UNIT]], 8)[0])


# ---- the host half ------------------------------------------------------------------------------------------------------------
def test_profile_direction():
    d = cells.profile_direction([0.0, math.pi / 2, math.pi / 4, -math.pi / 4])
    assert d.dtype == np.int32 and d.shape == (4, 2)
    assert d.tolist() == [[16384, 0], [0, 16384], [11585, 11585], [11585, -11585]]
    assert cells.profile_direction(np.float64(0.3)).tolist() == [[math.floor(16384 * math.cos(0.3) + 0.5),
                                                                 math.floor(16384 * math.sin(0.3) + 0.5)]]
    assert cells.profile_direction([]).shape == (0, 2)


def test_check_profile():
    assert cells.check_profile(None) is None
    assert cells.check_profile(2) == 2 and cells.check_profile(32) == 32 and cells.check_profile(np.int64(16)) == 16
    assert cells.check_profile(8.0) == 8
    for bad in (1, 33, 0, -4, True, False, "8", b"8", 2.5, float("nan"), float("inf"), [8], (4, 5)):
        with pytest.raises(ValueError):
            cells.check_profile(bad)


def test_pole_bins_spelled_out():
    assert cells.pole_bins(2) == ([], [])
    assert cells.pole_bins(4) == ([0], [3])
    assert cells.pole_bins(5) == ([0], [4])
    assert cells.pole_bins(8) == ([0, 1], [6, 7])
    assert cells.pole_bins(32) == (list(range(8)), list(range(24, 32)))
    for N in range(2, 33):
        lo, hi = cells.pole_bins(N)
        assert lo == [b for b in range(N) if (2 * b + 1) / N - 1 < -0.5] and len(lo) == len(hi)
        assert hi == [N - 1 - b for b in reversed(lo)]


def test_summary_peak_at_a_pole():
    # N = 8: pole bins 0, 1 and 6, 7
    count = [4, 4, 4, 4, 4, 4, 4, 4]
    sums = [400, 200, 40, 40, 40, 40, 100, 100]
    ratio, asym, peak = cells.profile_columns(count, sums)
    assert ratio == (800 * 16) / (16 * 160) == 5.0                 # pole mean 50 over mid mean 10
    assert asym == abs(600 * 8 - 200 * 8) / (600 * 8 + 200 * 8) == 0.5      # A = 75, B = 25
    assert peak == 1 / 8 - 1 == -0.875


def test_summary_peak_at_mid_cell():
    count = [2, 3, 5, 5, 5, 5, 3, 2]
    sums = [20, 30, 50, 500, 450, 50, 30, 20]
    ratio, asym, peak = cells.profile_columns(count, sums)
    assert ratio == (100 * 20) / (10 * 1050) and ratio < 1       # pole mean 10 over mid mean 52.5
    assert asym == 0.0
    assert peak == 7 / 8 - 1 == -0.125                            # bin 3, mean 100


def test_summary_tie_goes_to_the_smaller_bin():
    # bins 1 and 2 have the mean 7 / 3 exactly, as 14 / 6 and 7 / 3: a float compare could differ, the integers cannot
    count = [1, 6, 3, 1]
    sums = [2, 14, 7, 2]
    ratio, asym, peak = cells.profile_columns(count, sums)
    assert peak == 3 / 4 - 1 == -0.25
    assert ratio == (4 * 9) / (2 * 21) and asym == 0.0
    assert cells.profile_columns([3, 1, 6, 1], [7, 2, 14, 2])[2] == 1 / 4 - 1      # the same means, the other way round
    big = 2 ** 40 + 1                                             # the means differ by one part in 2^80: no fp64 sees it
    assert cells.profile_columns([big, big + 1, 1, 1], [big - 1, big, 0, 0])[2] == 3 / 4 - 1
    assert cells.profile_columns([big + 1, big, 1, 1], [big, big - 1, 0, 0])[2] == 1 / 4 - 1


def test_summary_empty_pole_and_empty_cells():
    ratio, asym, peak = cells.profile_columns([0, 5, 5, 2], [0, 50, 100, 60])
    assert ratio == (60 * 10) / (2 * 150) == 2.0                  # the pole group still has the other end
    assert math.isnan(asym) and peak == 7 / 4 - 1 == 0.75
    ratio, asym, peak = cells.profile_columns([0, 5, 5, 0], [0, 50, 100, 0])
    assert math.isnan(ratio) and math.isnan(asym) and peak == 0.25
    ratio, asym, peak = cells.profile_columns([3, 0, 0, 3], [30, 0, 0, 90])      # no mid-cell pixel
    assert math.isnan(ratio) and asym == 0.5 and peak == 0.75
    assert all(math.isnan(v) for v in cells.profile_columns([4, 4], [1, 2])[:2])   # N = 2 has no pole bins
    assert cells.profile_columns([4, 4], [1, 2])[2] == 0.5
    assert all(math.isnan(v) for v in cells.profile_columns([0] * 4, [0] * 4))
    ratio, asym, peak = cells.profile_columns([2, 2, 2, 2], [0, 0, 0, 0])        # a dark cell
    assert math.isnan(ratio) and math.isnan(asym) and peak == -0.75
    assert cells.profile_columns([2, 2, 2, 2], [5, 0, 0, 5])[0] == math.inf


def columns_by_fractions(count, sums):
    """the three summary columns of one cell restated with fractions.Fraction, straight from their definitions"""
    from fractions import Fraction
    cnt, sm = [int(v) for v in count], [int(v) for v in sums]
    N = len(cnt)
    nan = float("nan")
    lo, hi = [b for b in range(N) if 4 * b + 2 < N], [b for b in range(N) if 4 * b + 2 > 3 * N]
    mid = [b for b in range(N) if b not in lo + hi]
    mean = lambda bins: Fraction(sum(sm[b] for b in bins), sum(cnt[b] for b in bins)) if sum(cnt[b] for b in bins) else None
    pole, rest, A, B = mean(lo + hi), mean(mid), mean(lo), mean(hi)
    if pole is None or rest is None or (pole == 0 and rest == 0):
        ratio = nan
    else:
        ratio = float(pole / rest) if rest else math.inf
    asym = float(abs(A - B) / (A + B)) if A is not None and B is not None and A + B else nan
    full = [b for b in range(N) if cnt[b]]
    peak = (2 * max(full, key=lambda b: (Fraction(sm[b], cnt[b]), -b)) + 1) / N - 1 if full else nan
    return ratio, asym, peak


def test_many_cells_at_once_against_fractions():
    rng = np.random.default_rng(11)
    for N in (2, 3, 4, 5, 8, 16, 32):
        n = 400
        count = rng.integers(0, 6, (N, n)) * (rng.random((N, n)) < 0.7)
        sums = count * rng.integers(0, 4, (N, n)) + (rng.random((N, n)) < 0.2) * (count > 0)      # many ties, many zeros
        count[:, :3], sums[:, :3] = 0, 0
        count[:, 3], sums[:, 3] = 2 ** 31 - 1, (2 ** 31 - 1) * 65535                               # the largest sums there are
        count[0, 4], sums[0, 4] = 3 * 10 ** 8, 7 * 10 ** 8                                         # 7 / 3 three times: equal in
        count[N - 1, 4], sums[N - 1, 4] = 3, 7                                                     # integers and in fp64
        count[1:N - 1, 4], sums[1:N - 1, 4] = 0, 0
        got = cells.profile_columns(count, sums)
        assert len(got) == 3 and all(len(col) == n for col in got)
        for s in range(n):
            want = columns_by_fractions(count[:, s], sums[:, s])
            one = cells.profile_columns(count[:, s], sums[:, s])                                   # one cell: the same function
            for g, w, o in zip(got, want, one):
                assert (math.isnan(g[s]) and math.isnan(w) and math.isnan(o)) or g[s] == w == o, (N, s, g[s], w, o)
        assert all(type(v) is float for col in got for v in col)
    assert [len(col) for col in cells.profile_columns(np.zeros((16, 0), np.uint32), np.zeros((16, 0), np.uint64))] == [0, 0, 0]
    # two bins whose exact means differ and whose fp64 means do not: the integers decide
    a, b, k = 13, 12, 692861481133922
    assert (a * k - 1) / (b * k) == a / b and (a * k - 1) * b < a * b * k and a * k < 2 ** 53
    for order in ((0, 1), (1, 0)):
        count, sums = np.zeros((4, 1), np.int64), np.zeros((4, 1), np.int64)
        count[order[0] + 1, 0], sums[order[0] + 1, 0] = b * k, a * k - 1          # the smaller mean
        count[order[1] + 1, 0], sums[order[1] + 1, 0] = b, a                      # the larger one
        assert sums.max() < 2 ** 53
        assert cells.profile_columns(count, sums)[2] == [(2 * (order[1] + 1) + 1) / 4 - 1]
        assert columns_by_fractions(count[:, 0], sums[:, 0])[2] == (2 * (order[1] + 1) + 1) / 4 - 1


def test_empty_stack_gives_the_empty_table_with_the_profile_columns():
    """a stack without a cell (a blank field of view): the profile integers are empty, the table is too"""
    import cells_ref as ref
    lab = np.zeros((2, 6, 9), np.int64)
    off = ref.frame_tables(lab)
    assert off.tolist() == [0, 0, 0]
    img = np.full((2, 2, 6, 9), 7, np.uint16)
    raw = ref.measure(lab, off, img)
    for N in (2, 16, 32):
        prof = (np.zeros((N, 0), np.uint32), np.zeros((2, N, 0), np.uint64), np.zeros((2, 0), np.int64))
        same = pref.profile(lab, off, img, np.zeros((0, 4)), np.zeros((0, 2)), N)
        assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(prof, same))
        df = cells.table_from_sums(off, 6, 9, raw, [0, 1], profile=prof)
        assert len(df) == 0 and list(df.columns) == cells.columns([0, 1], False, profile=True)
        assert list(df.columns)[:-7] == list(cells.table_from_sums(off, 6, 9, raw, [0, 1]).columns)
        rows = cells.profiles_from_raw(off, raw["shape"][0], [0, 1], prof[0], prof[1])
        assert len(rows) == 0 and list(rows.columns) == cells.PROFILE_TABLE_COLUMNS
    assert cells._cell_directions(raw).shape == (0, 2)


# ---- the kernel's division, restated in numpy float32 -------------------------------------------------------------------------
def quotient_like_the_kernel(num, D, ulps=0):
    """pf_quotient of csrc/profile.hip step by step with numpy's IEEE float32: b = int(min(float(num) * (1.0f / float(D)), 32)),
    r = num - b D in 64 bits, b - 1 if r < 0, b + 1 if r >= D.  ``ulps``: the reciprocal moved by so many float32 steps, as a
    reciprocal instruction of that accuracy would give it.  num, D: uint64 arrays"""
    rcp = np.float32(1) / D.astype(np.float32)
    for _ in range(abs(ulps)):
        rcp = np.nextafter(rcp, np.float32(np.inf if ulps > 0 else 0))
    b = np.minimum(num.astype(np.float32) * rcp, np.float32(32)).astype(np.int64)
    with np.errstate(over="ignore"):
        r = (num - b.astype(np.uint64) * D).view(np.int64)
    return np.where(r < 0, b - 1, np.where(r.view(np.uint64) >= D, b + 1, b))


@pytest.mark.parametrize("ulps", [0, -2, 2])
def test_the_kernels_quotient_is_the_floor_at_bin_edges_and_large_extents(ulps):
    """the fp32 estimate with the 64-bit correction equals floor(num / D) for every N, for extents D up to 2^57, at the bin
    edges ceil(k D / N) and one beside them, at both ends, and for random numerators"""
    rng = np.random.default_rng(21 + ulps)
    m = 20000
    bits = rng.integers(1, 58, m)
    D = (rng.integers(0, 2 ** 62, m, dtype=np.int64).astype(np.uint64) >> (62 - bits).astype(np.uint64)) | np.uint64(1)
    third = np.arange(m) % 3 == 0
    D[third] = (np.uint64(1) << (bits[third] - 1).astype(np.uint64)) + rng.integers(0, 3, int(third.sum())).astype(np.uint64)
    D[:8] = [1, 2, 3, 16384 * 69999 + 1, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 57 - 1, 23170 * 9 + 1]
    checked = 0
    for N in range(2, 33):
        k = rng.integers(0, N, m).astype(object)
        Do = D.astype(object)
        edge = (k * Do + N - 1) // N                                  # the first q - qmin of bin k
        for dq in (edge, edge - 1, edge + 1, Do - 1, Do * 0, rng.integers(0, 2 ** 62, m).astype(object) % Do):
            dq = np.clip(dq, 0, Do - 1)
            want = np.array((dq * N) // Do, np.int64)
            got = quotient_like_the_kernel(np.array(dq * N, np.uint64), D, ulps)
            assert np.array_equal(got, want), (N, ulps, int(np.flatnonzero(got != want)[0]))
            assert want.max() <= N - 1
            checked += m
    assert checked == 31 * 6 * m


def test_axis_extent():
    assert cells.axis_extent(0, 0) == 1.0
    assert cells.axis_extent(-16384 * 3, 16384 * 25) == 29.0
    assert cells.axis_extent(11585 * 2, 11585 * 20) == 11585 * 18 / 16384 + 1


def test_profile_table_from_integers():
    off = np.array([0, 2, 3], np.int64)
    area = np.array([3, 0, 4])
    count = np.array([[1, 0, 4], [2, 0, 0]], np.uint32)
    sums = np.array([[[10, 0, 8], [30, 0, 0]], [[1, 0, 2], [3, 0, 0]]], np.uint64)
    df = cells.profiles_from_raw(off, area, [2, 0], count, sums)
    assert list(df.columns) == cells.PROFILE_TABLE_COLUMNS == ['frame', 'channel', 'label', 'bin', 'bin_pos', 'count', 'sum',
                                                               'mean']
    assert df[['frame', 'channel', 'label', 'bin']].values.tolist() == [
        [0, 2, 1, 0], [0, 2, 1, 1], [0, 0, 1, 0], [0, 0, 1, 1], [1, 2, 1, 0], [1, 2, 1, 1], [1, 0, 1, 0], [1, 0, 1, 1]]
    assert df['bin_pos'].tolist() == [-0.5, 0.5] * 4
    assert df['count'].tolist() == [1, 2, 1, 2, 4, 0, 4, 0] and df['sum'].tolist() == [10, 30, 1, 3, 8, 0, 2, 0]
    mean = df['mean'].tolist()
    assert mean[:5] == [10.0, 15.0, 1.0, 1.5, 2.0] and math.isnan(mean[5]) and mean[6] == 0.5 and math.isnan(mean[7])


def test_columns_with_profile():
    plain = cells.columns([0, 2], True)
    assert cells.columns([0, 2], True, profile=False) == plain
    assert cells.columns([0, 2], True, profile=True) == plain + [
        'axis_extent', 'pole_mid_ratio_ch0', 'pole_asym_ch0', 'profile_peak_ch0', 'pole_mid_ratio_ch2', 'pole_asym_ch2',
        'profile_peak_ch2']
    with_spots = cells.columns([1], False, spots=True, profile=True)
    assert with_spots[-4:] == ['axis_extent', 'pole_mid_ratio_ch1', 'pole_asym_ch1', 'profile_peak_ch1']
    assert with_spots[-5] == 'bg_spots_ch1'
    import inspect
    assert list(inspect.signature(cells.columns).parameters)[-1] == 'profile'
    assert list(inspect.signature(cells.measure_cells).parameters)[-1] == 'profile'
    assert inspect.signature(cells.measure_cells).parameters['profile'].default is None


def test_table_from_sums_with_profile_integers():
    """the table from restated integers alone: no device"""
    import cells_ref as ref
    lab = np.zeros((1, 12, 40), np.int64)
    lab[0, 3:7, 4:33] = 1                                         # a 29-pixel rod along the columns
    lab[0, 9, 2] = 2
    off = ref.frame_tables(lab)
    img = np.full((1, 1, 12, 40), 5, np.uint16)
    img[0, 0, 3:7, 4:12] = 50                                     # the eight columns of the pole bins 0 .. 7
    raw = ref.measure(lab, off, img)
    dirs = cells._cell_directions(raw)
    assert dirs.tolist() == [[0, 16384], [11585, 11585]]          # equal variances (a single pixel): +pi/4
    prof = pref.profile(lab, off, img, raw["bbox"], dirs, 32)
    assert (prof[0][:, 0] == 0).sum() == 3                        # 29 pixel columns in 32 bins: three stay empty
    df = cells.table_from_sums(off, 12, 40, raw, [0], profile=prof)
    assert list(df.columns) == cells.columns([0], False, profile=True)
    assert df['axis_extent'].tolist() == [29.0, 1.0]
    assert df['profile_peak_ch0'].tolist() == [1 / 32 - 1, 1 / 32 - 1]
    assert df['pole_mid_ratio_ch0'][0] > 1 and math.isnan(df['pole_mid_ratio_ch0'][1])
    assert df['pole_asym_ch0'][0] == (50 - 5) / (50 + 5) and math.isnan(df['pole_asym_ch0'][1])
    plain = cells.table_from_sums(off, 12, 40, raw, [0])
    assert plain.equals(df[list(plain.columns)])
    with pytest.raises(ValueError):
        cells.table_from_sums(off, 12, 40, ref.measure(lab, off), [], profile=prof)


def test_measure_cells_refuses_a_profile_without_an_image():
    lab = np.zeros((1, 4, 4), np.int32)
    with pytest.raises(ValueError, match="profile"):
        cells.measure_cells(lab, profile=1, device="cpu")
    with pytest.raises(ValueError, match="no image"):
        cells.measure_cells(lab, profile=8, device="cpu")


def test_infer_worker_default():
    from microbeseg_amd.inference.infer import InferWorker
    assert InferWorker.profile is None and hasattr(InferWorker, "profile_table")


# ---- the command line ---------------------------------------------------------------------------------------------------------
BASE = ["-i", "x", "-m", "y"]
ON = BASE + ["--cells"]


def _parser():
    import infer_script_local as script
    return script.build_parser()


def test_profile_values():
    parser = _parser()
    assert parser.parse_args(BASE).profile is None and parser.parse_args(ON).profile is None
    assert parser.parse_args(ON + ["--profile"]).profile == 16                      # the bare flag
    for n in (2, 8, 32):
        assert parser.parse_args(ON + ["--profile", str(n)]).profile == n
    args = parser.parse_args(BASE + ["--profile", "--spots", "40", "--cells"])
    assert (args.profile, args.spots) == (16, 40)
    action, = [a for a in parser._actions if "--profile" in a.option_strings]
    assert action.help.startswith("[extension]") and action.type is int
    assert action.nargs == "?" and action.const == 16 and action.default is None


@pytest.mark.parametrize("extra", [["--profile"], ["--profile", "8"]])
def test_profile_without_cells_is_refused_with_the_scripts_message(extra, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(BASE + extra)
    assert exit_.value.code == 2 and "--profile needs --cells" in capsys.readouterr().err


@pytest.mark.parametrize("value", ["1", "0", "33", "-2"])
def test_profile_out_of_range_is_refused_with_the_scripts_message(value, capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(ON + ["--profile", value])
    err = capsys.readouterr().err
    assert exit_.value.code == 2 and "--profile: " in err and "2 .. 32 expected" in err and f"got {value}" in err


def test_profile_that_is_no_whole_number_is_refused(capsys):
    with pytest.raises(SystemExit) as exit_:
        _parser().parse_args(ON + ["--profile", "2.5"])
    assert exit_.value.code == 2 and "argument --profile: invalid int value: '2.5'" in capsys.readouterr().err
