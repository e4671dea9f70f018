"""CPU: the structured stacks of tests/cells_cases.py do what they are meant to do, and the vectorised restatements
measure_fast / links_fast of tests/cells_ref.py, which judge the device on them, equal the per-label loops.

cells_cases.model() restates how cm_kernel splits a stack; its counters say which paths a case makes the kernel take.
With one deliberate defect switched on it must disagree with measure_fast on a named case (test_non_vacuity prints the
table), and the same defects are tried on the scenes of tests/test_gpu_cells.py: NOTICED_BEFORE records which of them
those scenes could have noticed.  No GPU."""
import functools

import numpy as np
import pytest

import cells_cases as CC
import cells_ref as ref
from test_cells_host import CASES as REGIONPROPS, load_case

KEYS = ("shape", "bbox", "ch_sums", "ch_minmax", "bg_sums", "bg_minmax")
SMALL = [n for n in CC.MEASURE if n[:2] in ("M3", "M4", "M5")]


def same(got, want):
    return all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in KEYS)


@functools.lru_cache(maxsize=None)
def case(name):
    return (CC.MEASURE.get(name) or CC.LINKS[name])()


@functools.lru_cache(maxsize=None)
def truth(name):
    return ref.measure_fast(*case(name))


@functools.lru_cache(maxsize=None)
def modelled(name):
    return CC.model(*case(name))


# ---- the scenes of tests/test_gpu_cells.py ----------------------------------------------------------------------------------------
def old_scenes():
    """(name, labels, off, img) as test_gpu_cells.py builds them: scene_a, shape_b (every length), shape_c, the layouts frame"""
    from test_gpu_cells import scene_a
    rng = np.random.default_rng(11)
    img16 = rng.integers(0, 65536, (3, 2, 37, 53)).astype(np.uint16)
    for dt in (np.uint16, np.int32):
        lab, off = scene_a(dt)
        yield f"scene_a[{np.dtype(dt).name}]", lab, off, img16
    lab, off = scene_a(np.uint16)
    yield "layouts", lab[:1], off[:2], img16[:1]
    img = np.random.default_rng(5).integers(0, 65536, (1, 2, 8, 200)).astype(np.uint16)
    for length in range(1, 71):
        lab = np.zeros((1, 8, 200), np.uint16)
        for r, x0 in enumerate(range(61, 67)):
            lab[0, r, x0:x0 + length] = r + 1
        lab[0, 6, 200 - length:] = 7
        lab[0, 7, :length] = 7
        yield f"shape_b[{length}]", lab, np.array([0, 7], np.int64), img
    full = np.full((1, 1, 300, 300), 65535, np.uint16)
    yield "shape_c[ones]", np.ones((1, 300, 300), np.uint16), np.array([0, 1], np.int64), full
    yield "shape_c[zeros]", np.zeros((1, 300, 300), np.uint16), np.array([0, 0], np.int64), full


# ---- the fast restatements are the slow ones --------------------------------------------------------------------------------------
def test_fast_restatements_equal_the_loops_on_the_known_scenes():
    from test_gpu_cells import random_small_labels, scene_a, scripted_scene
    rng = np.random.default_rng(3)
    stacks = []
    for dt in (np.uint16, np.int32):
        lab, off = scene_a(dt)
        stacks.append((lab, off, rng.integers(0, 65536, (3, 2, 37, 53)).astype(np.uint16)))
    for lab in (scripted_scene(), random_small_labels()):
        stacks.append((lab, ref.frame_tables(lab), rng.integers(0, 256, (lab.shape[0], 1) + lab.shape[1:]).astype(np.uint8)))
    for name in REGIONPROPS:
        g = load_case(name)
        stacks.append((g["label"][None], ref.frame_tables(g["label"][None]), g["img"][None, None]))
    for lab, off, img in stacks:
        assert same(ref.measure_fast(lab, off, img), ref.measure(lab, off, img))
        assert same(ref.measure_fast(lab, off), ref.measure(lab, off))
        for a, b in zip(ref.links_fast(lab, off), ref.links(lab, off)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", SMALL)
def test_fast_restatements_equal_the_loops_on_the_new_cases(name):
    """M3 to M5 at their full size (the loops take a second at most there; M1, M2 and M6 are what they are too slow for)"""
    lab, off, img = case(name)
    assert same(truth(name), ref.measure(lab, off, img))
    if lab.shape[0] > 1:
        for a, b in zip(ref.links_fast(lab, off), ref.links(lab, off)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["L1_exact_fill", "L2_one_over_many", "L2_many_over_one"])
def test_fast_links_equal_the_loop_on_the_links_cases(name):
    lab, off, _ = case(name)
    for dt in (np.uint16, np.int32):
        for a, b in zip(ref.links_fast(lab.astype(dt), off), ref.links(lab, off)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(CC.MEASURE))
def test_model_without_a_defect_equals_the_restatement(name):
    got, _ = modelled(name)
    assert same(got, truth(name))
    lab, off, img = case(name)
    if name.startswith("M1"):
        assert same(CC.model(lab, off, None)[0], ref.measure_fast(lab, off, None))


# ---- each case holds what it claims -----------------------------------------------------------------------------------------------
def test_cases_are_read_only_and_typed():
    for name in list(CC.MEASURE) + list(CC.LINKS):
        lab, off, img = case(name)
        assert not lab.flags.writeable and not off.flags.writeable and off.dtype == np.int64 and off[0] == 0, name
        assert lab.dtype in (np.uint16, np.int32) and len(off) == lab.shape[0] + 1, name
        if name in CC.MEASURE:
            assert img.dtype in (np.uint8, np.uint16) and not img.flags.writeable and img.shape[1] in (1, 2), name
            assert img.shape == (lab.shape[0], img.shape[1]) + lab.shape[1:], name
        assert lab.size <= 4.4e6, name


def test_m1_m2_waves_own_several_steps_and_change_frame():
    a, b, m2 = (modelled(n)[1] for n in ("M1_tiny_frames_a", "M1_tiny_frames_b", "M2_three_steps"))
    assert (a["chunks"], a["steps"], a["waves"], a["per"], a["idle"], a["crossing"]) == (1, 4099, 4096, 2, 2046, 2049)
    assert (b["chunks"], b["steps"], b["waves"], b["per"], b["idle"], b["crossing"]) == (3, 4101, 4096, 2, 2045, 683)
    assert (m2["chunks"], m2["steps"], m2["per"], m2["crossing"]) == (2818, 8454, 3, 2) and 2818 % 3 != 0
    for name in ("M1_tiny_frames_a", "M1_tiny_frames_b"):
        lab, off, _ = case(name)
        K = np.diff(off)
        flat = lab.reshape(lab.shape[0], -1)
        cells = np.array([np.unique(f[(f > 0) & (f <= k)]).size for f, k in zip(flat, K)])
        assert set(cells) == {0, 1, 2, 3}, name
        assert (flat == 0).all(axis=1).any(), "a frame that is all background"
        assert (flat != 0).all(axis=1).any(), "a frame without background"
        assert ((cells == 0) & (flat > K[:, None]).any(axis=1)).any(), "a frame whose only label is beyond the table"
    lab, off, _ = case("M2_three_steps")
    big = int(off[1])
    area = [(lab[t] == big).sum() for t in range(3)]
    assert area[0] >= 2 ** 20 and np.array_equal(lab[0] == big, lab[1] == big) and np.array_equal(lab[1] == big, lab[2] == big)
    t = truth("M2_three_steps")["shape"][0]
    assert (t > 0).sum() > 17000 and 0.75 < np.median(t[t > 0]) / 63 < 0.85         # 7 x 9 blocks, 20 % holes


def test_m3_every_scan_step_merges_and_stops_and_a_run_fills_a_wave():
    for name in ("M3_long_runs_i32", "M3_long_runs_u16"):
        info = modelled(name)[1]
        assert info["per"] == 1 and info["crossing"] == 0
        assert all(info["merged"][d] > 0 and info["stopped"][d] > 0 for d in CC.SCAN_STEPS), info
        assert info["full_wave_runs"] > 0 and info["longest_run"] == CC.CHUNK
    lab, off, _ = case("M3_long_runs_i32")
    H, W = lab.shape[1:]
    lengths = [8 * m + r for m in CC.M3_M for r in CC.M3_R]
    assert len(lengths) == 48 and max(lengths) == 527
    for t, n in enumerate(lengths):
        for row in range(H):
            p = np.flatnonzero(lab[t, row]) + row * W
            assert p.size == n and p[-1] - p[0] == n - 1 and (lab[t, row][lab[t, row] > 0] == row + 1).all()
            if row < 3:
                assert p[0] % CC.CHUNK == CC.M3_BEGIN[row], (t, row)
            else:
                assert (CC.CHUNK - 1) - p[-1] % CC.CHUNK == CC.M3_END[row - 3], (t, row)
    assert all((lab[48, r] == r + 1).all() for r in range(H)) and (lab[49] == 1).all()      # rows filled whole


def test_m4_m5_m6_and_links_cases_hold_the_stated_structure():
    for W in (63, 64, 65):
        lab, off, _ = case(f"M4_alternation_w{W}")
        assert set(np.unique(lab)) == {0, 1, 3, 5} and np.diff(off).tolist() == [3] * 6
        for j, q in enumerate(CC.M4_PERIODS):
            flat = lab[j].ravel().astype(int)
            assert (np.diff(np.flatnonzero(np.diff(flat) != 0)) == q).all(), (W, q)
    # the whole-frame fills: every lane starts a row (W = 8), holds a row end (W = 4), every pixel is its own row (W = 1)
    assert [case(f"M4_fill_w{w}")[0].shape for w in (64, 8, 4, 1)] == [(1, 1000, w) for w in (64, 8, 4, 1)]
    assert case("M4_fill_h1")[0].shape == (1, 1, 5000) and all((case(n)[0] == 1).all() for n in CC.MEASURE if "fill" in n)
    assert modelled("M4_fill_w8")[1]["longest_run"] == 8 and modelled("M4_fill_w1")[1]["longest_run"] == 1
    for K in (65535, 65534):
        lab, off, _ = case(f"M5_id_edges_u16_k{K}")
        assert {1, 32767, 32768, 65535} <= set(np.unique(lab)) and np.diff(off).tolist() == [K, K]
        area = truth(f"M5_id_edges_u16_k{K}")["shape"][0]
        assert area[32768 - 1] > 0 and (K == 65534 or area[65535 - 1] > 0) and (area > 0).sum() == 2 * (4 if K == 65535 else 3)
    lab, off, img = case("M5_id_edges_i32")
    assert {-1, -2 ** 31, 2 ** 31 - 1, 1, 2, 3} <= set(np.unique(lab).tolist())
    t = truth("M5_id_edges_i32")
    assert t["bg_sums"][0, :, 0].tolist() == [(lab[f] == 0).sum() for f in range(2)]
    assert ((lab[0] < 0) | (lab[0] > 3)).sum() > 0 and t["shape"][0].sum() + t["bg_sums"][0, :, 0].sum() < lab.size
    lab, off, _ = case("M6_wide_frame")
    assert lab.shape == (1, 2, 2_200_000) and modelled("M6_wide_frame")[1]["per"] == 3
    shape, bbox = CC.wide_frame_sums()
    t = truth("M6_wide_frame")
    assert [[int(v) for v in row] for row in t["shape"]] == shape and t["bbox"].tolist() == bbox
    assert shape[0] == [45 + 47 + 100, 2_097_100, 8] and max(shape[4]) < 2 ** 64
    # links
    lab, off, _ = case("L1_exact_fill")
    assert [len(ref.pairs(lab, off, t)[0]) for t in (1, 2)] == [CC.L1_CAP, CC.L1_CAP + 1]
    for name, t_one in (("L2_one_over_many", 1), ("L2_many_over_one", 0)):
        lab, off, _ = case(name)
        l, m, count = ref.pairs(lab, off, 1)
        assert l.size > 1900 and (count == 6).all() and (lab[t_one] == 1).all(), name
    pred, ovl = ref.links_fast(*case("L2_one_over_many")[:2])
    grid = case("L2_one_over_many")[0][0]
    assert pred[-1] == grid[grid > 0].min() and ovl[-1] == 6
    assert ref.links_fast(*case("L3_three_steps")[:2])[1].max() > 2 ** 20


# ---- non-vacuity ------------------------------------------------------------------------------------------------------------------
# where each defect is looked for (the model takes a second on the stacks of millions of pixels, so not everywhere)
LOOK = {d: SMALL for d in CC.DEFECTS}
LOOK["no_bg_flush_on_frame_change"] = ["M1_tiny_frames_a", "M1_tiny_frames_b"]
LOOK["u64_sum_xx"] = SMALL + ["M6_wide_frame"]
# which defects the scenes of tests/test_gpu_cells.py notice (the model on old_scenes()).  The two scan steps are noticed
# by one scene only, the 300-pixel rows of shape_c (its runs reach 38 lanes: longer than the 70 pixels of shape_b, but
# none fills a wave), a link across a row's first pixel by the label of shape_b that goes on at column 0 of the next row
# and by the whole-frame label of shape_c (W = 200 and 300: rows that begin at a lane's first pixel).
# Nothing there makes a wave change frame, uses an id above 1000 or below 0, or reaches column 2^21.
NOTICED_BEFORE = {"drop_scan_d16": True, "drop_scan_d32": True, "no_bg_flush_on_frame_change": False, "link_across_x0": True,
                  "u16_top_bit_is_sign": False, "negative_is_background": False, "u64_sum_xx": False}


def test_non_vacuity(capsys):
    table, before = {}, {}
    scenes = [(n, lab, off, img, ref.measure_fast(lab, off, img)) for n, lab, off, img in old_scenes()]
    for defect in CC.DEFECTS:
        table[defect] = [n for n in LOOK[defect] if not same(CC.model(*case(n), defect=defect)[0], truth(n))]
        before[defect] = [n for n, lab, off, img, want in scenes if not same(CC.model(lab, off, img, defect=defect)[0], want)]
    with capsys.disabled():
        print("\ndefect -> new cases that notice it | scenes of test_gpu_cells.py that notice it")
        for defect in CC.DEFECTS:
            old = before[defect][:2] + ([f"... {len(before[defect])} in all"] if len(before[defect]) > 2 else [])
            print(f"  {defect:30s} {', '.join(table[defect]) or '-'} | {', '.join(old) or '-'}")
    for n, lab, off, img, want in scenes:
        assert same(CC.model(lab, off, img)[0], want), n
    for defect in CC.DEFECTS:
        assert table[defect], f"no new case notices {defect}"
        assert bool(before[defect]) == NOTICED_BEFORE[defect], (defect, before[defect])
    assert set(before["drop_scan_d16"]) == set(before["drop_scan_d32"]) == {"shape_c[ones]"}
    assert all(n.startswith("shape_b") or n == "shape_c[ones]" for n in before["link_across_x0"])
    assert {"M3_long_runs_i32", "M3_long_runs_u16"} <= set(table["drop_scan_d16"]) & set(table["drop_scan_d32"])
    assert table["u64_sum_xx"] == ["M6_wide_frame"]
    assert "M5_id_edges_i32" in table["negative_is_background"] and "M5_id_edges_u16_k65535" in table["u16_top_bit_is_sign"]


# ---- the overflow, without a GPU --------------------------------------------------------------------------------------------------
def test_old_closed_form_fails_on_the_runs_that_span_column_2_21():
    """The 64-bit closed form S(b) - S(a - 1) replayed in Python integers modulo 2^64 on every run that the kernel adds
    for M6 (the model's cuts), and on the whole runs that rs_runs_kernel takes.  m (m + 1) (2m + 1) wraps once for
    2^21 <= m < 2 642 245; 2^64 = 4 (mod 6), so S(b) and S(a - 1) both come out 2^64 / 6 too small (rounded alike) when both
    have wrapped, and their difference is right again: the form is wrong exactly where a - 1 < 2^21 <= b."""
    sq = lambda m: m * (m + 1) * (2 * m + 1) // 6
    assert 2_642_245 * 2_642_246 * (2 * 2_642_245 + 1) < 2 ** 65 <= 2_642_246 * 2_642_247 * (2 * 2_642_246 + 1) and CC.M6_W < 2_642_245
    # the three runs of the issue text
    assert CC.old_sum_xx(2_097_140, 2_097_147) == sq(2_097_147) - sq(2_097_139)
    assert CC.old_sum_xx(2_097_145, 2_097_152) != sq(2_097_152) - sq(2_097_144)
    assert CC.old_sum_xx(2_097_152, 2_097_159) != sq(2_097_159) - sq(2_097_151)
    y, x0, n = modelled("M6_wide_frame")[1]["runs"]
    pieces = [(int(a), int(a + k - 1)) for a, k in zip(x0, n)]
    whole = [(a, b) for _, _, a, b in CC.M6_RUNS]
    for runs in (pieces, whole):
        wrong = [(a, b) for a, b in runs if CC.old_sum_xx(a, b) != sq(b) - sq(a - 1)]
        assert wrong and wrong == [(a, b) for a, b in runs if a - 1 < CC.WRAP <= b]
        assert any(a - 1 >= CC.WRAP for a, b in runs) and any(b < CC.WRAP for a, b in runs)
    assert sorted(a for a, b in pieces if a - 1 < CC.WRAP <= b) == [2_097_100, 2_097_152]      # cell 1 in row 1; cell 3's last pixel
    assert [(a, b) for a, b in whole if a - 1 < CC.WRAP <= b] == [(2_097_145, 2_097_152), (2_097_100, 2_097_199)]
    # and the model with that form loses exactly these cells
    got = CC.model(*case("M6_wide_frame"), defect="u64_sum_xx")[0]
    want = truth("M6_wide_frame")
    assert (got["shape"][4] != want["shape"][4]).tolist() == [True, False, True]
    assert all(np.array_equal(got[k], want[k]) for k in KEYS if k != "shape") and np.array_equal(got["shape"][[0, 1, 2, 3, 5]], want["shape"][[0, 1, 2, 3, 5]])
