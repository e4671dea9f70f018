"""CPU: the structured worst-case frames of tests/geometry_ref.py have the properties they were built for, and the C oracle
reproduces the reference's answers on them (tests/golden/postproc_geometry.npz, made by tools/gen_golden_postproc.py with the
real reference) bit for bit — so the oracle may judge the device on every other pattern of the family."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import geometry_ref as G
from helpers import load_npz
from oracle import eval_ref, postproc_ref as R


@pytest.fixture(scope="module")
def fx():
    return load_npz("postproc_geometry.npz")


def _oracle(cell, border, th_cell, th_seed, hw1=True):
    if hw1:
        return R.distance_postprocessing(border[..., None], cell[..., None], th_seed, th_cell)
    return R.distance_postprocessing(border, cell, th_seed, th_cell)


# ---- the oracle against the reference's own answers --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice_61x67", "lattice_120x130", "serpentine_65x70", "plateau", "mirror_vertical",
                                  "mirror_horizontal", "mirror_point"])
def test_oracle_equals_reference_on_distance_patterns(name, fx):
    cell, border, _ = G.fixture_distance_cases()[name]
    assert np.array_equal(cell, fx[f"{name}/cell"]) and np.array_equal(border, fx[f"{name}/border"]), "generator drifted"
    assert np.array_equal(fx["th"], np.array(G.THS))
    for j, (th_cell, th_seed) in enumerate(G.THS):
        for key, hw1 in ((f"{name}/labels_hw1_{j}", True), (f"{name}/labels_2d_{j}", False)):
            got = _oracle(cell, border, th_cell, th_seed, hw1)
            assert got.dtype == np.uint16 and np.array_equal(got, fx[key]), f"{key}: {(got != fx[key]).sum()} px differ"


@pytest.mark.parametrize("name", ["checkerboard_64x65", "serpentine_129x131"])
def test_oracle_equals_reference_on_boundary_patterns(name, fx):
    probs, _ = G.fixture_boundary_cases()[name]
    assert np.array_equal(probs, fx[f"{name}/probs"]), "generator drifted"
    assert np.array_equal(R.boundary_postprocessing(probs), fx[f"{name}/labels"])


def test_fixture_is_small_and_holds_arrays_only(golden_dir):
    assert (golden_dir / "postproc_geometry.npz").stat().st_size < (golden_dir / "postproc_distance_256.npz").stat().st_size
    with np.load(golden_dir / "postproc_geometry.npz", allow_pickle=False) as f:
        assert all(f[k].dtype in (np.float32, np.float64, np.uint16) for k in f.files)


# ---- the oracle's host entry keeps one-row and one-column frames two-dimensional -----------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (1, 64), (65, 1)])
def test_oracle_accepts_frames_of_one_row_or_column(H, W):
    cell, border, f = G.degenerate(H, W, "ones")
    out3 = R.distance_postprocessing(border[..., None], cell[..., None], 0.45, 0.10)
    out2 = R.distance_postprocessing(border, cell, 0.45, 0.10)
    assert out3.shape == out2.shape == (H, W) and R.gaussian05(cell[..., None]).shape == (H, W)
    assert int(out3.max()) == int(out2.max()) == f["n_inst"] == (1 if H * W > 4 else 0)
    assert np.array_equal(out3, np.full((H, W), f["n_inst"], np.uint16))


def test_oracle_answers_for_existing_shapes_are_unchanged():
    for name in ("distance_generic", "distance_small_seeds"):
        g = load_npz(f"postproc_{name}.npz")
        for j, (th_cell, th_seed) in enumerate(g["th"]):
            assert np.array_equal(_oracle(g["cell"], g["border"], th_cell, th_seed), g[f"labels_hw1_{j}"])
            assert np.array_equal(_oracle(g["cell"], g["border"], th_cell, th_seed, False), g[f"labels_2d_{j}"])
    g = load_npz("postproc_gauss_sigma05.npz")
    assert np.array_equal(R.gaussian05(g["x"][..., None]), g["y"]) and np.array_equal(R.gaussian05(g["x"]), g["y2d"])
    assert np.array_equal(R.gaussian05(g["x"][:3, :2].copy()), g["tiny"])


# ---- facts, pattern by pattern ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", G.DEGENERATE_SHAPES)
@pytest.mark.parametrize("kind", G.DEGENERATE_KINDS)
def test_degenerate(H, W, kind):
    cell, border, f = G.degenerate(H, W, kind)
    want = _oracle(cell, border, 0.10, 0.45)
    assert want.shape == (H, W) and int(want.max()) == f["n_inst"]
    n = 0 if kind == "zeros" or H * W <= 4 else 1          # one seed over the whole frame, removed when its area is <= 4
    assert f["n_inst"] == n and np.array_equal(want, np.full((H, W), n, np.uint16))
    probs, fb = G.degenerate_boundary(H, W, kind)
    wb = R.boundary_postprocessing(probs)
    assert wb.shape == (H, W) and int(wb.max()) == fb["n_inst"]
    if kind == "ones":
        assert fb["n_inst"] == (1 if H * W > 4 else 0)


def test_degenerate_known_answers():
    assert G.degenerate(2, 2, "ones")[2]["n_inst"] == 0 and G.degenerate(3, 5, "ones")[2]["n_inst"] == 1


@pytest.mark.parametrize("H,W", G.SCAN_SHAPES)
def test_scan_edges(H, W):
    n = H * W
    assert n in (G.SCAN_TILE - 1, G.SCAN_TILE, G.SCAN_TILE + 1)
    for f in (G.scan_edges(H, W)[2], G.scan_edges_boundary(H, W)[1]):
        assert f["n_kept"] == 2
        assert f["kept_first_px"] == 0 and f["kept_last_px"] == n - 1          # first slot of the first tile, last pixel
        assert f["kept_first_px"] // G.SCAN_TILE == 0 and f["kept_last_px"] // G.SCAN_TILE == (n - 1) // G.SCAN_TILE


@pytest.mark.parametrize("H,W", [(64, 65), (257, 255)])
def test_checkerboard(H, W):
    probs, f = G.checkerboard(H, W)
    mask = probs[..., 1] > 0.5
    assert ndi.label(mask)[1] == -(-H * W // 2) == f["n_mask_comp"]
    assert f["n_seed_comp"] == 1 and f["n_inst"] == 1
    assert np.array_equal(R.boundary_postprocessing(probs), mask.astype(np.uint16))     # label 1 on every black square


WINDING = [("serpentine", 129, 131, 8), ("spiral", 129, 131, 8), ("comb", 129, 131, 10),
           ("serpentine", 255, 257, 8), ("spiral", 255, 257, 8), ("comb", 255, 257, 8)]
PPW_TILE_L = 30720


@pytest.mark.parametrize("kind,H,W,pitch", WINDING)
@pytest.mark.parametrize("ramped", [False, True])
def test_winding_distance(kind, H, W, pitch, ramped):
    cell, border, f = G.winding_distance(kind, H, W, pitch, ramped)
    assert f["n_mask_comp"] == 1 and f["box_is_frame"] == [True]
    assert f["n_inst"] == 2 and f["max_inst_per_comp"] == 2              # a seed at each end: labels meet inside the component
    assert f["mask_area"] < 3.5 * H * W / pitch                           # 3 px thick after the smoothing
    assert ((H + 2) * (W + 2) > PPW_TILE_L) == (H > 200)                  # the larger size probes global memory by default
    assert (f["marker_ties"] == 0) == ramped
    want = _oracle(cell, border, 0.10, 0.45)
    assert set(np.unique(want)) == {0, 1, 2}


@pytest.mark.parametrize("kind,H,W", [("serpentine", 129, 131), ("spiral", 129, 131), ("comb", 129, 131),
                                      ("serpentine", 255, 257), ("serpentine", 64, 65), ("comb", 64, 65)])
def test_winding_boundary(kind, H, W):
    probs, f = G.winding_boundary(kind, H, W, 2)
    assert f["n_mask_comp"] == 1 and f["box_is_frame"] == [True] and f["n_inst"] == 2 and f["max_inst_per_comp"] == 2
    assert abs(f["mask_area"] - H * W / 2) < H + W                        # a line on every second row: n / pitch
    assert set(np.unique(R.boundary_postprocessing(probs))) == {0, 1, 2}


@pytest.mark.parametrize("H,W,pitch,r,n", [(61, 67, 12, 8, 30), (120, 130, 10, 7, 156)])
def test_lattice(H, W, pitch, r, n):
    cell, border, f = G.lattice(H, W, pitch, r)
    assert f["n_mask_comp"] == 1 and f["n_inst"] == n == f["max_inst_per_comp"]
    # cells whose centre is not within the smoothing's reach of the frame edge hold bit-identical values
    maxima = [np.float32(m).tobytes() for m in f["seed_max"]]
    assert max(maxima.count(m) for m in set(maxima)) >= n - max(H // pitch, W // pitch) - 1
    assert f["marker_ties"] > n
    assert int(_oracle(cell, border, 0.10, 0.45).max()) == n


@pytest.mark.parametrize("axis", G.MIRROR_AXES)
def test_mirror_pair(axis):
    cell, border, f = G.mirror_pair(axis)
    assert cell.shape == (40, 48) and f["n_mask_comp"] == 1 and f["n_inst"] == 2
    assert 2 <= f["seed_gap"] <= 6
    a, b = f["seed_max"]
    assert np.float32(a).tobytes() == np.float32(b).tobytes(), "the two seeds' maxima must be bit-equal"
    assert f["seed_areas"][0] == f["seed_areas"][1]


def test_plateau_and_terraces():
    cell, border, f = G.plateau()
    assert cell.shape == (46, 56) and f["n_mask_comp"] == 1 and f["box_is_frame"] == [True] and f["n_inst"] == 1
    assert len(np.unique(cell)) == 2
    assert (_oracle(cell, border, 0.10, 0.45) == 1).all()
    cell, border, f = G.terraces()
    assert f["n_mask_comp"] == 1 and f["n_inst"] == 6 and len(np.unique(cell)) == 2 and f["marker_ties"] > 6
    assert len({np.float32(m).tobytes() for m in f["seed_max"]}) == 1


@pytest.mark.parametrize("ramped", [False, True])
def test_disk_one_seed(ramped):
    cell, border, f = G.disk_one_seed(ramped=ramped)
    assert cell.shape == (200, 200) and f["n_mask_comp"] == 1 and f["n_seed_comp"] == 1 and f["n_inst"] == 1
    assert f["mask_area"] > 3.1 * 90 * 90
    assert (f["marker_ties"] == 0) == ramped


@pytest.fixture(scope="module")
def many():
    cell, border, f = G.many_instances()
    probs, fb = G.many_instances_boundary()
    return cell, border, f, probs


def test_many_instances(many):
    cell, border, f, probs = many
    assert cell.shape == (1028, 1024) and f["n_squares"] == 65792 == ndi.label(cell > 0)[1]
    assert f["scan_tiles"] == 514 > 256                                    # a second trip of the block-sum kernel
    for want in (_oracle(cell, border, *G.MANY_TH), R.boundary_postprocessing(probs)):
        assert int(want.max()) == 65535 and len(np.unique(want)) == 65536
        assert int(((want == 0) & (cell > 0)).sum()) == 9                  # exactly one square wraps to 0
        assert not want[cell == 0].any()


@pytest.mark.parametrize("H,diagonal", G.SEPARATOR_CASES)
def test_separator(H, diagonal):
    cell, border, f = G.separator(H, diagonal)
    assert cell.shape == (3, H, 66)
    assert f["merged_differs"], "a tall image without the separator row must give other labels"
    cs = [R.gaussian05(c) for c in cell]
    half = 33 if diagonal else 66
    for k in range(2):                                                      # facing rows are foreground
        assert (cs[k][H - 1, :half - 1] > 0.10).all() and (cs[k + 1][0, 66 - half + 1:] > 0.10).all()


# ---- label images ----------------------------------------------------------------------------------------------------------------
def test_label_shapes():
    for name, (m, f) in G.label_shapes().items():
        lab = eval_ref.label_image(m)
        assert int(lab.max()) == f["n_labels"], name
    m = G.border_shapes()
    counts = [int(eval_ref.label_image(eval_ref.border_correction(m, bw)).max()) for bw in (0, 3, 10)]
    assert counts[0] > counts[1] > counts[2] >= 1, counts
    frames = G.stack_shapes()
    assert frames.shape[0] == 3 and (frames[:-1, -1] == frames[1:, 0]).all() and (frames[:, 0] > 0).all()
    tall = eval_ref.label_image(frames.reshape(-1, frames.shape[2]))
    per = sum(int(eval_ref.label_image(fr).max()) for fr in frames)
    assert int(tall.max()) < per                                             # facing rows would merge across frames


@pytest.mark.parametrize("width", [1, 2])
def test_cell_masks_for_label_creation(width):
    from oracle import labels_ref
    for m, winding in ((G.two_cells_winding_gap(width), True), (G.comb_cells(width), False)):
        assert m.shape == (96, 112) and set(np.unique(m)) == {0, 1, 2}
        assert ndi.label(m == 1)[1] == 1 and ndi.label(m == 2)[1] == 1
        assert not (ndi.binary_dilation(m == 1, structure=G.S8) & (m == 2)).any()          # the gap separates them everywhere
        comp, weight = labels_ref.bottom_hat_closing(m)
        sizes = np.bincount(comp.ravel())[1:]
        if winding:
            assert sizes.max() >= 100 * width, "one long gap component between the two cells"
        else:
            assert sizes.sum() >= 300, "the gap between the combs is closed: 13 teeth of 56 rows"


# ---- ties between labels only; a run of equal roots across a row end -----------------------------------------------------------------
@pytest.mark.parametrize("axis", G.MIRROR_AXES)
def test_ramped_mirror_pair_ties_only_across_the_two_seeds(axis):
    cell, border, f = G.mirror_pair(axis, ramped=True)
    assert f["n_mask_comp"] == 1 and f["n_inst"] == 2 and f["seed_areas"][0] == f["seed_areas"][1]
    assert f["marker_ties"] == f["seed_areas"][0], "each marker ties with its mirror image and with nothing else"
    a, b = f["seed_max"]
    assert np.float32(a).tobytes() == np.float32(b).tobytes()


def test_ramped_lattice_ties_only_across_cells():
    cell, border, f = G.lattice(61, 67, 12, 8, ramped=True)
    assert f["n_mask_comp"] == 1 and f["n_inst"] == 30
    cs = R.gaussian05(cell)
    seeds, k = ndi.label(cs > np.float32(0.45), structure=G.S8)
    assert k == 30 and all(len(np.unique(cs[seeds == i])) == (seeds == i).sum() for i in range(1, k + 1))
    assert f["marker_ties"] > 30


def test_row_wrap():
    cell, border, f = G.row_wrap()
    H, W = cell.shape
    assert W < 64 and f["n_inst"] == 2 and f["n_mask_comp"] == 1
    seeds = ndi.label(R.gaussian05(cell) > np.float32(0.45), structure=G.S8)[0]
    big = seeds == seeds[4, 0]
    flat = big.ravel()
    wraps = [y for y in range(1, H) if flat[y * W - 1] and flat[y * W]]          # a run of the seed continues across a row end
    ys, xs = np.nonzero(big)
    first_raster = (ys[0], xs[0])
    first_colmajor = min(zip(xs, ys))
    assert wraps and first_raster[1] > 0 and first_colmajor[0] == 0             # the two orders name different first pixels
    other = np.nonzero((seeds > 0) & ~big)
    key = lambda y, x: x * H + y
    assert key(first_colmajor[1], 0) < key(other[0][0], other[1].min()) < key(*first_raster)
    probs, fb = G.row_wrap_boundary()
    assert fb["n_inst"] == 2 and fb["n_mask_comp"] == 2
