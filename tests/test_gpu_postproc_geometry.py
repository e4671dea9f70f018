"""GPU (MI355X): post-processing, relabelling and label creation on the structured worst-case frames of tests/geometry_ref.py
— serpentines, spirals, combs, tied lattices, mirror pairs, plateaus, checkerboards, 65 792 instances, frames of one pixel —
bit for bit against the C oracle (and the reference's own answers, tests/golden/postproc_geometry.npz, where they exist).
No tolerance anywhere, except the module's existing DTOL for the two distance-label images.

What the patterns drove on an MI355X (status words, rule bits, durations): DESIGN.md, section "Structured worst-case frames"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import geometry_ref as G
from helpers import load_npz
from oracle import eval_ref, labels_ref, postproc_ref as R
from test_gpu_cells import Guarded

pytestmark = pytest.mark.gpu
TUNINGS = [(1, -1, -1), (16, 0, 0), (1, 0, 0), (2, 400, 2000), (16, 0, -1)]      # of test_component_flood_paths_agree


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from microbeseg_amd.inference import postprocessing
    return postprocessing


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(pp):
    """a HIP error after a test (a faulted kernel) ends the session: nothing more is started on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, stopping: {e}", returncode=3)


@pytest.fixture(scope="module")
def lib(pp):
    from microbeseg_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def fx():
    return load_npz("postproc_geometry.npz")


@pytest.fixture(params=[1, 0], ids=["marker_phase_closed_form", "marker_phase_heap_replay"])
def const_stream(request, lib):
    """both marker phases of the constant-image flood, as in tests/test_gpu_postproc.py"""
    assert lib.mseg_postproc_set_const_stream(request.param) == 0
    yield request.param
    lib.mseg_postproc_set_const_stream(1)


# ---- the distance patterns ---------------------------------------------------------------------------------------------------------
DISTANCE = {
    "scan_edges_23x89": lambda: G.scan_edges(23, 89),
    "scan_edges_32x64": lambda: G.scan_edges(32, 64),
    "scan_edges_3x683": lambda: G.scan_edges(3, 683),
    "serpentine_129x131": lambda: G.winding_distance("serpentine", 129, 131, 8),
    "spiral_129x131": lambda: G.winding_distance("spiral", 129, 131, 8),
    "comb_129x131": lambda: G.winding_distance("comb", 129, 131, 10),
    "serpentine_255x257": lambda: G.winding_distance("serpentine", 255, 257, 8),
    "spiral_255x257": lambda: G.winding_distance("spiral", 255, 257, 8),
    "comb_255x257": lambda: G.winding_distance("comb", 255, 257, 8),
    "serpentine_129x131_ramp": lambda: G.winding_distance("serpentine", 129, 131, 8, True),
    "serpentine_255x257_ramp": lambda: G.winding_distance("serpentine", 255, 257, 8, True),
    "spiral_255x257_ramp": lambda: G.winding_distance("spiral", 255, 257, 8, True),
    "comb_129x131_ramp": lambda: G.winding_distance("comb", 129, 131, 10, True),
    "lattice_61x67": lambda: G.lattice(61, 67, 12, 8),
    "lattice_120x130": lambda: G.lattice(120, 130, 10, 7),
    "mirror_vertical": lambda: G.mirror_pair("vertical"),
    "mirror_horizontal": lambda: G.mirror_pair("horizontal"),
    "mirror_point": lambda: G.mirror_pair("point"),
    "plateau": G.plateau,
    "terraces": G.terraces,
    "disk_one_seed": G.disk_one_seed,
    "disk_one_seed_ramp": lambda: G.disk_one_seed(ramped=True),
    "serpentine_65x70": lambda: G.winding_distance("serpentine", 65, 70, 8),
    "lattice_61x67_ramp": lambda: G.lattice(61, 67, 12, 8, True),
    "mirror_vertical_ramp": lambda: G.mirror_pair("vertical", ramped=True),
    "mirror_horizontal_ramp": lambda: G.mirror_pair("horizontal", ramped=True),
    "mirror_point_ramp": lambda: G.mirror_pair("point", ramped=True),
    "row_wrap_12x40": G.row_wrap,
}
TIE_FREE = ["serpentine_129x131_ramp", "serpentine_255x257_ramp", "disk_one_seed_ramp"]
TIED = ["lattice_61x67", "lattice_120x130", "mirror_vertical", "mirror_horizontal", "mirror_point", "plateau", "terraces",
        "lattice_61x67_ramp", "mirror_vertical_ramp", "mirror_horizontal_ramp", "mirror_point_ramp"]
FIXTURE = ["lattice_61x67", "lattice_120x130", "serpentine_65x70", "plateau", "mirror_vertical", "mirror_horizontal",
           "mirror_point"]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (cell, border, {(th_cell, th_seed): (oracle (H, W, 1) ids, oracle (H, W) ids, host facts)}), computed once"""
    cell, border, _ = DISTANCE[name]()
    want = {}
    for th_cell, th_seed in G.THS:
        want[(th_cell, th_seed)] = (R.distance_postprocessing(border[..., None], cell[..., None], th_seed, th_cell),
                                    R.distance_postprocessing(border, cell, th_seed, th_cell),
                                    G.distance_facts(cell, border, th_cell, th_seed))
    for a in (cell, border):
        a.setflags(write=False)
    return cell, border, want


def device_call(pp, cell, border, th_cell, th_seed, col_major=True):
    c, b = torch.from_numpy(cell).cuda(), torch.from_numpy(border).cuda()
    labels, n_inst, status = pp.distance_postprocessing_device(b, c, th_seed, th_cell, col_major_ids=col_major)
    return labels.cpu().numpy().view(np.uint16), int(n_inst), int(status)


def words(status):
    return f"status {status & 3} rules(3,3a,2b,2a,1) {(status >> 8) & 31:05b}"


def gapless(labels, n):
    ids = np.unique(labels)
    return np.array_equal(ids[ids > 0], np.arange(1, n + 1))


@pytest.mark.parametrize("name", list(DISTANCE))
def test_distance_pattern_equals_oracle(name, pp, fx):
    cell, border, want = case(name)
    for j, ((th_cell, th_seed), (hw1, flat, facts)) in enumerate(want.items()):
        for col_major, oracle in ((True, hw1), (False, flat)):
            got, n_inst, status = device_call(pp, cell, border, th_cell, th_seed, col_major)
            print(name, (th_cell, th_seed), "col_major", col_major, "instances", n_inst, words(status))
            assert np.array_equal(got, oracle), f"{(got != oracle).sum()} px differ, {words(status)}"
            assert n_inst == facts["n_inst"] == int(oracle.max()) and gapless(got, n_inst)
        assert np.array_equal(pp.distance_postprocessing(border[..., None], cell[..., None], th_seed=th_seed,
                                                         th_cell=th_cell), hw1)
        assert np.array_equal(pp.distance_postprocessing(border, cell, th_seed=th_seed, th_cell=th_cell), flat)
        if name in FIXTURE:                                    # the reference's own answer
            assert np.array_equal(hw1, fx[f"{name}/labels_hw1_{j}"]) and np.array_equal(flat, fx[f"{name}/labels_2d_{j}"])


@pytest.mark.parametrize("name", TIE_FREE)
def test_tie_free_patterns_stay_on_the_component_flood(name, pp):
    cell, border, want = case(name)
    th_cell, th_seed = G.THS[0]
    hw1, _, facts = want[G.THS[0]]
    assert facts["marker_ties"] == 0 and facts["n_mask_comp"] == 1
    got, _, status = device_call(pp, cell, border, th_cell, th_seed)
    print(name, words(status))
    assert np.array_equal(got, hw1)
    assert status & 1 == 0, f"no two markers are equal, yet the frame was redone serially: {words(status)}"


def test_tied_patterns_are_exact_whichever_path_they_take(pp):
    serial = 0
    for name in TIED:
        cell, border, want = case(name)
        for (th_cell, th_seed), (hw1, _, facts) in want.items():
            got, _, status = device_call(pp, cell, border, th_cell, th_seed)
            print(name, (th_cell, th_seed), "tied markers", facts["marker_ties"], words(status))
            assert np.array_equal(got, hw1), f"{name} {(th_cell, th_seed)}: {(got != hw1).sum()} px differ, {words(status)}"
            serial += status & 1
    assert serial >= 1, "no tied frame was sent to the exact serial flood"


@pytest.mark.parametrize("col_major", [True, False])
def test_many_instances_wrap_like_uint16(col_major, pp):
    """65 792 instances: ids above 65 535 wrap (astype(np.uint16)), exactly one square becomes 0; 514 tiles of the prefix sum.
    (The nine equal markers of a square are a chain of ties, so the frame is redone by the serial flood: 2.5 s.)"""
    cell, border, facts = G.many_instances()
    th_cell, th_seed = G.MANY_TH
    inp = (border[..., None], cell[..., None]) if col_major else (border, cell)
    want = R.distance_postprocessing(*inp, th_seed, th_cell)
    got, n_inst, status = device_call(pp, cell, border, th_cell, th_seed, col_major)
    print("many_instances col_major", col_major, n_inst, words(status))
    assert n_inst == facts["n_squares"] == 65792
    assert np.array_equal(got, want), f"{(got != want).sum()} px differ"
    assert int(got.max()) == 65535 and int(((got == 0) & (cell > 0)).sum()) == 9


# ---- the boundary patterns -----------------------------------------------------------------------------------------------------------
BOUNDARY = {
    "scan_edges_23x89": lambda: G.scan_edges_boundary(23, 89),
    "scan_edges_32x64": lambda: G.scan_edges_boundary(32, 64),
    "scan_edges_3x683": lambda: G.scan_edges_boundary(3, 683),
    "checkerboard_64x65": lambda: G.checkerboard(64, 65),
    "checkerboard_257x255": lambda: G.checkerboard(257, 255),
    "serpentine_129x131": lambda: G.winding_boundary("serpentine", 129, 131, 2),
    "spiral_129x131": lambda: G.winding_boundary("spiral", 129, 131, 2),
    "comb_129x131": lambda: G.winding_boundary("comb", 129, 131, 2),
    "serpentine_255x257": lambda: G.winding_boundary("serpentine", 255, 257, 2),
    "many_instances": G.many_instances_boundary,
    "row_wrap_12x40": G.row_wrap_boundary,
}


@functools.lru_cache(maxsize=None)
def bcase(name):
    probs, facts = BOUNDARY[name]()
    probs.setflags(write=False)
    return probs, facts, R.boundary_postprocessing(probs)


@pytest.mark.parametrize("name", list(BOUNDARY))
def test_boundary_pattern_equals_oracle(name, pp, fx, const_stream):
    probs, facts, want = bcase(name)
    labels, n_inst, status = pp.boundary_postprocessing_device(torch.from_numpy(probs).cuda())
    got = labels.cpu().numpy().view(np.uint16)
    print(name, "instances", int(n_inst), words(int(status)))
    assert np.array_equal(got, want), f"{(got != want).sum()} px differ"
    if name == "many_instances":
        assert int(n_inst) == facts["n_squares"] == 65792 and int(((got == 0) & (probs[..., 1] > 0.5)).sum()) == 9
    else:
        assert int(n_inst) == facts["n_inst"] == int(want.max()) and gapless(got, int(n_inst))
    if f"{name}/labels" in fx:
        assert np.array_equal(want, fx[f"{name}/labels"])
    if name.startswith("checkerboard"):
        assert np.array_equal(got, (probs[..., 1] > 0.5).astype(np.uint16))           # label 1 on every black square
    assert np.array_equal(pp.boundary_postprocessing(probs), want)


# ---- degenerate sizes and the separator row, through the C ABI with guard words --------------------------------------------------------
class GuardedLabels:
    """n uint16 labels inside an int32 buffer between guard bands; an odd n leaves half a sentinel word behind the labels"""

    def __init__(self, n):
        self.n, self.g = n, Guarded(((n + 1) // 2,), torch.int32)
        self.ptr = self.g.ptr

    def host(self, shape):
        h = self.g.host(np.int32).view(np.uint16)
        assert self.n % 2 == 0 or h[-1] == 0x5A5A, "the half word behind the labels was written"
        return h[:self.n].reshape(shape).copy()


class Workspace:
    def __init__(self, need):
        assert need > 0
        self.need, self.t = need, torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")

    def check(self):
        assert bool((self.t[self.need:] == 0xA5).all()), "written behind the workspace"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_distance(lib, cell, border, th_cell, th_seed, col_major):
    H, W = cell.shape
    ws = Workspace(lib.mseg_postproc_workspace_bytes(H, W))
    c, b = torch.from_numpy(cell).cuda(), torch.from_numpy(border).cuda()
    lab, n, st = GuardedLabels(H * W), Guarded((1,), torch.int32), Guarded((1,), torch.int32)
    rc = lib.mseg_distance_postprocess(b.data_ptr(), c.data_ptr(), H, W, th_cell, th_seed, int(col_major), lab.ptr, n.ptr,
                                       st.ptr, ws.t.data_ptr(), ws.need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ws.check()
    return lab.host((H, W)), int(n.host(np.int32)[0]), int(st.host(np.int32)[0])


def c_boundary(lib, probs):
    H, W, _ = probs.shape
    ws = Workspace(lib.mseg_postproc_workspace_bytes(H, W))
    p = torch.from_numpy(probs).cuda()
    lab, n, st = GuardedLabels(H * W), Guarded((1,), torch.int32), Guarded((1,), torch.int32)
    rc = lib.mseg_boundary_postprocess(p.data_ptr(), H, W, lab.ptr, n.ptr, st.ptr, ws.t.data_ptr(), ws.need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ws.check()
    return lab.host((H, W)), int(n.host(np.int32)[0]), int(st.host(np.int32)[0])


def c_distance_group(lib, cell, border, th_cell, th_seed, col_major):
    N, H, W = cell.shape
    ws = Workspace(lib.mseg_postproc_batch_workspace_bytes(N, H, W))
    c, b = torch.from_numpy(cell).cuda(), torch.from_numpy(border).cuda()
    lab, n, st = GuardedLabels(N * H * W), Guarded((N,), torch.int32), Guarded((N,), torch.int32)
    rc = lib.mseg_distance_postprocess_batch(b.data_ptr(), c.data_ptr(), N, H, W, W, H * W, th_cell, th_seed, int(col_major),
                                             lab.ptr, n.ptr, st.ptr, ws.t.data_ptr(), ws.need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ws.check()
    return lab.host((N, H, W)), n.host(np.int32).copy(), st.host(np.int32).copy()


@pytest.mark.parametrize("H,W", G.DEGENERATE_SHAPES)
def test_degenerate_sizes(H, W, lib):
    """frames smaller than the gaussian's reach, narrower than a wavefront, one block: all ones, all zeros and a ramp through
    both methods; nothing but the outputs is written"""
    for kind in G.DEGENERATE_KINDS:
        cell, border, facts = G.degenerate(H, W, kind)
        for th_cell, th_seed in G.THS:
            for col_major in (1, 0):
                inp = (border[..., None], cell[..., None]) if col_major else (border, cell)
                want = R.distance_postprocessing(*inp, th_seed, th_cell)
                got, n_inst, status = c_distance(lib, cell, border, th_cell, th_seed, col_major)
                assert np.array_equal(got, want), (kind, th_cell, col_major, got.tolist(), want.tolist())
                assert n_inst == int(want.max())
        assert c_distance(lib, cell, border, 0.10, 0.45, 1)[1] == facts["n_inst"]
        probs, bfacts = G.degenerate_boundary(H, W, kind)
        for mode in (1, 0):
            assert lib.mseg_postproc_set_const_stream(mode) == 0
            try:
                got, n_inst, status = c_boundary(lib, probs)
            finally:
                lib.mseg_postproc_set_const_stream(1)
            want = R.boundary_postprocessing(probs)
            assert np.array_equal(got, want), (kind, mode, got.tolist(), want.tolist())
            assert n_inst == bfacts["n_inst"] == int(want.max())
    if (H, W) == (2, 2):
        assert not c_distance(lib, *G.degenerate(2, 2, "ones")[:2], 0.10, 0.45, 1)[0].any()       # area 4 <= 4: no instance
    if (H, W) == (3, 5):
        assert (c_distance(lib, *G.degenerate(3, 5, "ones")[:2], 0.10, 0.45, 1)[0] == 1).all()


@pytest.mark.parametrize("H,diagonal", G.SEPARATOR_CASES)
def test_separator_row_keeps_frames_apart(H, diagonal, lib):
    """foreground on the last row of frame k and the first row of frame k + 1: the group entry must answer frame by frame"""
    cell, border, facts = G.separator(H, diagonal)
    assert facts["merged_differs"]
    for col_major in (1, 0):
        got, n_inst, status = c_distance_group(lib, cell, border, 0.10, 0.45, col_major)
        print("separator", H, diagonal, "col_major", col_major, n_inst.tolist(), [words(int(s)) for s in status])
        for k in range(cell.shape[0]):
            inp = (border[k][..., None], cell[k][..., None]) if col_major else (border[k], cell[k])
            want = R.distance_postprocessing(*inp, 0.45, 0.10)
            single = c_distance(lib, cell[k], border[k], 0.10, 0.45, col_major)
            assert np.array_equal(got[k], want), f"frame {k}: {got[k].tolist()} != {want.tolist()}"
            assert np.array_equal(got[k], single[0]) and (int(n_inst[k]), int(status[k])) == single[1:]
            assert int(n_inst[k]) == facts["n_inst"][k] == int(want.max())                     # ids restart at 1


# ---- group entries ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_group():
    H, W = 61, 67
    cells = [G.lattice(H, W, 12, 8)[0], G.winding_distance("serpentine", H, W, 6)[0], np.zeros((H, W), np.float32),
             np.ones((H, W), np.float32), G.plateau(H, W)[0]]
    cell = np.stack(cells)
    border = np.zeros_like(cell)
    want = {(cm, th): [R.distance_postprocessing(*((b[..., None], c[..., None]) if cm else (b, c)), th[1], th[0])
                       for c, b in zip(cell, border)] for cm in (True, False) for th in G.THS}
    return cell, border, want


def _check_group(pp, cell_d, border_d, cell, border, want, pads=(0, 0)):
    for (col_major, (th_cell, th_seed)), oracle in want.items():
        labels, n_inst, status = pp.distance_postprocessing_batch_device(border_d, cell_d, th_seed, th_cell, pads=pads,
                                                                         col_major_ids=col_major)
        got = labels.cpu().numpy().view(np.uint16)
        for i in range(got.shape[0]):
            single = device_call(pp, cell[i], border[i], th_cell, th_seed, col_major)
            where = f"frame {i}, col_major {col_major}, ths {(th_cell, th_seed)}"
            assert np.array_equal(got[i], oracle[i]), f"{where}: {(got[i] != oracle[i]).sum()} px differ from the oracle"
            assert np.array_equal(got[i], single[0]), where
            assert (int(n_inst[i]), int(status[i])) == single[1:], where
            assert gapless(got[i], int(n_inst[i])), where                                       # ids restart at 1
        print("group", col_major, (th_cell, th_seed), n_inst.tolist(), [words(int(s)) for s in status])


def test_mixed_group_equals_single_frames_and_oracle(pp):
    cell, border, want = mixed_group()
    c, b = torch.from_numpy(cell).cuda(), torch.from_numpy(border).cuda()
    _check_group(pp, c, b, cell, border, want)
    for i in range(len(cell)):                                                                  # N = 1
        _check_group(pp, c[i:i + 1], b[i:i + 1], cell[i:i + 1], border[i:i + 1], {k: v[i:i + 1] for k, v in want.items()})


def test_mixed_group_reads_padded_predictions_in_place(pp):
    cell, border, want = mixed_group()
    N, H, W = cell.shape
    pt, pl = 32, 56
    cp = torch.full((N, 1, H + pt, W + pl), 5.0, device="cuda")
    bp = torch.full((N, 1, H + pt, W + pl), -3.0, device="cuda")
    cp[:, 0, pt:, pl:] = torch.from_numpy(cell).cuda()
    bp[:, 0, pt:, pl:] = torch.from_numpy(border).cuda()
    _check_group(pp, cp[:, 0], bp[:, 0], cell, border, want, pads=(pt, pl))


def test_boundary_batch_of_patterns_equals_single_frames(pp, const_stream):
    H, W = 64, 65
    yy, xx = np.mgrid[0:H, 0:W]
    frames = [G.checkerboard(H, W)[0], G.winding_boundary("serpentine", H, W, 2)[0], G.winding_boundary("comb", H, W, 2)[0],
              G.boundary_probs(np.zeros((H, W), bool)), G.boundary_probs(np.ones((H, W), bool)),
              G.winding_boundary("spiral", H, W, 2)[0], G.scan_edges_boundary(H, W)[0], G.boundary_probs((yy // 4 + xx // 4) % 2 == 0)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    single = [(l.cpu().numpy().copy(), int(n), int(s)) for l, n, s in (pp.boundary_postprocessing_device(f) for f in dev)]
    for f, s in zip(frames, single):
        assert np.array_equal(s[0].view(np.uint16), R.boundary_postprocessing(f))
    for B in (8, 3):
        for start in range(0, 8, B):
            got = pp.boundary_postprocessing_batch_device(dev[start:start + B], first_slot=2)
            for k, (l, n, s) in enumerate(got):
                assert np.array_equal(l.cpu().numpy(), single[start + k][0]), (B, start + k)
                assert (int(n), int(s)) == single[start + k][1:], (B, start + k)


# ---- tuned paths, threshold sweep --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,tile_s,tile_l", TUNINGS)
def test_patterns_through_the_tuned_flood_paths(rows, tile_s, tile_l, pp, lib):
    """one LDS row (spill), no tile at all (global probes), small tiles: the queue as long as a disk's perimeter, a component
    whose box is the frame, 156 tied cells in one component"""
    assert lib.mseg_postproc_tuning(rows, tile_s, tile_l) == 0
    try:
        for name in ("disk_one_seed", "disk_one_seed_ramp", "serpentine_255x257", "serpentine_255x257_ramp", "lattice_120x130"):
            cell, border, want = case(name)
            for (th_cell, th_seed), (hw1, _, facts) in want.items():
                got, n_inst, status = device_call(pp, cell, border, th_cell, th_seed)
                print(name, (rows, tile_s, tile_l), (th_cell, th_seed), words(status))
                assert np.array_equal(got, hw1), f"{name} {(th_cell, th_seed)}: {(got != hw1).sum()} px differ, {words(status)}"
                if facts["marker_ties"] == 0:
                    assert status & 1 == 0
    finally:
        assert lib.mseg_postproc_tuning(-1, -1, -1) == 0


@pytest.mark.parametrize("name", ["lattice_61x67", "lattice_120x130", "serpentine_129x131", "serpentine_255x257_ramp"])
def test_threshold_sweep_equals_single_calls(name, pp):
    cell, border, _ = case(name)
    ths = list(G.THS) + [(0.125, 0.45), (0.05, 0.35)]
    c, b = torch.from_numpy(cell).cuda(), torch.from_numpy(border).cuda()
    labels, n_inst, status = pp.distance_postprocessing_sweep_device(b, c, ths)
    got = labels.cpu().numpy().view(np.uint16)
    for i, (th_cell, th_seed) in enumerate(ths):
        single = device_call(pp, cell, border, th_cell, th_seed)
        assert np.array_equal(got[i], single[0]) and (int(n_inst[i]), int(status[i])) == single[1:], (name, ths[i])
        assert np.array_equal(got[i], R.distance_postprocessing(border[..., None], cell[..., None], th_seed, th_cell))


# ---- relabelling ------------------------------------------------------------------------------------------------------------------------
def _relabel_ref(m, bw):
    return eval_ref.label_image(eval_ref.border_correction(m, bw) if bw > 0 else m)


@pytest.mark.parametrize("name", ["one_id_two_pieces", "two_ids_adjacent", "same_id_diagonal", "checkerboard_two_ids", "serpentine"])
@pytest.mark.parametrize("bw", [0, 3, 10])
def test_eval_relabel_on_label_shapes(name, bw, pp):
    from microbeseg_amd.evaluation import stats_utils
    m, facts = G.label_shapes()[name]
    want = _relabel_ref(m, bw)
    lab, k = stats_utils.relabel_device(m, border_width=bw)
    assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), want)
    assert k == int(want.max())
    if bw == 0 or name in ("checkerboard_two_ids", "serpentine"):
        assert k == facts["n_labels"]


@pytest.mark.parametrize("bw", [0, 3, 10])
def test_eval_relabel_border_correction_around_a_serpentine(bw, pp):
    from microbeseg_amd.evaluation import stats_utils
    m = G.border_shapes()
    want = _relabel_ref(m, bw)
    lab, k = stats_utils.relabel_device(m, border_width=bw)
    assert np.array_equal(lab.cpu().numpy(), want) and k == int(want.max())


def test_eval_relabel_many_instances_do_not_wrap(pp):
    from microbeseg_amd.evaluation import stats_utils
    m = G.many_squares().astype(np.uint16)
    lab, k = stats_utils.relabel_device(m, border_width=0)
    got = lab.cpu().numpy()
    assert k == 65792 == int(got.max())
    assert np.array_equal(got, eval_ref.label_image(m))


@pytest.mark.parametrize("dtype", [np.uint16, np.int32], ids=["MSEG_PIX_U16", "MSEG_PIX_I32"])
def test_stack_relabel_frame_by_frame(dtype, pp):
    """T = 3, frame t's last row and frame t + 1's first row carry the same value: components must not cross frames"""
    from microbeseg_amd.inference import analysis
    frames = G.stack_shapes().astype(dtype)
    dev = torch.from_numpy(frames.view(np.int16) if dtype == np.uint16 else frames).cuda()
    lab, k = analysis.relabel_stack(dev)
    lab, k = lab.cpu().numpy(), k.cpu().numpy()
    for t in range(frames.shape[0]):
        want = eval_ref.label_image(frames[t])
        assert np.array_equal(lab[t], want), f"frame {t}: {(lab[t] != want).sum()} px differ"
        assert int(k[t]) == int(want.max())


# ---- label creation (csrc/labels.hip) on structured cell masks ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["winding_gap", "comb"])
@pytest.mark.parametrize("width", [1, 2])
def test_label_creation_on_long_gaps(shape, width, pp):
    from microbeseg_amd.training import train_data_representations as T
    from test_labels import DTOL
    m = G.two_cells_winding_gap(width) if shape == "winding_gap" else G.comb_cells(width)
    closed, corr = T.bottom_hat_closing(m)
    comp, weight = labels_ref.bottom_hat_closing(m)
    assert np.array_equal(closed, comp) and np.array_equal(corr, weight)
    cell, nb = T.distance_label(m, 60)
    c, d = labels_ref.distance_label(m, 60)
    assert np.abs(cell - c).max() <= DTOL and np.abs(nb - d).max() <= DTOL
    assert np.array_equal(T.j4_label(m), labels_ref.j4_label(m))
