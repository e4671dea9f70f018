"""GPU (MI355X): label creation (csrc/labels.hip, label_boundary_kernel of csrc/augment.hip) on the structured worst-case masks
of tests/labels_cases.py against oracle/labels_ref.py: distance maps within the module's existing 1e-6, every integer label
bit for bit.  Batches through the C ABI (N = 3 planes must equal three N = 1 calls), workspace hygiene (0xFF-filled
against zeroed), determinism, the whole-window contract and the argument errors.

tests/test_labels_structured_host.py shows on the CPU which fixture notices which wrong decision.  The last test prints the
largest difference to the oracle per entry point."""
import functools

import numpy as np
import pytest
import torch

import labels_cases as LC
from oracle import labels_ref

pytestmark = pytest.mark.gpu
DTOL = 1e-6                                        # tests/test_labels.py
NAMES = sorted(LC.CASES)
J4_PARAMS = ((0, 1), (2, 4), (16, 16), (1, 16))
GUARD = 256                                        # bytes on either side of every output
EINVAL, EWORKSPACE = -1, -3                        # include/mseg_hip.h
WORST = {}                                         # entry point -> (largest |device - oracle|, fixture)
SAME_SHAPE = (("edge_x1_in", "edge_y0_out", "partial_neighbour"),        # 24 x 24, ids 1 and 2 in each
              ("comb_same_rows", "comb_transposed", "comb_rows_away"))      # 64 x 64, ids 1 and 2 in each
HYGIENE = ("ring_gap", "diagonal_gap", "seven_ids", "frame_whole", "near_left", "gap_g3_l30_t8", "tiny_1x9", "tiny_7x7")


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from microbeseg_amd.training import train_data_representations
    return train_data_representations


@pytest.fixture(scope="module")
def lib(T):
    from microbeseg_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(T):
    """a HIP error after a test (a faulted kernel) ends the session: nothing more is started on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, stopping: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def want(name):
    """the oracle's answers for one fixture, computed once and frozen"""
    mask, sr = LC.CASES[name]
    cell, nb = labels_ref.distance_label(mask, sr)
    comp, weight = labels_ref.bottom_hat_closing(mask)
    out = dict(cell=cell, nb=nb, comp=comp, weight=weight, celld=labels_ref.cell_distance_label(mask, sr),
               boundary=labels_ref.boundary_label(mask), border=labels_ref.border_label(mask),
               mal=labels_ref.major_axis_lengths(mask))
    for c in (5, 2):
        out[f"clip{c}"] = labels_ref.cell_distance_label(mask, sr, apply_clipping=True, clip_val=c)
    for k, r in J4_PARAMS:
        out[f"j4_{k}_{r}"] = labels_ref.j4_label(mask, k, r)
    for v in out.values():
        v.setflags(write=False)
    return out


def note(entry, name, got, ref):
    d = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(initial=0.0))
    if entry not in WORST or d > WORST[entry][0]:
        WORST[entry] = (d, name)
    return d


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the Python entry points, every fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_distance_label(T, name):
    mask, sr = LC.CASES[name]
    w = want(name)
    cell, nb = T.distance_label(mask, sr)
    assert cell.dtype == np.float32 and nb.dtype == np.float32 and cell.shape == mask.shape == nb.shape
    dc, dn = note("distance_label: cell map", name, cell, w["cell"]), note("distance_label: neighbour map", name, nb, w["nb"])
    print(f"{name}: cell {dc:.3g} neighbour {dn:.3g}")
    assert dc <= DTOL and dn <= DTOL
    cb, nbb = T.distance_label_batch(np.stack([mask, np.zeros_like(mask), mask]), sr)
    # planes 0 and 2 of a batch = the single call, bit for bit (this is also the second run: determinism)
    for j in (0, 2):
        assert np.array_equal(bits(cb[j]), bits(cell)) and np.array_equal(bits(nbb[j]), bits(nb)), j
    assert not cb[1].any() and not nbb[1].any()    # an empty plane between them stays empty


@pytest.mark.parametrize("name", NAMES)
def test_cell_distance_label(T, name):
    mask, sr = LC.CASES[name]
    w = want(name)
    got = T.cell_distance_label(mask, sr)
    d = note("cell_distance_label", name, got, w["celld"])
    print(f"{name}: plain {d:.3g} bit-identical {np.array_equal(bits(got), bits(w['celld']))}")
    assert got.dtype == np.float32 and d <= DTOL
    for c in (5, 2):
        g = T.cell_distance_label(mask, sr, apply_clipping=True, clip_val=c)
        assert note(f"cell_distance_label clip {c}", name, g, w[f"clip{c}"]) <= DTOL, c
    assert np.array_equal(bits(T.cell_distance_label(mask, sr)), bits(got))


@pytest.mark.parametrize("name", NAMES)
def test_bottom_hat_closing(T, name):
    mask, _ = LC.CASES[name]
    w = want(name)
    closed, corr = T.bottom_hat_closing(mask)
    assert corr.dtype == np.float32
    assert np.array_equal(closed, w["comp"])       # component numbering
    assert np.array_equal(bits(corr), bits(w["weight"]))
    c2, r2 = T.bottom_hat_closing(mask)
    assert np.array_equal(c2, closed) and np.array_equal(bits(r2), bits(corr))


@pytest.mark.parametrize("name", NAMES)
def test_boundary_border_j4(T, name):
    mask, _ = LC.CASES[name]
    w = want(name)
    assert np.array_equal(T.boundary_label(mask), w["boundary"])
    assert np.array_equal(T.border_label(mask), w["border"])
    for k, r in J4_PARAMS:
        got = T.j4_label(mask, k_neighbors=k, se_radius=r)
        assert got.dtype == np.uint8 and np.array_equal(got, w[f"j4_{k}_{r}"]), (k, r)


@pytest.mark.parametrize("name", NAMES)
def test_max_major_axis_length(T, name):
    mask, _ = LC.CASES[name]
    mal = want(name)["mal"]
    ref = float(mal.max()) if mal.size else 0.0
    got = T.max_major_axis_length(mask)
    print(f"{name}: {got!r} vs {ref!r}")
    assert abs(got - ref) <= 1e-9 * ref
    if ref:
        note("max_major_axis_length (relative)", name, np.array(got / ref), np.array(1.0))


def test_major_axis_of_single_pixels_and_lines(T):
    m = np.zeros((9, 11), np.uint16)
    m[1, 1], m[4, 9], m[8, 0] = 1, 65535, 7
    assert T.max_major_axis_length(m) == 0.0       # single pixels only
    m[6, 4] = m[6, 5] = 3
    assert abs(T.max_major_axis_length(m) - 2.0) <= 2e-9            # two pixels: 4 * sqrt(1 / 4)
    n = LC.CASES["small_shapes"][0]
    line = 4 * np.sqrt(2 * (9 * 9 - 1) / 12)                        # 9 pixels on a diagonal
    assert abs(T.max_major_axis_length(n) - line) <= 1e-9 * line


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
class Out:
    """a device output between two guard bands; everything starts as 0xA5 bytes"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.t = torch.full((self.nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD

    def host(self):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + self.nbytes:] == 0xA5).all(), "guard band written"
        return h[GUARD:GUARD + self.nbytes].copy().view(self.dtype).reshape(self.shape)

    def untouched(self):
        return bool((self.t == 0xA5).all())


def dev16(a):
    return torch.from_numpy(np.array(a, dtype=np.uint16, order="C").view(np.int16)).cuda()


def workspace(nbytes, fill):
    return torch.full((max(int(nbytes), 1),), fill, dtype=torch.uint8, device="cuda")


def c_call(lib, entry, masks, sr=0, clip=0.0, k=2, r=4, mode=0, fill=0, ws_short=0):
    """one C entry point on a batch (N, H, W) -> (return code, outputs as Out objects)"""
    masks = np.ascontiguousarray(masks)
    N, H, W = masks.shape
    m = dev16(masks)
    st = torch.cuda.current_stream().cuda_stream
    need = lib.mseg_label_distance_workspace_bytes(N, H, W)
    if entry == "distance":
        ws = workspace(need, fill)
        outs = [Out((N, H, W), np.float32), Out((N, H, W), np.float32)]
        rc = lib.mseg_label_distance(m.data_ptr(), N, H, W, sr, outs[0].ptr, outs[1].ptr, ws.data_ptr(), need - ws_short, st)
    elif entry == "bottom_hat":
        ws = workspace(need, fill)
        outs = [Out((N, H, W), np.int32), Out((N, H, W), np.float32)]
        rc = lib.mseg_label_bottom_hat(m.data_ptr(), N, H, W, outs[0].ptr, outs[1].ptr, ws.data_ptr(), need - ws_short, st)
    elif entry == "cell_distance":
        ws = workspace(need, fill)
        outs = [Out((N, H, W), np.float32)]
        rc = lib.mseg_label_cell_distance(m.data_ptr(), N, H, W, sr, float(clip), outs[0].ptr, ws.data_ptr(), need - ws_short,
                                          st)
    elif entry == "j4":
        ws = workspace(N * H * W, fill)
        outs = [Out((N, H, W), np.uint8)]
        rc = lib.mseg_label_j4(m.data_ptr(), N, H, W, k, r, ws.data_ptr(), outs[0].ptr, st)
    elif entry == "max_major_axis":
        need = lib.mseg_label_major_axis_workspace_bytes(N)
        ws = workspace(need, fill)
        outs = [Out((N,), np.float64)]
        rc = lib.mseg_label_max_major_axis(m.data_ptr(), N, H, W, outs[0].ptr, ws.data_ptr(), need - ws_short, st)
    else:
        assert entry == "boundary"
        outs = [Out((N, H, W), np.uint8)]
        rc = lib.mseg_label_boundary(m.data_ptr(), N, H, W, mode, outs[0].ptr, st)
    torch.cuda.synchronize()
    return rc, outs


ENTRIES = (("distance", {}), ("bottom_hat", {}), ("cell_distance", {}), ("cell_distance", dict(clip=5.0)),
           ("j4", dict(k=2, r=4)), ("j4", dict(k=16, r=16)), ("max_major_axis", {}), ("boundary", dict(mode=0)),
           ("boundary", dict(mode=1)))


@pytest.mark.parametrize("group", range(len(SAME_SHAPE)), ids=["windows_24x24", "combs_64x64"])
@pytest.mark.parametrize("entry,kw", ENTRIES, ids=[e + "".join(f"_{v}" for v in kw.values()) for e, kw in ENTRIES])
def test_batch_of_three_equals_three_single_calls(lib, group, entry, kw):
    """N = 3 through the C ABI (the Python wrappers of these entry points only ever pass N = 1): the per-image table offsets.
    The three masks reuse the same ids, so a table that is shared between the images shows at once."""
    names = SAME_SHAPE[group]
    masks = np.stack([LC.CASES[n][0] for n in names])
    assert all({1, 2} <= set(np.unique(m)) for m in masks) and len({m.tobytes() for m in masks}) == 3
    sr = LC.CASES[names[0]][1]
    rc, batch = c_call(lib, entry, masks, sr=sr, **kw)
    assert rc == 0
    batch = [o.host() for o in batch]
    for j in range(3):
        rc, single = c_call(lib, entry, masks[j:j + 1], sr=sr, **kw)
        assert rc == 0
        for b, s in zip(batch, single):
            assert np.array_equal(bits(b[j]), bits(s.host()[0])), (names[j], j)
    if entry == "distance":                        # and the planes are right (one search radius for the whole batch)
        for j, n in enumerate(names):
            if LC.CASES[n][1] == sr:
                assert np.abs(batch[0][j] - want(n)["cell"]).max() <= DTOL
                assert np.abs(batch[1][j] - want(n)["nb"]).max() <= DTOL


@pytest.mark.parametrize("name", HYGIENE)
@pytest.mark.parametrize("entry,kw", ENTRIES[:4], ids=["distance", "bottom_hat", "cell_distance", "cell_distance_clip5"])
def test_workspace_content_does_not_matter(lib, name, entry, kw):
    """a workspace full of 0xFF bytes (all tables saturated, every plane NaN / -1) against a zeroed one"""
    mask, sr = LC.CASES[name]
    rc0, clean = c_call(lib, entry, mask[None], sr=sr, fill=0, **kw)
    rc1, dirty = c_call(lib, entry, mask[None], sr=sr, fill=0xFF, **kw)
    assert rc0 == 0 and rc1 == 0
    for a, b in zip(clean, dirty):
        assert np.array_equal(bits(a.host()), bits(b.host()))
    if entry == "distance":
        assert np.abs(clean[0].host()[0] - want(name)["cell"]).max() <= DTOL
        assert np.abs(clean[1].host()[0] - want(name)["nb"]).max() <= DTOL


# ---- contract ---------------------------------------------------------------------------------------------------------------------
def test_whole_window_cell_gives_zero(T):
    """no pixel of the window lies outside the cell: 0 in both maps (header of labels.hip); not an oracle comparison"""
    _, mask, sr = LC.whole_window()
    cell, nb = T.distance_label(mask, sr)
    assert not cell.any() and not nb.any()
    assert not T.cell_distance_label(mask, sr).any()
    assert not T.cell_distance_label(mask, sr, apply_clipping=True).any()


def test_argument_errors_write_nothing(lib):
    mask = LC.CASES["ring_gap"][0][None]
    bad = [("distance", dict(sr=0), EINVAL), ("distance", dict(sr=-3), EINVAL), ("cell_distance", dict(sr=0), EINVAL),
           ("cell_distance", dict(sr=-1), EINVAL), ("cell_distance", dict(sr=4, clip=-1.0), EINVAL),
           ("j4", dict(k=17, r=4), EINVAL), ("j4", dict(k=-1, r=4), EINVAL), ("j4", dict(k=2, r=0), EINVAL),
           ("j4", dict(k=2, r=17), EINVAL), ("boundary", dict(mode=2), EINVAL),
           ("distance", dict(sr=4, ws_short=1), EWORKSPACE), ("bottom_hat", dict(ws_short=1), EWORKSPACE),
           ("cell_distance", dict(sr=4, ws_short=1), EWORKSPACE), ("max_major_axis", dict(ws_short=1), EWORKSPACE)]
    for entry, kw, code in bad:
        rc, outs = c_call(lib, entry, mask, **kw)
        assert rc == code, (entry, kw, rc)
        assert all(o.untouched() for o in outs), (entry, kw)
    assert lib.mseg_label_distance_workspace_bytes(0, 8, 8) == 0 and lib.mseg_label_distance_workspace_bytes(1, 0, 8) == 0
    assert lib.mseg_label_major_axis_workspace_bytes(0) == 0


def test_zz_report(capsys):
    """not a check: the largest difference to the oracle per entry point, over every fixture of this module"""
    with capsys.disabled():
        print("\nlargest |device - oracle| per entry point")
        for entry, (d, name) in sorted(WORST.items()):
            print(f"  {entry:36s} {d:.3g}  ({name})")
