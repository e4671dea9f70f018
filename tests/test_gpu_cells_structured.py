"""GPU (MI355X): the per-cell table kernels (csrc/cells.hip) on the structured worst-case stacks of tests/cells_cases.py
through the C ABI with guarded buffers: every output of mseg_cell_measure and mseg_cell_links bit for bit equal to the
vectorised restatements of tests/cells_ref.py (measure_fast, links_fast), the shifted, field and gap calls byte for byte equal
to the plain one, the pair table at exactly 100 % load, and the frame wider than 2^21 columns through mseg_cell_measure and
mseg_region_stats against Python integers.

tests/test_cells_structured_host.py shows on the CPU which path of cm_kernel each case takes and which defect it notices.
The only floating-point comparison is that of the two axis lengths of mseg_region_stats, at the rtol = 1e-9 of
test_gpu_cells.check_table."""
import ctypes as C
import fractions
import functools
import math

import numpy as np
import pytest
import torch

import cells_cases as CC
import cells_ref as ref
from test_gpu_cells import Guarded, c_links, c_measure, tchw_strides
from test_gpu_drift import c_links_shifted
from test_gpu_flow import c_links_field
from test_gpu_gap import c_links_gap

pytestmark = pytest.mark.gpu
KEYS = ("shape", "bbox", "ch_sums", "ch_minmax", "bg_sums", "bg_minmax")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(_gpu):
    """a HIP error after a test (a faulted kernel) ends the session: nothing more is started on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error, stopping: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def case(name):
    return (CC.MEASURE.get(name) or CC.LINKS[name])()


@functools.lru_cache(maxsize=None)
def want_measure(name):
    """the restatement's answer for one case, computed once and frozen"""
    out = ref.measure_fast(*case(name))
    for v in out.values():
        v.setflags(write=False)
    return out


def assert_same(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.flatnonzero(got[k].ravel() != want[k].ravel())
        assert bad.size == 0, (k, bad.size, bad[:4].tolist(), got[k].ravel()[bad[:4]].tolist(), want[k].ravel()[bad[:4]].tolist())


def measure(lab, off, img):
    """mseg_cell_measure on a [T, C, H, W] image (or none); the guard bands are checked by Guarded.host"""
    if img is None:
        return c_measure(np.array(lab), np.array(off))
    return c_measure(np.array(lab), np.array(off), np.array(img), tchw_strides(img), img.shape[1])


def clean_cap(lab, off):
    """the next power of two above twice the largest number of distinct pairs of a frame pair (at least the ABI's 64)"""
    most = max(len(ref.pairs(lab, off, t)[0]) for t in range(1, lab.shape[0]))
    return max(64, 1 << (2 * most).bit_length())


# ---- measure ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CC.MEASURE))
def test_measure_equals_the_restatement(name):
    lab, off, img = case(name)
    assert_same(measure(lab, off, img), want_measure(name))


@pytest.mark.parametrize("name", ["M1_tiny_frames_a", "M1_tiny_frames_b"])
def test_m1_without_an_image_and_with_five_channels(name):
    lab, off, img = case(name)
    want = want_measure(name)
    bufs = c_measure(np.array(lab), np.array(off), keep=True)
    assert np.array_equal(bufs["shape"].host(np.uint64), want["shape"]) and np.array_equal(bufs["bbox"].host(np.int32), want["bbox"])
    assert all(bufs[k].untouched() for k in KEYS[2:])
    five = np.random.default_rng(5).integers(0, 256, (lab.shape[0], 5) + lab.shape[1:]).astype(np.uint8)      # two launches
    assert_same(measure(lab, off, five), ref.measure_fast(lab, off, five))


def test_m2_through_an_interleaved_view():
    """[T, H, W, 2] read in place: pixel stride 2, the loads that are not a frame's contiguous plane"""
    lab, off, img = case("M2_three_steps")
    T, H, W = lab.shape
    two = np.concatenate([img, np.random.default_rng(6).integers(0, 256, img.shape).astype(np.uint8)], axis=1)
    hwc = np.ascontiguousarray(np.moveaxis(two, 1, -1))
    got = c_measure(np.array(lab), np.array(off), hwc, (H * W * 2, 1, 2 * W, 2), 2)
    want = ref.measure_fast(lab, off, two)
    assert_same(got, want)
    for k in KEYS:                                  # channel 0 is the case's own image
        sub = want[k] if k in ("shape", "bbox") else want[k][..., :1] if k.startswith("bg") else want[k][:, :1]
        assert np.array_equal(sub, want_measure("M2_three_steps")[k]), k


def test_m6_sums_equal_python_integers():
    lab, off, img = case("M6_wide_frame")
    got = measure(lab, off, img)
    shape, bbox = CC.wide_frame_sums()
    print("sum_xx device", [int(v) for v in got["shape"][4]], "exact", shape[4])
    assert [[int(v) for v in row] for row in got["shape"]] == shape
    assert got["bbox"].tolist() == bbox


def test_m6_region_stats_area_and_axes():
    """mseg_region_stats on the wide frame as int32: area exact, the axis lengths against fp64 values derived from the exact
    integer moments (rational arithmetic up to the eigenvalues' square root) at rtol = 1e-9"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    lab, off, _ = case("M6_wide_frame")
    T, H, W = lab.shape
    n = int(off[-1])
    lab_d, off_d = torch.from_numpy(lab.astype(np.int32)).cuda(), torch.from_numpy(np.array(off)).cuda()
    area, total = Guarded((n,), torch.int64), Guarded((T,), torch.int64)
    major, minor = (torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    ws = torch.zeros(lib.mseg_region_stats_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    code = lib.mseg_region_stats(lab_d.data_ptr(), T, H, W, off_d.data_ptr(), n, area.ptr, major[1:].data_ptr(),
                                 minor[1:].data_ptr(), total.ptr, ws.data_ptr(), ws.numel(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert code == 0, code
    shape, _ = CC.wide_frame_sums()
    assert area.host(np.int64).tolist() == shape[0]
    assert total.host(np.int64).tolist() == [sum((k + 1) * shape[0][k] for k in range(n))]
    major, minor = major.cpu().numpy(), minor.cpu().numpy()
    assert np.isnan(major[[0, -1]]).all() and np.isnan(minor[[0, -1]]).all()
    want = []
    for k in range(n):
        N, sy, sx, syy, sxx, sxy = (shape[j][k] for j in range(6))
        F = fractions.Fraction
        a, c, b = F(N * syy - sy * sy, N * N), F(N * sxx - sx * sx, N * N), F(N * sxy - sx * sy, N * N)
        h, q2 = (a + c) / 2, (a - c) * (a - c) / 4 + b * b
        # sqrt of a rational to 30 digits by an integer square root (exact where q2 is a square: every one-row cell)
        q = F(math.isqrt(q2.numerator * q2.denominator * 10 ** 60), q2.denominator * 10 ** 30)
        want.append((4 * math.sqrt(max(float(h + q), 0.0)), 4 * math.sqrt(max(float(h - q), 0.0))))
    print("major", major[1:-1].tolist(), "minor", minor[1:-1].tolist(), "want", want)
    np.testing.assert_allclose(major[1:-1], [w[0] for w in want], rtol=1e-9, atol=0)
    np.testing.assert_allclose(minor[1:-1], [w[1] for w in want], rtol=1e-9, atol=0)


# ---- links ------------------------------------------------------------------------------------------------------------------------
def link_dtypes(name, lab):
    return (np.int32,) if lab.dtype == np.int32 else (np.uint16, np.int32)


@pytest.mark.parametrize("name", sorted(CC.LINKS))
def test_links_equal_the_restatement_and_the_four_calls_agree(name):
    lab0, off, _ = case(name)
    off = np.array(off)                             # copies go to the device: the cases are read-only
    T, H, W = lab0.shape
    n = int(off[-1])
    want_pred, want_ovl = ref.links_fast(lab0, off)
    cap = clean_cap(lab0, off)
    zero, field = np.zeros((T, 2), np.int32), np.zeros((T, -(-H // 64), -(-W // 64), 2), np.int32)
    ones = np.ones(n, bool)
    for dt in link_dtypes(name, lab0):
        lab = lab0.astype(dt)
        pred, ovl, status = c_links(lab, off, cap)
        assert not status.any(), (dt, cap)
        assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl), dt
        others = {"shifted": c_links_shifted(lab, off, cap, zero), "field": c_links_field(lab, off, cap, field, 64),
                  "gap": c_links_gap(lab, off, cap, 1, ones, ones)}
        for call, (p, o, s) in others.items():
            assert p.tobytes() == pred.tobytes() and o.tobytes() == ovl.tobytes() and s.tobytes() == status.tobytes(), (dt, call)


@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
def test_l1_table_of_64_holds_64_pairs_and_reports_65(label_dtype):
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab0, off, _ = case("L1_exact_fill")
    off = np.array(off)
    lab = lab0.astype(label_dtype)
    want_pred, want_ovl = ref.links_fast(lab0, off)
    n = int(off[-1])
    zero, field = np.zeros((3, 2), np.int32), np.zeros((3, 1, 1, 2), np.int32)
    calls = {"plain": c_links(lab, off, CC.L1_CAP), "shifted": c_links_shifted(lab, off, CC.L1_CAP, zero),
             "field": c_links_field(lab, off, CC.L1_CAP, field, 64),
             "gap": c_links_gap(lab, off, CC.L1_CAP, 1, np.ones(n, bool), np.ones(n, bool))}
    for call, (pred, ovl, status) in calls.items():
        assert status[0] == 0 and status[1] == 0 and status[2] != 0, (call, status)
        s = slice(0, int(off[2]))                   # frames 0 and 1: the table of 64 took all 64 pairs
        assert np.array_equal(pred[s], want_pred[s]) and np.array_equal(ovl[s], want_ovl[s]), call
    lab_d = torch.from_numpy(lab.view(np.int16) if label_dtype == np.uint16 else lab).cuda()
    pix = _lib.PIX_U16 if label_dtype == np.uint16 else _lib.PIX_I32
    pred, ovl = cells.link_raw(lab_d, pix, off, table_cap=CC.L1_CAP)      # redoes the full pair
    assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes():
    for name in ("M1_tiny_frames_a", "M1_tiny_frames_b"):
        a, b = (measure(*case(name)) for _ in range(2))
        assert all(a[k].tobytes() == b[k].tobytes() for k in KEYS), name
    for name in ("L2_one_over_many", "L2_many_over_one"):
        lab, off, _ = case(name)
        cap = clean_cap(lab, off)
        a, b = (c_links(np.array(lab), np.array(off), cap) for _ in range(2))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name
