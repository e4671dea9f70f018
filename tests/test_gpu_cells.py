"""GPU (MI355X): the per-cell table kernels (csrc/cells.hip) through the C ABI and through measure_cells, bit for bit
against the numpy restatement tests/cells_ref.py; scikit-image's own values through the device path.

Maxima measured on an MI355X (derived floats of measure_cells against the fp64 restatement, all cases of this file): see
DESIGN.md §2, row "per-cell table"."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

import cells_ref as ref
from test_cells_host import CASES, check_against_library, load_case

pytestmark = pytest.mark.gpu
GUARD = 64
SENT64, SENT32 = -0x0123456789ABCDEF, 0x5A5A5A5A
PIX = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int32): 2}
EINVAL, EWORKSPACE = -1, -3


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Guarded:
    """a device buffer between two guard bands, everything pre-filled with a sentinel"""

    def __init__(self, shape, dtype):
        self.shape, self.n = shape, int(np.prod(shape))
        self.fill = SENT64 if dtype == torch.int64 else SENT32
        self.t = torch.full((self.n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def host(self, view):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == self.fill).all() and (h[GUARD + self.n:] == self.fill).all(), "guard band written"
        return h[GUARD:GUARD + self.n].view(view).reshape(self.shape)

    def untouched(self):
        return bool((self.t == self.fill).all())


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def c_measure(lab, off, base=None, strides=(0, 0, 0, 0), nch=0, keep=False):
    """mseg_cell_measure through ctypes.  lab: uint16 / int32 [T, H, W]; base: the image's memory (any shape) with the
    element strides (frame, channel, row, pixel) of channel 0.  -> the outputs as in cells_ref.measure"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    lab_d, off_d = _dev(lab), torch.from_numpy(np.asarray(off, np.int64)).cuda()
    img_d = _dev(base) if base is not None else None
    bufs = {"shape": Guarded((6, n), torch.int64), "bbox": Guarded((n, 4), torch.int32),
            "ch_sums": Guarded((2, nch, n), torch.int64), "ch_minmax": Guarded((2, nch, n), torch.int32),
            "bg_sums": Guarded((3, T, nch), torch.int64), "bg_minmax": Guarded((2, T, nch), torch.int32)}
    code = lib.mseg_cell_measure(lab_d.data_ptr(), PIX[lab.dtype], T, H, W, off_d.data_ptr(), n,
                                 img_d.data_ptr() if img_d is not None else None,
                                 PIX[base.dtype] if base is not None else 0, nch, *(int(s) for s in strides),
                                 bufs["shape"].ptr, bufs["bbox"].ptr, bufs["ch_sums"].ptr, bufs["ch_minmax"].ptr,
                                 bufs["bg_sums"].ptr, bufs["bg_minmax"].ptr,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert code == 0, code
    if keep:
        return bufs
    views = {"shape": np.uint64, "bbox": np.int32, "ch_sums": np.uint64, "ch_minmax": np.uint32, "bg_sums": np.uint64,
             "bg_minmax": np.uint32}
    return {k: b.host(views[k]) for k, b in bufs.items()}


def c_links(lab, off, cap):
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n = int(off[-1])
    lab_d, off_d = _dev(lab), torch.from_numpy(np.asarray(off, np.int64)).cuda()
    pred, ovl, status = Guarded((n,), torch.int32), Guarded((n,), torch.int32), Guarded((T,), torch.int32)
    nbytes = lib.mseg_cell_links_workspace_bytes(T, n, cap)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    code = lib.mseg_cell_links(lab_d.data_ptr(), PIX[lab.dtype], T, H, W, off_d.data_ptr(), n, cap, pred.ptr, ovl.ptr,
                               status.ptr, ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert code == 0, code
    return pred.host(np.int32), ovl.host(np.int32), status.host(np.int32)


def tchw_strides(img):
    T, Cn, H, W = img.shape
    return (Cn * H * W, H * W, W, 1)


def assert_same(got, want, keys=None):
    for k in keys or want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def scene_a(label_dtype):
    """T = 3, 37 x 53: rows shorter than a wave.  Frame 0 / 1: blobs, a label that ends a row at the last column and goes on at
    column 0 of the next row, 1-pixel cells, absent ids, ids above the frame's table; frame 2 has no cells."""
    rng = np.random.default_rng(7)
    T, H, W = 3, 37, 53
    lab = np.zeros((T, H, W), np.int64)
    for t in range(2):
        k = 0
        for _ in range(14):
            k += 1
            if k in (3, 9):
                continue                                        # absent ids
            y, x = rng.integers(0, H - 6), rng.integers(0, W - 9)
            lab[t, y:y + rng.integers(1, 6), x:x + rng.integers(1, 9)] = k
        lab[t, 10, W - 3:] = 15                                 # ends row 10 at the last column ...
        lab[t, 11, :4] = 15                                     # ... and starts row 11 at column 0
        lab[t, 20, W - 1] = 16
        lab[t, 21, 0] = 16
        for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (18, 7), (18, 9))):
            lab[t, y, x] = 17 + i                               # 1-pixel cells
        lab[t, 30:33, 20:30] = 40 + t                           # above the table (22 entries)
        lab[t, 5, 5] = 1000
    off = np.array([0, 22, 44, 44], np.int64)
    return lab.astype(label_dtype), off


@pytest.fixture(scope="module")
def images_a():
    rng = np.random.default_rng(11)
    img16 = rng.integers(0, 65536, (3, 2, 37, 53)).astype(np.uint16)
    img8 = rng.integers(0, 256, (3, 1, 37, 53)).astype(np.uint8)
    return img16, img8


@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
def test_measure_shape_a_rows_shorter_than_a_wave(label_dtype, images_a):
    lab, off = scene_a(label_dtype)
    assert (lab[0, 10, -1] == lab[0, 11, 0] == 15) and lab[2].max() == 0 and (lab[0] == 3).sum() == 0
    for img in images_a:
        got = c_measure(lab, off, img, tchw_strides(img), img.shape[1])
        assert_same(got, ref.measure(lab, off, img))
    s = int(off[0]) + 15 - 1            # the row-crossing label is one cell of two runs: its box spans both rows
    assert got["bbox"][s].tolist() == [10, 0, 12, 53]


def test_measure_shape_b_runs_across_lane_and_wave_boundaries():
    """T = 1, 8 x 200: runs of length 1 .. 70 starting at x = 61 .. 66 (rows 0 .. 5: every offset against the 8-pixel lanes
    and the 512-pixel wave steps), and one label that crosses from the end of row 6 into row 7"""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 65536, (1, 2, 8, 200)).astype(np.uint16)
    img8 = rng.integers(0, 256, (1, 1, 8, 200)).astype(np.uint8)
    off = np.array([0, 7], np.int64)
    for length in range(1, 71):
        lab = np.zeros((1, 8, 200), np.uint16)
        for r, x0 in enumerate(range(61, 67)):
            lab[0, r, x0:x0 + length] = r + 1
        lab[0, 6, 200 - length:] = 7
        lab[0, 7, :length] = 7
        got = c_measure(lab, off, img, tchw_strides(img), 2)
        assert_same(got, ref.measure(lab, off, img))
        got = c_measure(lab.astype(np.int32), off, img8, tchw_strides(img8), 1)
        assert_same(got, ref.measure(lab, off, img8))


def test_measure_shape_c_sums_past_32_bits_and_background_slot():
    T, H, W = 1, 300, 300
    img = np.full((T, 1, H, W), 65535, np.uint16)
    lab = np.ones((T, H, W), np.uint16)
    got = c_measure(lab, np.array([0, 1], np.int64), img, tchw_strides(img), 1)
    assert int(got["ch_sums"][0, 0, 0]) == 90000 * 65535 > 2 ** 32
    assert int(got["ch_sums"][1, 0, 0]) == 90000 * 65535 ** 2
    assert_same(got, ref.measure(lab, np.array([0, 1], np.int64), img))
    assert got["bg_sums"].sum() == 0 and got["bg_minmax"].sum() == 0
    lab0 = np.zeros((T, H, W), np.uint16)
    got = c_measure(lab0, np.array([0, 0], np.int64), img, tchw_strides(img), 1)
    assert got["bg_sums"][:, 0, 0].tolist() == [90000, 90000 * 65535, 90000 * 65535 ** 2]
    assert got["bg_minmax"][:, 0, 0].tolist() == [65535, 65535]


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_measure_layouts_through_the_strides(dtype):
    rng = np.random.default_rng(3)
    H, W = 37, 53
    lab, off = scene_a(np.uint16)
    lab, off = lab[:1], off[:2]
    chw = rng.integers(0, np.iinfo(dtype).max + 1, (3, H, W)).astype(dtype)
    hwc = np.ascontiguousarray(np.moveaxis(chw, 0, -1))
    want = ref.measure(lab, off, chw[None])
    assert_same(c_measure(lab, off, chw[None], (3 * H * W, H * W, W, 1), 3), want)          # [T, C, H, W]
    assert_same(c_measure(lab, off, hwc, (H * W * 3, 1, 3 * W, 3), 3), want)                # [H, W, 3] interleaved
    assert_same(c_measure(lab, off, chw, (0, H * W, W, 1), 3), want)                        # [3, H, W]
    # a padded row pitch: every row starts 3 elements further than W
    pitched = np.zeros((3, H, W + 3), dtype)
    pitched[:, :, :W] = chw
    assert_same(c_measure(lab, off, pitched, (0, H * (W + 3), W + 3, 1), 3), want)


def test_measure_without_channels_touches_no_channel_buffer(images_a):
    lab, off = scene_a(np.uint16)
    img = images_a[0]
    want = ref.measure(lab, off, img)
    for base, nch in ((None, 0), (img, 0), (None, 2)):
        bufs = c_measure(lab, off, base, tchw_strides(img), nch, keep=True)
        assert np.array_equal(bufs["shape"].host(np.uint64), want["shape"])
        assert np.array_equal(bufs["bbox"].host(np.int32), want["bbox"])
        for k in ("ch_sums", "ch_minmax", "bg_sums", "bg_minmax"):
            assert bufs[k].untouched(), k


def test_measure_more_channels_than_one_launch_holds():
    rng = np.random.default_rng(9)
    lab, off = scene_a(np.int32)
    img = rng.integers(0, 65536, (3, 6, 37, 53)).astype(np.uint16)
    assert_same(c_measure(lab, off, img, tchw_strides(img), 6), ref.measure(lab, off, img))


# ---- derived values -----------------------------------------------------------------------------------------------------------
def check_table(df, want, channels, link):
    """measure_cells against cells_ref.table: integers, centroid and mean bit-equal, std and axes rtol 1e-9, orientation as
    in the host test; prints the maxima"""
    from microbeseg_amd.inference import cells
    assert list(df.columns) == cells.columns(channels, link) == [c for c in want.columns if c != "_skip"]
    assert len(df) == len(want)
    exact = ["frame", "label", "area", "centroid_y", "centroid_x", "bbox_min_row", "bbox_min_col", "bbox_max_row",
             "bbox_max_col", "touches_border"]
    close = ["major_axis_length", "minor_axis_length"]
    for c in channels:
        exact += [f"{k}_ch{c}" for k in ("mean", "min", "max", "sum", "bg_mean")]
        close.append(f"std_ch{c}")
    if link:
        exact += ["pred_label", "overlap", "track_id", "parent_track"]
    for col in exact:
        a, b = df[col].to_numpy(), want[col].to_numpy()
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), col
    worst = {}
    for col in close:
        a, b = df[col].to_numpy(np.float64), want[col].to_numpy(np.float64)
        worst[col] = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))
    skip = want["_skip"].to_numpy(bool)
    a, b = df["orientation"].to_numpy(np.float64)[~skip], want["orientation"].to_numpy(np.float64)[~skip]
    worst["orientation_abs"] = float(np.max(np.abs(a - b), initial=0.0))
    print("max relative difference to the fp64 restatement:", worst)
    for col in close:
        np.testing.assert_allclose(df[col].to_numpy(np.float64), want[col].to_numpy(np.float64), rtol=1e-9, atol=0)
    if len(skip):
        assert skip.mean() <= 0.10
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-6)


def blob_stack(T=2, H=61, W=83, n=18, seed=2):
    """non-overlapping random ellipses drifting by 1 - 2 px per frame (uint16 labels) and a 2-channel uint16 image"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    lab = np.zeros((T, H, W), np.uint16)
    cells = []
    for _ in range(300):
        if len(cells) == n:
            break
        cy, cx, a, b, th = rng.uniform(4, H - 4), rng.uniform(4, W - 4), rng.uniform(3, 8), rng.uniform(1.5, 3), rng.uniform(0, np.pi)
        if all((cy - c[0]) ** 2 + (cx - c[1]) ** 2 > (a + c[2] + 1.5) ** 2 for c in cells):
            cells.append((cy, cx, a, b, th))
    for t in range(T):
        for k, (cy, cx, a, b, th) in enumerate(cells):
            dy, dx = yy - (cy + 1.5 * t), xx - (cx + t)
            u, v = dy * np.cos(th) + dx * np.sin(th), -dy * np.sin(th) + dx * np.cos(th)
            lab[t][(u / a) ** 2 + (v / b) ** 2 <= 1] = k + 1
    img = rng.integers(0, 65536, (T, 2, H, W)).astype(np.uint16)
    return lab, img


def test_measure_cells_derived_values():
    from microbeseg_amd.inference.cells import measure_cells
    lab, img = blob_stack()
    check_table(measure_cells(lab, img, link=False), ref.table(lab, img, channels=[0, 1], link=False), [0, 1], False)
    # one channel out of two, named by its index; int32 labels; a device tensor as the image
    df = measure_cells(lab.astype(np.int32), torch.from_numpy(img.view(np.int16)).cuda(), channels=[1], link=False)
    check_table(df, ref.table(lab, img, channels=[1], link=False), [1], False)
    lab_a, _ = scene_a(np.uint16)        # 1-pixel cells, the row-crossing label
    lab_a[lab_a > 22] = 0
    check_table(measure_cells(lab_a, link=False), ref.table(lab_a, link=False), [], False)


def test_measure_cells_views_of_interleaved_and_planar_sources():
    from microbeseg_amd.inference.cells import measure_cells
    lab, img = blob_stack(T=1)
    chw = img[0, [0, 1, 0]]
    hwc = np.ascontiguousarray(np.moveaxis(chw, 0, -1))
    want = measure_cells(lab, chw[None], link=False)
    got = measure_cells(lab, np.moveaxis(hwc, -1, 0)[None], link=False)      # [H, W, 3] read in place
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    got = measure_cells(lab, np.moveaxis(hwc, -1, 0)[None], channels=[0, 2], link=False)
    pd.testing.assert_frame_equal(got, want[list(got.columns)], check_exact=True)


@pytest.mark.parametrize("name", CASES)
def test_regionprops_fixture_through_measure_cells(name):
    from microbeseg_amd.inference.cells import measure_cells
    g = load_case(name)
    df = measure_cells(g["label"], g["img"], link=False)
    check_against_library(df, g, ref.table(g["label"][None], link=False)["_skip"])


# ---- links ---------------------------------------------------------------------------------------------------------------------
def scripted_scene():
    """T = 4, 64 x 96, blobs drifting 1 - 2 px per frame: a division, a merge, an appearance, a disappearance, an exact tie
    between two predecessors, a cell over background only"""
    T, H, W = 4, 64, 96
    lab = np.zeros((T, H, W), np.uint16)

    def rect(t, k, y, x, h, w):
        lab[t, y:y + h, x:x + w] = k

    for t in range(T):                      # a plain drifting cell, id 1 everywhere
        rect(t, 1, 4 + t, 4 + 2 * t, 6, 10)
    rect(0, 2, 20, 10, 8, 16)               # divides in frame 1
    rect(1, 2, 21, 11, 8, 7)
    rect(1, 3, 21, 19, 8, 9)
    rect(2, 2, 22, 12, 8, 7)
    rect(2, 3, 22, 21, 8, 9)
    rect(3, 2, 23, 13, 8, 7)
    rect(3, 3, 23, 22, 8, 9)
    rect(0, 3, 40, 10, 6, 8)                # ids 3 and 4 of frame 0 merge in frame 2
    rect(0, 4, 40, 20, 6, 8)
    rect(1, 4, 41, 11, 6, 8)
    rect(1, 5, 41, 20, 6, 5)
    rect(2, 4, 42, 12, 6, 16)
    rect(3, 4, 43, 13, 6, 16)
    rect(0, 5, 50, 60, 4, 6)                # disappears after frame 1
    rect(1, 6, 51, 61, 4, 6)
    rect(2, 5, 4, 70, 4, 6)                 # appears in frame 2 over background
    rect(3, 5, 5, 71, 4, 6)
    rect(0, 6, 30, 60, 6, 4)                # two neighbours ...
    rect(0, 7, 30, 64, 6, 4)
    rect(1, 7, 30, 62, 6, 4)                # ... and a cell with 12 pixels on each: the tie goes to the smaller id
    rect(2, 6, 31, 63, 6, 4)
    rect(3, 6, 32, 64, 6, 4)
    return lab


@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
def test_links_scripted_scene(label_dtype):
    lab = scripted_scene().astype(label_dtype)
    off = ref.frame_tables(lab)
    pred, ovl, status = c_links(lab, off, 1024)
    want_pred, want_ovl = ref.links(lab, off)
    assert not status.any()
    assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
    assert not pred[:off[1]].any() and not ovl[:off[1]].any()              # frame 0
    at = lambda t, l: int(off[t]) + l - 1
    assert pred[at(1, 2)] == 2 and pred[at(1, 3)] == 2                         # division
    assert pred[at(2, 4)] == 4 and ovl[at(2, 4)] > 0                           # merge: the larger overlap wins
    assert pred[at(2, 5)] == 0 and ovl[at(2, 5)] == 0                          # appearance over background
    assert 6 not in pred[off[2]:off[3]]                                        # disappearance: nobody names it
    assert pred[at(1, 7)] == 6 and ovl[at(1, 7)] == 12                         # the tie
    assert ((lab[1] == 7) & (lab[0] == 7)).sum() == 12


def random_small_labels(seed=4):
    """T = 3, 96 x 128, about 2000 labels of 2 x 3 pixels per frame on a grid that shifts from frame to frame"""
    rng = np.random.default_rng(seed)
    T, H, W = 3, 96, 128
    lab = np.zeros((T, H, W), np.uint16)
    for t in range(T):
        gy, gx = (H - t) // 2, (W - t) // 3
        ids = rng.permutation(gy * gx) + 1
        ids[rng.random(ids.size) < 0.03] = 0
        block = np.repeat(np.repeat(ids.reshape(gy, gx), 2, axis=0), 3, axis=1)
        lab[t, t:t + 2 * gy, t:t + 3 * gx] = block
    return lab


def test_links_random_case_and_table_overflow():
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    lab = random_small_labels()
    off = ref.frame_tables(lab)
    assert np.diff(off).min() > 1900
    want_pred, want_ovl = ref.links(lab, off)
    pred, ovl, status = c_links(lab, off, 16384)              # more entries than H * W = 12288 pixels: cannot fill up
    assert not status.any() and np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
    # the smallest table the ABI accepts fills up: the status word of both frame pairs says so
    lib = _lib.load()
    assert lib.mseg_cell_links_workspace_bytes(3, int(off[-1]), 32) == 0
    assert lib.mseg_cell_links_workspace_bytes(3, int(off[-1]), 96) == 0
    _, _, status = c_links(lab, off, 64)
    assert status[0] == 0 and status[1] != 0 and status[2] != 0
    # the wrapper redoes such pairs at the worst-case size: exact again
    lab_d = _dev(lab)
    pred, ovl = cells.link_raw(lab_d, _lib.PIX_U16, off, table_cap=64)
    assert np.array_equal(pred, want_pred) and np.array_equal(ovl, want_ovl)
    df = cells.measure_cells(lab, link=True)
    present = np.concatenate([np.bincount(lab[t].ravel(), minlength=int(k) + 1)[1:int(k) + 1] > 0
                              for t, k in enumerate(np.diff(off))])
    assert np.array_equal(df["pred_label"].to_numpy(), want_pred[present])
    assert np.array_equal(df["overlap"].to_numpy(), want_ovl[present])


@pytest.mark.parametrize("label_dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("shape", [(5, 63), (5, 65), (70, 131)])
def test_links_on_frames_that_are_no_multiple_of_eight_pixels(shape, label_dtype):
    """H * W = 315, 325, 9170: the last lane of every frame takes the loader's scalar tail, and with uint16 labels every
    second frame starts at an address that is no multiple of 16 bytes.  The plain call against the restatement, and byte for
    byte against the shifted and the field call under all-zero shifts."""
    import drift_ref as dref
    from test_gpu_drift import c_links_shifted, random_labels
    from test_gpu_flow import c_links_field
    H, W = shape
    lab64, off = random_labels(H, W)
    T = lab64.shape[0]
    lab, off = lab64.astype(label_dtype), np.array(off)       # copies: the sources are read-only
    assert T == 4 and (H * W) % 8 != 0
    zero = np.zeros((T, 2), np.int32)
    field = np.zeros((T, -(-H // 64), -(-W // 64), 2), np.int32)
    want_pred, want_ovl = dref.links_shifted(lab64, off, zero)
    assert want_ovl.any()
    clean = 1 << (H * W).bit_length()                         # more entries than pixels: cannot fill up
    for cap in (64, clean):
        pred, ovl, status = c_links(lab, off, cap)
        moved = [c_links_shifted(lab, off, cap, zero), c_links_field(lab, off, cap, field, 64)]
        assert status[0] == 0 and (cap == 64 or not status.any())
        for other in moved:
            assert np.array_equal(other[2] != 0, status != 0), cap
        for t in np.nonzero(status == 0)[0]:
            s = slice(int(off[t]), int(off[t + 1]))
            assert np.array_equal(pred[s], want_pred[s]) and np.array_equal(ovl[s], want_ovl[s]), (cap, t)
            for other in moved:
                assert pred[s].tobytes() == other[0][s].tobytes() and ovl[s].tobytes() == other[1][s].tobytes(), (cap, t)


def c_cells_refused(entry, lab, off, dtype_code=None, dims=None, n=None, cap=1024, tile=64, null_shift=False, short=0):
    """One call of ``entry`` (measure, links, links_shifted, links_field) that must be refused: every output and the
    workspace are guarded and pre-filled.  The overrides replace single arguments of an otherwise valid call.
    -> (return code, True if nothing was written)"""
    from microbeseg_amd import _lib
    lib = _lib.load()
    T, H, W = lab.shape
    n_real = int(off[-1])
    lab_d, off_d = _dev(lab), torch.from_numpy(np.array(off, np.int64)).cuda()      # a copy: the source is read-only
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (lab_d.data_ptr(), PIX[lab.dtype] if dtype_code is None else dtype_code, *(dims or (T, H, W)), off_d.data_ptr(),
            n_real if n is None else n)
    if entry == "measure":
        img = _dev(np.random.default_rng(1).integers(0, 65536, (T, 1, H, W)).astype(np.uint16))
        bufs = [Guarded((6, n_real), torch.int64), Guarded((n_real, 4), torch.int32), Guarded((2, 1, n_real), torch.int64),
                Guarded((2, 1, n_real), torch.int32), Guarded((3, T, 1), torch.int64), Guarded((2, T, 1), torch.int32)]
        code = lib.mseg_cell_measure(*head, img.data_ptr(), PIX[np.dtype(np.uint16)], 1, H * W, H * W, W, 1,
                                     *(b.ptr for b in bufs), stream)
    else:
        bufs = [Guarded((n_real,), torch.int32), Guarded((n_real,), torch.int32), Guarded((T,), torch.int32)]
        nbytes = lib.mseg_cell_links_workspace_bytes(T, n_real, 1024)
        assert nbytes > 0
        ws = Guarded((nbytes // 4,), torch.int32)
        bufs.append(ws)
        tail = (*(b.ptr for b in bufs[:3]), ws.ptr, nbytes - short, stream)
        if entry == "links":
            code = lib.mseg_cell_links(*head, cap, *tail)
        elif entry == "links_shifted":
            shift = torch.zeros((T, 2), dtype=torch.int32, device="cuda")
            code = lib.mseg_cell_links_shifted(*head, cap, None if null_shift else shift.data_ptr(), *tail)
        else:
            field = torch.zeros((T, -(-H // 64), -(-W // 64), 2), dtype=torch.int32, device="cuda")
            code = lib.mseg_cell_links_field(*head, cap, tile, field.data_ptr(), *tail)
    torch.cuda.synchronize()
    return code, all(b.untouched() for b in bufs)


@pytest.mark.parametrize("entry", ["measure", "links", "links_shifted", "links_field"])
def test_argument_errors_touch_nothing(entry):
    """a refused call writes nothing: neither an output, nor a status word, nor the workspace (so no memset and no kernel ran)"""
    from test_gpu_drift import random_labels
    lab64, off = random_labels(5, 65)
    lab = lab64.astype(np.uint16)
    T, H, W = lab.shape
    bad = [dict(dtype_code=0), dict(dtype_code=3), dict(n=-1)]
    bad += [dict(dims=d) for d in ((0, H, W), (T, 0, W), (T, H, 0), (-1, H, W), (T, -5, W), (T, H, -65))]
    if entry != "measure":
        bad += [dict(cap=96), dict(cap=32)]
    if entry == "links_field":
        bad.append(dict(tile=32))
    if entry == "links_shifted":
        bad.append(dict(null_shift=True))
    assert c_cells_refused(entry, lab, off) == (0, False)       # the call the bad ones are made from is a good one
    for kw in bad:
        assert c_cells_refused(entry, lab, off, **kw) == (EINVAL, True), kw
    if entry != "measure":
        assert c_cells_refused(entry, lab, off, short=1) == (EWORKSPACE, True)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_end_to_end_table_and_csv(tmp_path):
    from microbeseg_amd.inference.cells import measure_cells, write_cells
    lab = scripted_scene()
    img = np.random.default_rng(8).integers(0, 65536, (4, 2, 64, 96)).astype(np.uint16)
    for min_overlap in (1, 30):
        df = measure_cells(lab, img, min_overlap=min_overlap)
        check_table(df, ref.table(lab, img, channels=[0, 1], link=True, min_overlap=min_overlap), [0, 1], True)
    assert df["track_id"].max() > measure_cells(lab, img)["track_id"].max()      # the cut made new tracks
    write_cells(df, tmp_path / "cells.csv")
    back = pd.read_csv(tmp_path / "cells.csv", float_precision="round_trip")
    pd.testing.assert_frame_equal(back, df, check_exact=True, check_dtype=False)


def test_two_runs_give_identical_bytes(images_a):
    from microbeseg_amd.inference.cells import measure_cells
    lab, off = scene_a(np.uint16)
    img = images_a[0]
    a, b = (c_measure(lab, off, img, tchw_strides(img), 2) for _ in range(2))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    rl = random_small_labels()
    roff = ref.frame_tables(rl)
    a, b = (c_links(rl, roff, 16384) for _ in range(2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    s = scripted_scene()
    simg = np.random.default_rng(1).integers(0, 256, (4, 1, 64, 96)).astype(np.uint8)
    a, b = (measure_cells(s, simg) for _ in range(2))
    assert a.to_csv().encode() == b.to_csv().encode()
    pd.testing.assert_frame_equal(a, b, check_exact=True)


# ---- every family at once --------------------------------------------------------------------------------------------------------
def drifting_grid():
    """uint16 [3, 70, 131]: 4 x 5 ragged cells that drift by (1, -2) per frame, two of them touching; cell 8 is missed in the
    middle frame.  With it a [3, 70, 131, 3] uint16 image, foci on some cells, handed over as the strided [T, 3, H, W] view"""
    rng = np.random.default_rng(12)
    lab = np.zeros((3, 70, 131), np.uint16)
    base = rng.integers(0, 300, (3, 70, 131, 3)).astype(np.uint16)
    for t in range(3):
        for j in range(4):
            for i in range(5):
                l, y, x = 5 * j + i + 1, 4 + 16 * j + t, 12 + 24 * i - 2 * t
                if (t, l) == (1, 8):
                    continue
                lab[t, y:y + 9, x:x + (24 if l == 12 else 15)] = l
                lab[t, y, x:x + 1 + l % 4] = 0                       # ragged corners: no cell is its own hull
                lab[t, y + 8, x + 10 - l % 3:x + 15] = 0
                if l % 3 == 0:
                    base[t, y + 4, x + 3 + l % 5, :] += 40000 + 100 * l
    return lab, np.moveaxis(base, -1, 1)


def test_every_family_at_once_equals_every_family_alone():
    """one measure_cells call with every column family on: the columns of ``columns``, and under every family's columns what
    a call with that family alone returns (the single-family calls are pinned to the restatements by their own files).
    The link columns hold what link, drift, flow and gap make of them together, so they are compared with a call with
    these four on and no other family; pred_gap is compared with link and gap alone as well."""
    from microbeseg_amd.inference import cells
    lab, img = drifting_grid()
    assert not img.flags["C_CONTIGUOUS"] and img.shape == (3, 3, 70, 131)
    ch, motion = [0, 2], dict(drift=4, flow=2, flow_tile=64, gap=1)
    everything = dict(motion, hull=True, midline=True, percentiles=(5, 50), neighbors=3, spots=500, profile=4)
    df = cells.measure_cells(lab, img, ch, **everything)
    assert list(df.columns) == cells.columns(ch, True, True, True, True, (5, 50), True, True, True, True, True)
    assert len(df) == 59 and (df["pred_gap"] == 2).sum() == 1 and df["drift_x"].min() == -4
    assert df[[f"n_spots_ch{c}" for c in ch]].to_numpy().sum() >= 10

    def per_channel(stencil):
        return [name.format(c=c) for c in ch for name in stencil]
    alone = [
        (cells.SHAPE_COLUMNS, dict(link=False)),
        (per_channel(cells.CHANNEL_COLUMNS), dict(img=img, channels=ch, link=False)),
        (cells.LINK_COLUMNS + cells.GAP_COLUMNS, motion),
        (cells.DRIFT_COLUMNS, dict(drift=4)),
        (cells.FLOW_COLUMNS, dict(drift=4, flow=2, flow_tile=64)),
        (cells.GAP_COLUMNS, dict(gap=1)),
        (cells.HULL_COLUMNS, dict(link=False, hull=True)),
        (cells.MIDLINE_COLUMNS, dict(link=False, midline=True)),
        ([name.format(p=p, c=c) for name in cells.PERCENTILE_COLUMNS for c in ch for p in (5, 50)],
         dict(img=img, channels=ch, link=False, percentiles=(5, 50))),
        (cells.NEIGHBOR_COLUMNS, dict(link=False, neighbors=3)),
        (per_channel(cells.SPOT_COLUMNS), dict(img=img, channels=ch, link=False, spots=500)),
        (["axis_extent"] + per_channel(cells.PROFILE_COLUMNS), dict(img=img, channels=ch, link=False, profile=4)),
    ]
    for cols, switches in alone:
        one = cells.measure_cells(lab, **switches)
        assert one[cols].equals(df[cols]), switches


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_infer_script_cells_end_to_end(tmp_path):
    import subprocess
    import sys
    from microbeseg_amd.inference.cells import columns, measure_cells
    from microbeseg_amd.utils import synth, tiffio
    from test_cells_host import ROOT
    from test_gpu_analysis import _constant_distance_model
    model = _constant_distance_model(tmp_path / "distance_model_00")      # one cell per frame, whatever the input
    rng = np.random.Generator(np.random.PCG64(9))
    stack = np.stack([synth.synth_crop(rng, 128)["img"] for _ in range(4)])
    rgb = rng.integers(0, 256, (1, 128, 128, 3)).astype(np.uint8)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    tiffio.imwrite(str(imgs / "movie.tif"), stack)
    tiffio.imwrite(str(imgs / "movie_f32.tif"), stack.astype(np.float32))
    imgs_rgb = tmp_path / "imgs_rgb"
    imgs_rgb.mkdir()
    tiffio.imwrite(str(imgs_rgb / "rgb.tif"), rgb)                          # read back as [H, W, 3]
    res = tmp_path / "results"
    cmd = [sys.executable, str(ROOT / "infer_script_local.py"), "-i", str(imgs), "-m", str(model), "-r", str(res), "--cells"]
    r = subprocess.run(cmd + ["--measure_channels", "0", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "channel" in r.stderr and "--- Start inference ---" not in r.stdout
    assert not list(res.glob("mask_*"))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Skip intensity columns of movie_f32 (they need uint8 / uint16 images, got float32)" in r.stdout
    read = lambda name: pd.read_csv(res / name, float_precision="round_trip")
    mask = tiffio.imread(str(res / "mask_movie_channel0.tif"))
    df = read("mask_movie_channel0_cells.csv")
    pd.testing.assert_frame_equal(df, measure_cells(mask, stack), check_exact=True, check_dtype=False)
    assert df["track_id"].tolist() == [1, 1, 1, 1] and df["pred_label"].tolist() == [0, 1, 1, 1]
    assert list(read("mask_movie_f32_channel0_cells.csv").columns) == columns([], link=True)
    cmd[cmd.index("-i") + 1] = str(imgs_rgb)
    r = subprocess.run(cmd + ["-c", "1", "--measure_channels", "2", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    mask = tiffio.imread(str(res / "mask_rgb_channel1.tif"))
    df = read("mask_rgb_channel1_cells.csv")
    assert list(df.columns) == columns([2, 0], link=True)
    want = measure_cells(mask, np.ascontiguousarray(np.moveaxis(rgb[0], -1, 0))[None], channels=[2, 0])
    pd.testing.assert_frame_equal(df, want, check_exact=True, check_dtype=False)
