"""GPU (MI355X): every kernel form of the network's first layer (microbeseg_amd/csrc/first.hip) through the C ABI —
mseg_first_conv_fwd, mseg_first_conv_fwd_raw, mseg_first_wgrad — pinned to its kernel and compared element by element with
the plain references of tests/conv_ref.py (conv_fwd and wgrad, K = 3, stride 1; P is dz, Q is channel 0 of x4).

ONE table (ROWS).  A row holds the entry, N, Cin, Cout, H, W, the storage of z / dz and the kernel mseg_last_kernel() must
report after the launch (another kernel is launched right before, so a stale name cannot pass).  The library has no query
for these entries; `dispatch` below RESTATES the selection of first.hip (first_rows_ok, first_blocks) so that the table can
be walked without a device: test_row_names_its_kernel, test_table_covers_every_kernel and test_launch_geometry, which
asserts that the shapes reach the paths they are here for.  Keep it in step with first.hip.

Two modes per row:

  exact   operands small integers (|v| <= 3), integer bias; conv_ref.assert_exact checks that the sum of magnitudes S of
          every output stays below 2^24, so every partial sum is exact in fp32 in any order and the fp32 result must equal
          the int64 reference BIT FOR BIT.  A bf16 z must be bit-equal to conv_ref.round_bf16(ref) (sums beyond 256 are
          rounding ties); a bf16 dz holds the same integers exactly.  Raw frames: pixels are the frame's minimum or maximum
          only, which normalise to exactly -1 and +1 (the frame padding is -1 too).
  float   N(0, 1) operands.  Per element e = |got - ref64| / max(S, 2^-100) must satisfy
              e <= max(4 e_ref, FLOOR[kernel])   and   e <= (K + 32) 2^-24
          with K = 9 Cin + 1 for the forward and K = N H W for the weight gradient, e_ref = the largest e of torch's CPU
          fp32 result on the same inputs.  No element is exempt.  A bf16 z is the rounding of an fp32 value y that obeys the
          rule, so half a bf16 ulp (taken at |ref| + (K + 32) 2^-24 S, where y can lie at most) is subtracted from
          |got - ref| before the rule is applied; a bf16 dz is drawn on the bf16 grid, so the rule applies as it is.
          Raw frames: the reference is the fp64 convolution of the header's host formula 2 * (f32(x) - min) / (max - min) - 1
          evaluated in fp32 numpy (tests/test_gpu_kernels.py keeps the bit-for-bit test of the normalised values).

Buffers: z, dW and the weight-gradient workspace are NaN-filled between 256 sentinel words on either side, which must come
back untouched.  x4 holds zeros in the channels Cin .. 3 (the header's contract: first_conv_fwd_kernel<4> multiplies them by
zero weights), except in the Cin = 1 rows, whose kernels must ignore the nonzero junk planted in channels 1 .. 3.  A refused
call (MSEG_EINVAL) writes nothing.

FLOOR, in units of 2^-24: about twice the largest e a kernel showed on the MI355X over all float runs of this table; beside
it torch's CPU fp32 on the same inputs and the largest share of the worst-case bound (K + 32) 2^-24 any element used:
#   kernel                        runs   e_hip    e_ref    e_hip / bound
#   first_conv_fwd_rows_kernel     18    4.28     3.44     0.102       (forward and raw-frame forms)
#   first_conv_fwd_kernel          14    6.28     5.14     0.105
#   first_wgrad_rows_kernel        17    1.05     3.62     0.021
#   first_wgrad_kernel              4    0.54     2.70     0.016
The smallest worst-case bound of the table is 33 (a one-pixel weight gradient): every floor is far below it.  The weight
gradients sit below torch because their second stage sums the partial results in fp64.
"""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
from conv_table import U, TINY, EINVAL, Guarded, _b, _sync, _stream, _eng, _t32

FLOOR = {"first_conv_fwd_rows_kernel": 9.0, "first_conv_fwd_kernel": 13.0, "first_wgrad_rows_kernel": 2.5,
         "first_wgrad_kernel": 1.5}

FR_ROWS = 8


def FROWS(b16): return f"first_conv_fwd_rows_kernel<{_b(b16)}, false>"
def FRAW(b16): return f"first_conv_fwd_rows_kernel<{_b(b16)}, true>"
def FPIX(ci): return f"first_conv_fwd_kernel<{ci}>"
def WROWS(b16): return f"first_wgrad_rows_kernel<{_b(b16)}>"
WPIX = "first_wgrad_kernel"


Row = collections.namedtuple("Row", "id entry N Cin Cout H W st kernel opt")


def fwd(id, N, Cin, Cout, H, W, st, kernel):
    return Row(id, "fwd", N, Cin, Cout, H, W, st, kernel, {})


def wg(id, N, Cout, H, W, st, kernel):
    return Row(id, "wgrad", N, 1, Cout, H, W, st, kernel, {})


def raw(id, pix, H0, W0, pad_top, pad_left, Cout, st, kernel):
    return Row(id, "raw", 1, 1, Cout, H0 + pad_top, W0 + pad_left, st, kernel, dict(pix=pix, H0=H0, W0=W0, pt=pad_top, pl=pad_left))


ROWS = []
# ---- the row-walking forms, Cin 1: forward and weight gradient, both storages --------------------------------------------------
for tag, (N, H, W, Co) in {"one_pixel": (1, 1, 1, 8), "seam_off_unit": (2, 19, 50, 64), "c256": (3, 9, 9, 256),
                           "w_xs_plus_1": (1, 8, 129, 16), "c128": (1, 17, 33, 128), "c32": (2, 7, 64, 32)}.items():
    for st in ("f32", "bf16"):
        ROWS.append(fwd(f"rows_fwd_{tag}_{st}", N, 1, Co, H, W, st, FROWS(st == "bf16")))
        ROWS.append(wg(f"rows_wgrad_{tag}_{st}", N, Co, H, W, st, WROWS(st == "bf16")))
ROWS += [
    # the round-robin second trip of first_wgrad_rows_kernel: accumulators cross units and images
    wg("rows_wgrad_10_units_on_5", 2, 64, 40, 1, "f32", WROWS(0)),
    wg("rows_wgrad_16_units_on_1", 2, 8, 64, 1, "bf16", WROWS(1)),
    wg("rows_wgrad_6_units_on_3", 2, 16, 24, 3, "f32", WROWS(0)),
    # the reduction: 42 partials (a second trip of its own loop), exactly 32, and exactly one (one_pixel above)
    wg("rows_wgrad_42_partials", 1, 64, 48, 200, "f32", WROWS(0)),
    wg("rows_wgrad_32_partials", 4, 64, 64, 2, "bf16", WROWS(1)),
    # ---- per-pixel forward <1>: Cin 1 with Cout 4, the only Cout the row-walking form does not take -----------------------------
    fwd("pix1_one_pixel", 1, 1, 4, 1, 1, "f32", FPIX(1)),
    fwd("pix1_seam", 2, 1, 4, 19, 50, "f32", FPIX(1)),
    fwd("pix1_seam_bf16", 2, 1, 4, 19, 50, "bf16", FPIX(1)),
    # ---- per-pixel forward <4>: Cin 2, 3, 4 ---------------------------------------------------------------------------------------
    fwd("pix4_ci2_c4", 2, 2, 4, 9, 11, "f32", FPIX(4)),
    fwd("pix4_ci2_c16", 1, 2, 16, 5, 7, "bf16", FPIX(4)),
    fwd("pix4_ci2_c64", 2, 2, 64, 9, 11, "f32", FPIX(4)),
    fwd("pix4_ci3_c4", 1, 3, 4, 19, 50, "bf16", FPIX(4)),
    fwd("pix4_ci3_c16", 2, 3, 16, 9, 11, "f32", FPIX(4)),
    fwd("pix4_ci3_c64", 1, 3, 64, 5, 7, "bf16", FPIX(4)),
    fwd("pix4_ci4_c4", 2, 4, 4, 9, 11, "f32", FPIX(4)),
    fwd("pix4_ci4_c16", 1, 4, 16, 19, 50, "f32", FPIX(4)),
    fwd("pix4_ci4_c64", 2, 4, 64, 9, 11, "bf16", FPIX(4)),
    fwd("pix4_ci3_c128", 1, 3, 128, 5, 7, "f32", FPIX(4)),
    fwd("pix4_grid_stride", 1, 3, 256, 182, 181, "f32", FPIX(4)),             # 32 942 pixels against 32 768 per pass
    # ---- per-pixel weight gradient: Cout 4 only -------------------------------------------------------------------------------------
    wg("wpix_one_pixel", 1, 4, 1, 1, "f32", WPIX),
    wg("wpix_seam", 3, 4, 9, 70, "f32", WPIX),
    wg("wpix_seam_bf16", 3, 4, 9, 70, "bf16", WPIX),
    wg("wpix_two_pixels_per_slot", 1, 4, 725, 725, "f32", WPIX),                 # exact mode: S <= 9 x 525 625 < 2^24
    # ---- raw frames: uint8 / uint16, pads (0, 0), (3, 0), (0, 5), (12, 7), Cout 8 / 64 / 256, both storages --------------------------
    raw("raw_u8_c8", "u8", 19, 50, 0, 0, 8, "f32", FRAW(0)),
    raw("raw_u16_padtop_c64", "u16", 9, 9, 3, 0, 64, "bf16", FRAW(1)),
    raw("raw_u8_padleft_c256", "u8", 17, 33, 0, 5, 256, "bf16", FRAW(1)),
    raw("raw_u16_pads_c8", "u16", 8, 129, 12, 7, 8, "bf16", FRAW(1)),
    raw("raw_u16_c256", "u16", 7, 64, 0, 0, 256, "f32", FRAW(0)),
    raw("raw_u8_pads_c64", "u8", 1, 1, 12, 7, 64, "f32", FRAW(0)),
]
ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)
BY = {r.id: r for r in ROWS}

# every kernel instantiation first.hip can launch from the three entries (first_wgrad_reduce_kernel follows every weight
# gradient as a helper and does not name a call)
REACHABLE = [FROWS(0), FROWS(1), FRAW(0), FRAW(1), FPIX(1), FPIX(4), WROWS(0), WROWS(1), WPIX]


# =================================================================================================================================
# no device needed: the table against the restated dispatch
# =================================================================================================================================
def rows_ok(Cin, Cout):
    return Cin == 1 and Cout % 8 == 0 and 256 % (Cout // 8) == 0 and Cout <= 256


def first_blocks(P, Cout):
    """-> (workgroups, pixels per workgroup) of the per-pixel weight gradient; also the cap of the row-walking one"""
    up = lambda a, b: -(-a // b)
    ppb = 256 // (Cout // 4)
    per = max(up(up(P, 2048), ppb) * ppb, ppb)
    return up(P, per), per


def dispatch(r):
    """-> (kernel, partials): the kernel the entry launches for the row and, for a weight gradient, how many partial results
    the reduction sums (= workgroups of the first stage)"""
    b16 = r.st == "bf16"
    if r.entry == "raw":
        return FRAW(b16), None
    if r.entry == "fwd":
        return (FROWS(b16) if rows_ok(r.Cin, r.Cout) else FPIX(1 if r.Cin == 1 else 4)), None
    blocks, _ = first_blocks(r.N * r.H * r.W, r.Cout)
    if rows_ok(1, r.Cout):
        return WROWS(b16), min(units(r), blocks)
    return WPIX, blocks


def units(r):
    XS = 256 // (r.Cout // 8)
    return r.N * -(-r.H // FR_ROWS) * -(-r.W // XS)


@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_row_names_its_kernel(r):
    assert dispatch(r)[0] == r.kernel


def test_table_covers_every_kernel():
    named = {r.kernel for r in ROWS}
    missing = [k for k in REACHABLE if k not in named]
    assert not missing, "kernel instantiations without a row: " + ", ".join(missing)
    assert not named - set(REACHABLE), named - set(REACHABLE)
    # per-pixel forward <4>: every Cin and the channel counts at both ends; raw frames: both pixel types, every pad, every Cout
    p4 = [r for r in ROWS if r.kernel == FPIX(4)]
    assert {(r.Cin, r.Cout) for r in p4} >= {(ci, co) for ci in (2, 3, 4) for co in (4, 16, 64)} and {r.Cout for r in p4} >= {128, 256}
    rw = [r for r in ROWS if r.entry == "raw"]
    assert {r.opt["pix"] for r in rw} == {"u8", "u16"} and {(r.opt["pt"], r.opt["pl"]) for r in rw} == {(0, 0), (3, 0), (0, 5), (12, 7)}
    assert {r.Cout for r in rw} == {8, 64, 256} and {r.st for r in rw} == {"f32", "bf16"}
    assert {r.Cout for r in ROWS if r.kernel in (FROWS(0), FROWS(1))} == {8, 16, 32, 64, 128, 256}


def test_launch_geometry():
    """the shapes reach the paths they are in the table for"""
    geo = lambda id: (units(BY[id]), dispatch(BY[id])[1])
    assert geo("rows_wgrad_10_units_on_5") == (10, 5) and geo("rows_wgrad_16_units_on_1") == (16, 1)
    assert geo("rows_wgrad_6_units_on_3") == (6, 3)
    assert geo("rows_wgrad_42_partials") == (42, 42) and geo("rows_wgrad_32_partials") == (32, 32)
    assert geo("rows_wgrad_one_pixel_f32") == (1, 1)
    fewer_than_8 = [r.id for r in ROWS if r.entry == "wgrad" and dispatch(r)[1] < 8]
    assert len(fewer_than_8) >= 4
    r = BY["wpix_two_pixels_per_slot"]
    blocks, per = first_blocks(r.N * r.H * r.W, r.Cout)
    assert per == 2 * 256 and blocks == 1027 and 9 * r.N * r.H * r.W < CR.EXACT_LIMIT
    r = BY["pix4_grid_stride"]
    ppb = 256 // (r.Cout // 4)
    assert 8192 * ppb < r.N * r.H * r.W < 2 * 8192 * ppb
    r = BY["rows_fwd_w_xs_plus_1_f32"]
    assert r.W == 256 // (r.Cout // 8) + 1
    r = BY["rows_fwd_seam_off_unit_f32"]
    assert r.N > 1 and r.H % FR_ROWS and r.W % (256 // (r.Cout // 8))


# =================================================================================================================================
# data and references
# =================================================================================================================================
def _draw(rng, mode, shape, sigma=1.0):
    if mode == "exact":
        return rng.integers(-3, 4, size=shape).astype(np.float32)
    return (sigma * rng.normal(size=shape)).astype(np.float32)


def make_data(r, mode, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    cast = (lambda v: CR.as_exact(v).astype(np.float64)) if mode == "exact" else (lambda v: np.asarray(v, dtype=np.float64))
    d = {"mode": mode}
    if r.entry == "raw":
        o = r.opt
        top = 255 if o["pix"] == "u8" else 65535
        lo, hi = (int(v) for v in sorted(rng.choice(np.arange(1, top), size=2, replace=False)))
        if mode == "exact":
            frame = rng.choice([lo, hi], size=(o["H0"], o["W0"]))
            if o["H0"] * o["W0"] == 1:
                lo = 0                                     # one pixel: it is the maximum, the minimum must differ
        else:
            frame = rng.integers(lo, hi + 1, size=(o["H0"], o["W0"]))
        frame = frame.astype(np.uint8 if o["pix"] == "u8" else np.uint16)
        fmin, fmax = (lo, int(frame.max())) if o["H0"] * o["W0"] == 1 else (int(frame.min()), int(frame.max()))
        if fmax == fmin:
            fmin = fmax - 1
        d["frame"], d["minmax"] = frame, np.array([~np.uint32(fmin), fmax], dtype=np.uint32)
        # the header's host formula in fp32 numpy; the frame padding has the value `min`: exactly -1
        nrm = np.float32(2) * (frame.astype(np.float32) - np.float32(fmin)) / np.float32(fmax - fmin) - np.float32(1)
        assert nrm.dtype == np.float32
        x = np.full((1, r.H, r.W, 1), -1.0, dtype=np.float32)
        x[0, o["pt"]:, o["pl"]:, 0] = nrm
    else:
        x = _draw(rng, mode, (r.N, r.H, r.W, r.Cin))
        x4 = np.zeros((r.N, r.H, r.W, 4), dtype=np.float32)
        x4[..., :r.Cin] = x
        if r.Cin == 1:                                     # junk the Cin = 1 kernels must ignore
            x4[..., 1:] = rng.choice([-5.0, 3.0, 7.0], size=(r.N, r.H, r.W, 3))
        d["x4"] = x4
    d["x"] = x
    if r.entry == "wgrad":
        dz = _draw(rng, mode, (r.N, r.H, r.W, r.Cout))
        if r.st == "bf16":
            dz = CR.round_bf16(dz).astype(np.float32)
        d["dz"] = dz
        d["ref"], d["S"] = CR.wgrad(cast(dz), [cast(x)], 3, 1)
    else:
        d["w"] = _draw(rng, mode, (r.Cout, r.Cin, 3, 3), 1.0 if mode == "exact" else 1.0 / np.sqrt(9 * r.Cin))
        d["bias"] = _draw(rng, mode, (r.Cout,))
        ref, S = CR.conv_fwd([cast(x)], cast(d["w"]), cast(d["bias"]))
        d["ref"], d["S"] = ref.reshape(-1, r.Cout), S.reshape(-1, r.Cout)
    if mode == "exact":
        d["ref"], d["S"] = CR.as_exact(d["ref"]), CR.as_exact(d["S"])
        CR.assert_exact(d["S"])
    return d


def torch_fp32(r, d):
    x = _t32(d["x"]).permute(0, 3, 1, 2).contiguous()
    if r.entry == "wgrad":
        w = torch.zeros(r.Cout, 1, 3, 3, requires_grad=True)
        F.conv2d(x, w, None, padding=1).backward(_t32(d["dz"]).permute(0, 3, 1, 2).contiguous())
        return w.grad.numpy()
    y = F.conv2d(x, _t32(d["w"]), _t32(d["bias"]), padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, r.Cout).numpy()


# =================================================================================================================================
# launches
# =================================================================================================================================
@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _eng()[2]


def _dev(a, bf16=False):
    t = _t32(a).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def _prime(lib, kernel):
    """launch another kernel of the file so that mseg_last_kernel() cannot still hold `kernel` from an earlier call"""
    co = 8 if kernel == FPIX(1) else 4
    x4, w, z = torch.zeros(4, device="cuda"), torch.zeros(co * 9, device="cuda"), torch.zeros(co, device="cuda")
    assert lib.mseg_first_conv_fwd(x4.data_ptr(), w.data_ptr(), None, 1, 1, 1, 1, co, z.data_ptr(), 0, _stream()) == 0
    _sync()
    assert lib.mseg_last_kernel().decode() == (FROWS(0) if co == 8 else FPIX(1)) != kernel


def launch(lib, r, d):
    """-> the result as fp32 values (z: [N H W][Cout]; dW: (Cout, 1, 3, 3)) after the sentinel checks"""
    b16 = r.st == "bf16"
    _prime(lib, r.kernel)
    keep = []
    if r.entry == "wgrad":
        x4, dz = _dev(d["x4"]), _dev(d["dz"], b16)
        need = lib.mseg_first_wgrad_workspace_bytes(r.N, r.H, r.W, r.Cout)
        assert need > 0 and need % 4 == 0
        ws, dW = Guarded(1, need // 4, need // 4), Guarded(r.Cout, 9, 9)
        rc = lib.mseg_first_wgrad(x4.data_ptr(), dz.data_ptr(), int(b16), r.N, r.H, r.W, r.Cout, dW.ptr, ws.ptr, _stream())
        assert rc == 0, f"mseg_first_wgrad returned {rc} (hipError {lib.mseg_last_hip_error()})"
        assert lib.mseg_last_kernel().decode() == r.kernel
        ws.take()
        return dW.take().reshape(r.Cout, 1, 3, 3)
    w, bias = _dev(d["w"]), _dev(d["bias"])
    z = Guarded(r.N * r.H * r.W, r.Cout, r.Cout, bf16=b16)
    if r.entry == "raw":
        o = r.opt
        word = np.int8 if o["pix"] == "u8" else np.int16
        frame = torch.from_numpy(d["frame"].view(word)).cuda()
        mm = torch.from_numpy(d["minmax"].view(np.int32)).cuda()
        keep += [frame, mm]
        rc = lib.mseg_first_conv_fwd_raw(frame.data_ptr(), 0 if o["pix"] == "u8" else 1, o["H0"], o["W0"], o["pt"], o["pl"],
                                         mm.data_ptr(), w.data_ptr(), bias.data_ptr(), r.Cout, z.ptr, int(b16), _stream())
    else:
        x4 = _dev(d["x4"])
        keep.append(x4)
        rc = lib.mseg_first_conv_fwd(x4.data_ptr(), w.data_ptr(), bias.data_ptr(), r.N, r.H, r.W, r.Cin, r.Cout, z.ptr, int(b16),
                                     _stream())
    assert rc == 0, f"{r.entry} returned {rc} (hipError {lib.mseg_last_hip_error()})"
    assert lib.mseg_last_kernel().decode() == r.kernel
    return z.take()


def _seed(r, extra=0):
    return 1000 * ROW_IDS.index(r.id) + extra


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_exact(lib, r):
    """small integers: bit-equal to the int64 reference (a bf16 z: to its bf16 rounding), every sentinel intact"""
    d = make_data(r, "exact", _seed(r))
    got = launch(lib, r, d).astype(np.float64)
    ref = d["ref"].astype(np.float64)
    if r.st == "bf16" and r.entry != "wgrad":
        ref = CR.round_bf16(ref)
    wrong = np.argwhere(~(got == ref))
    assert wrong.shape[0] == 0, (f"{r.id}: {wrong.shape[0]} of {ref.size} elements differ; first at {wrong[0].tolist()}: "
                                 f"got {got[tuple(wrong[0])]}, expected {ref[tuple(wrong[0])]}")


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_float(lib, r):
    """random operands: per element within max(4 e_ref, floor) and within the worst-case dot-product bound, relative to S"""
    K = r.N * r.H * r.W if r.entry == "wgrad" else 9 * r.Cin + 1
    bound = (K + 32) * U
    fam = r.kernel.split("<")[0]
    floor = FLOOR[fam] * U
    d = make_data(r, "float", _seed(r, 1))
    got = launch(lib, r, d).astype(np.float64)
    S = np.maximum(d["S"], TINY)
    err = np.abs(got - d["ref"])
    if r.st == "bf16" and r.entry != "wgrad":               # the stored value is the bf16 rounding of the fp32 result
        err = np.maximum(err - 0.5 * CR.bf16_ulp(np.abs(d["ref"]) + bound * S), 0.0)
    e = err / S
    e_ref = float((np.abs(torch_fp32(r, d).astype(np.float64) - d["ref"]) / S).max())
    worst = np.unravel_index(np.argmax(np.where(np.isnan(e), np.inf, e)), e.shape)
    print(f"FIRST {r.id} {fam} e_hip={e.max() / U:.3f}u e_ref={e_ref / U:.3f}u bound={bound / U:.0f}u")
    assert not np.isnan(got).any(), f"{r.id}: NaN left in the destination at {worst}"
    assert e.max() <= max(4 * e_ref, floor), \
        f"{r.id}: e = {e.max() / U:.2f} u at {worst} (torch fp32 {e_ref / U:.2f} u, floor {floor / U:.2f} u)"
    assert e.max() <= bound, f"{r.id}: e = {e.max() / U:.2f} u at {worst} beyond the bound {bound / U:.0f} u"


@pytest.mark.gpu
def test_refusals_write_nothing(lib):
    """MSEG_EINVAL: nothing is launched, z / dW stay bit-unchanged and mseg_last_kernel() keeps the last launched name"""
    N, H, W = 2, 5, 7
    x4 = torch.zeros((N, H, W, 4), device="cuda")
    w, bias = torch.ones(512 * 4 * 9, device="cuda"), torch.ones(512, device="cuda")
    dz = torch.ones(N * H * W * 512, device="cuda")
    z, dW, ws = Guarded(N * H * W, 512, 512), Guarded(512, 9, 9), Guarded(1, 1 << 16, 1 << 16)
    _prime(lib, FROWS(0))
    st = _stream()
    fwd_ = lambda cin, cout, zd, zp=z.ptr: lib.mseg_first_conv_fwd(x4.data_ptr(), w.data_ptr(), bias.data_ptr(), N, H, W, cin, cout,
                                                                   zp, zd, st)
    for cout in (12, 0, 512, -8, 6):                           # 12: a multiple of 4 whose quads do not tile 256 threads
        assert fwd_(1, cout, 0) == EINVAL and fwd_(3, cout, 0) == EINVAL, cout
        assert lib.mseg_first_wgrad_workspace_bytes(N, H, W, cout) == 0, cout
        assert lib.mseg_first_wgrad(x4.data_ptr(), dz.data_ptr(), 0, N, H, W, cout, dW.ptr, ws.ptr, st) == EINVAL, cout
    for cin in (0, 5):
        assert fwd_(cin, 64, 0) == EINVAL, cin
    for zd in (2, -1):                                         # a storage other than fp32 / bf16
        assert fwd_(1, 64, zd) == EINVAL
        assert lib.mseg_first_wgrad(x4.data_ptr(), dz.data_ptr(), zd, N, H, W, 64, dW.ptr, ws.ptr, st) == EINVAL
    for n, h, ww in ((0, H, W), (N, 0, W), (N, H, 0)):
        assert lib.mseg_first_wgrad_workspace_bytes(n, h, ww, 64) == 0
        assert lib.mseg_first_conv_fwd(x4.data_ptr(), w.data_ptr(), bias.data_ptr(), n, h, ww, 1, 64, z.ptr, 0, st) == EINVAL
    assert fwd_(1, 64, 0, None) == EINVAL                      # a NULL destination
    frame = torch.zeros(H * W, dtype=torch.uint8, device="cuda")
    mm = torch.from_numpy(np.array([~np.uint32(0), 9], dtype=np.uint32).view(np.int32)).cuda()
    raw_ = lambda pix, cout, zd: lib.mseg_first_conv_fwd_raw(frame.data_ptr(), pix, H, W, 0, 0, mm.data_ptr(), w.data_ptr(),
                                                             bias.data_ptr(), cout, z.ptr, zd, st)
    assert raw_(0, 4, 0) == EINVAL                             # the raw form has no per-pixel kernel
    assert raw_(0, 12, 0) == EINVAL and raw_(0, 64, 2) == EINVAL and raw_(3, 64, 0) == EINVAL
    assert z.untouched() and dW.untouched() and ws.untouched()
    assert lib.mseg_last_kernel().decode() == FPIX(1)          # what _prime launched: a refused call names nothing
    assert raw_(0, 64, 0) == 0 and not z.untouched()           # the same call with a legal Cout is accepted
