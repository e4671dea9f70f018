"""GPU (MI355X): every fp32 instantiation of the convolution family (microbeseg_amd/csrc/igemm.hip, wgrad.hip) through the C ABI, pinned
to its kernel and compared element by element with the plain references of tests/conv_ref.py.

ONE table (ROWS).  A row names the operation, the shapes, how each source is transformed on load, the destination form and
the kernel instantiation the dispatch must take.  For every row, before the launch, engine.igemm_query / engine.wgrad_query
(and mseg_*_query on the very descriptor that is launched) must name exactly that kernel, and after the launch
mseg_last_kernel() must too.  test_table_covers_every_reachable_instantiation walks the table without a device.

Two modes per row:

  exact   small-integer operands (|v| <= 3), integer scale / shift with a nonzero shift (a padding pixel that is transformed
          instead of zeroed shows), activations none / relu only (a row whose kernel is the any-activation variant runs its
          relu sibling here: column `xkernel`).  conv_ref asserts that the sum of magnitudes S of every output stays below
          2^24, so every partial sum is an integer fp32 holds exactly and the result must equal the int64 reference BIT FOR
          BIT whatever the order of summation or the split-K.  Finds wrong taps, borders, parity classes, channel and tile
          tails exactly.
  float   N(0, 1) operands (+1.5 on channel 0 of the first source), scale ~ 1, random shift, every activation the row's
          kernel takes (none / relu swapped where a table keeps the transform alive; all three of leakyrelu, elu, mish on the
          any-activation kernels).  Per element e = |got - ref64| / max(S, 2^-100) must satisfy
              e <= max(4 e_ref, FLOOR[family])   and   e <= (K + 32) 2^-24
          e_ref = the largest e of torch's CPU fp32 result of the same operation on the same inputs.  K is the length of the
          dot product an output element is: T * Cin (taps x input channels) for the convolutions and, deliberately not that
          product, NB * Hp * Wp — the pixels summed over — for the weight gradients, whose sums run over pixels and not over
          taps and channels.  K 2^-24 is the worst-case bound of an fp32 dot product in any order, 32 2^-24 covers the
          operand transform (activation, multiply, add on each side).  No element is exempt.

Buffers: every destination sits inside a larger buffer — 256 sentinel words before and after it and sentinel columns where
the leading dimension exceeds the channels — and every sentinel must come back bit-unchanged.  A destination that is not
accumulated into starts as NaN (old content must leave no trace), an accumulating one must end as base + result.  Where the
API refuses a descriptor (MSEG_EINVAL) nothing may be written.

The floors and the errors measured on the MI355X per kernel family stand beside FLOOR below.

Dead instantiations: wgrad_halo_kernel<2, *> and <3, *> (pixel blocks 8 x 4 / 4 x 8) are compiled but cannot be reached.
For a row length that is no multiple of 16 the all-taps kernel wgrad_halo9_kernel picks the same block shape and applies
the same 80 % rule to the same numbers, so whenever wgrad_halo_kernel would qualify the all-taps kernel wins
(test_dead_wgrad_halo_instantiations asks the dispatch for every small shape).

The three reductions behind the weight gradients are helper launches the query does not name; the rows wred_* select them
through `splits` and the workspace: < 32 splits wgrad_reduce_kernel<4>, >= 32 wgrad_reduce_many_kernel, and >= 32 with a
workspace that is not 16-byte aligned (MsegWgrad.ws is a float*: 4-byte alignment is valid) wgrad_reduce_kernel<16>.  Its
other condition, Nch % 4 != 0, is refused by the argument check (test_refused_descriptors_write_nothing)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conv_table import (EINVAL, U, TINY, _b, row, is_wgrad, geom, epilogue_row_mode, float_variants, exact_acts, engine_query,
                        make_data, torch_fp32, build_igemm, build_wgrad, launch, family, _eng, _name, _stream)

# float mode: FLOOR[family] in units of 2^-24, about twice the largest e the kernels of the family showed on the MI355X over
# all float runs of this table (175 launches); beside it what torch's CPU fp32 showed on the same inputs and the largest
# share of the worst-case bound (K + 32) 2^-24 any element used.  All relative to S:
#   family               runs   e_hip    e_ref    e_hip / bound
#   igemm_halo_kernel     19    4.29     5.39     0.041
#   igemm_fast_kernel     44    4.43     4.49     0.092
#   igemm_kernel          18    4.38     3.56     0.030
#   wgrad_halo_kernel     12    3.13     3.16     0.049
#   wgrad_halo9_kernel    18    3.46     4.79     0.054
#   wgrad_kernel          19    3.09     4.67     0.070
#   wgrad_fast_kernel     45    7.03     5.40     0.160
FLOOR = {"igemm_halo_kernel": 9.0, "igemm_fast_kernel": 9.0, "igemm_kernel": 9.0, "wgrad_halo_kernel": 6.5,
         "wgrad_halo9_kernel": 7.0, "wgrad_kernel": 6.5, "wgrad_fast_kernel": 14.0}


# =================================================================================================================================
# the table
# =================================================================================================================================
def HALO(bn, tr): return f"igemm_halo_kernel<{bn}, {tr}>"
def FAST(bn, tr, ps, sb): return f"igemm_fast_kernel<128, {bn}, {tr}, {_b(ps)}, {_b(sb)}>"
def GEN(bn, ps, ga): return f"igemm_kernel<128, {bn}, {_b(ps)}, {_b(ga)}>"
def WH(t, q): return f"wgrad_halo_kernel<{t}, {q}>"
def W9(t, q): return f"wgrad_halo9_kernel<{t}, {q}>"
def WG(kw, ga, ps): return f"wgrad_kernel<{kw}, {_b(ga)}, {_b(ps)}>"
def WF(kw, p, q): return f"wgrad_fast_kernel<{kw}, {p}, {q}>"


ROWS = [
    # ---- igemm_halo_kernel<BN, TR>: 3x3 stride 1 on 128-pixel tiles of width 64 .. 4 --------------------------------------------
    row("halo_w64_plain", "conv", 1, [8], 8, 4, 64, HALO(64, 0)),
    row("halo_w32_affine", "conv", 1, [8], 72, 8, 32, HALO(128, 1), acts=["relu"], tabs=["c"]),
    row("halo_w16_overhang", "conv", 1, [32], 64, 20, 16, HALO(64, 1), acts=["relu"], tabs=["s"], dest="acc"),
    row("halo_w8_overhang_mish", "conv", 1, [16], 16, 40, 40, HALO(64, 2), HALO(64, 1), acts=["mish"], tabs=["s"]),
    row("halo_w4_overhang_ld", "conv", 1, [8], 6, 28, 12, HALO(64, 0), dest="ld", ldpad=2),      # Ngemm % 4 != 0, ld0 8
    row("halo_dgrad_wide_plain", "dgrad", 2, [8], 72, 8, 16, HALO(128, 0), dest="split", split=40),
    row("halo_wide_elu", "conv", 1, [8], 136, 16, 8, HALO(128, 2), HALO(128, 1), acts=["elu"], tabs=["c"]),
    row("halo_two_sources", "conv", 2, [32, 8], 16, 8, 16, HALO(64, 1), acts=["relu", "none"], tabs=["c", "s"]),
    row("halo_splitk_mish", "conv", 1, [128], 8, 8, 16, HALO(64, 2), HALO(64, 1), acts=["mish"], tabs=["c"], dest="split",
        split=4, splitk=2),
    row("halo_splitk_plain_ld", "dgrad", 1, [128], 12, 8, 16, HALO(64, 0), dest="ld", ldpad=4, splitk=2),
    # ---- igemm_fast_kernel<128, BN, TR, PS, SB = false>: 3x3 gathers that are no halo shape -------------------------------------
    row("fast_s2_odd_plain", "conv", 2, [8], 8, 9, 7, FAST(64, 0, 0, 0), stride=2),
    row("fast_dgrad_wide", "dgrad", 1, [72], 136, 12, 20, FAST(128, 0, 0, 0), dest="acc"),
    row("fast_affine", "conv", 1, [128], 64, 8, 8, FAST(64, 1, 0, 0), acts=["relu"], tabs=["c"]),
    row("fast_two_sources", "conv", 2, [32, 8], 40, 20, 12, FAST(64, 1, 1, 0), acts=["relu", "none"], tabs=["s", "c"]),
    row("fast_s2_wide_relu", "conv", 1, [8], 72, 10, 14, FAST(128, 1, 0, 0), stride=2, acts=["relu"]),
    row("fast_s2_wide_persample", "conv", 2, [8], 72, 6, 10, FAST(128, 1, 1, 0), stride=2, tabs=["s"], dest="ld", ldpad=4),
    row("fast_odd_leaky", "conv", 1, [8], 8, 5, 7, FAST(64, 2, 0, 0), FAST(64, 1, 0, 0), acts=["leakyrelu"], tabs=["c"]),
    row("fast_s2_mish_persample", "conv", 2, [12], 20, 8, 8, FAST(64, 2, 1, 0), FAST(64, 1, 1, 0), stride=2, acts=["mish"],
        tabs=["s"]),
    row("fast_wide_elu", "conv", 1, [8], 68, 6, 10, FAST(128, 2, 0, 0), FAST(128, 1, 0, 0), acts=["elu"]),
    row("fast_s2_wide_mish_persample", "conv", 2, [8], 68, 7, 9, FAST(128, 2, 1, 0), FAST(128, 1, 1, 0), stride=2,
        acts=["mish"], tabs=["s"]),
    # ---- igemm_fast_kernel<..., SB = true>: short K (ConvTranspose and its gradient, stride-2 data gradients) --------------------
    row("fast_parity_w32", "dgrad", 1, [8], 8, 8, 32, FAST(64, 0, 0, 1), stride=2),               # parity order, row mode 0
    row("fast_parity_w16", "dgrad", 1, [8], 8, 16, 16, FAST(64, 0, 0, 1), stride=2, dest="split", split=4),    # row mode 3
    row("fast_convT_dgrad_wide", "convT_dgrad", 1, [8], 72, 8, 12, FAST(128, 0, 0, 1)),
    row("fast_convT_dgrad", "convT_dgrad", 2, [8], 8, 6, 10, FAST(64, 0, 0, 1), dest="acc"),
    row("fast_convT_affine", "convT", 1, [16], 8, 5, 7, FAST(64, 1, 0, 1), acts=["relu"], tabs=["c"]),
    row("fast_convT_persample", "convT", 3, [16], 8, 6, 10, FAST(64, 1, 1, 1), tabs=["s"]),       # scatter across images, mode 2
    row("fast_convT_wide_relu", "convT", 1, [16], 20, 4, 8, FAST(128, 1, 0, 1), acts=["relu"]),
    row("fast_convT_wide_persample", "convT", 2, [8], 24, 3, 5, FAST(128, 1, 1, 1), acts=["relu"], tabs=["s"]),
    row("fast_convT_elu", "convT", 1, [8], 4, 6, 6, FAST(64, 2, 0, 1), FAST(64, 1, 0, 1), acts=["elu"], tabs=["c"]),
    row("fast_convT_mish_persample", "convT", 2, [8], 12, 4, 6, FAST(64, 2, 1, 1), FAST(64, 1, 1, 1), acts=["mish"], tabs=["s"]),
    row("fast_convT_wide_mish_w32", "convT", 1, [16], 40, 4, 32, FAST(128, 2, 0, 1), FAST(128, 1, 0, 1), acts=["mish"],
        tabs=["c"]),                                                                               # scatter, row mode 0
    row("fast_convT_wide_leaky_persample", "convT", 2, [16], 40, 2, 6, FAST(128, 2, 1, 1), FAST(128, 1, 1, 1),
        acts=["leakyrelu"], tabs=["s"]),
    # ---- igemm_kernel<128, BN, PS, GA>: the generic kernel ---------------------------------------------------------------------
    row("gen_two_sources_mish", "conv", 2, [8, 24], 136, 12, 20, GEN(128, 0, 1), GEN(128, 0, 0), acts=["mish", "none"],
        tabs=["c", "c"]),
    row("gen_parity_straddle", "dgrad", 1, [8], 8, 6, 10, GEN(64, 0, 0), stride=2),               # 60-pixel classes: row mode 4
    row("gen_two_sources_persample", "conv", 2, [8, 24], 40, 7, 9, GEN(64, 1, 0), acts=["relu", "none"], tabs=["s", None]),
    row("gen_two_sources_elu", "conv", 1, [8, 8], 8, 6, 6, GEN(64, 0, 1), GEN(64, 0, 0), acts=["elu", "none"], tabs=["c", None]),
    row("gen_s2_mish_persample", "conv", 2, [8, 24], 16, 9, 8, GEN(64, 1, 1), GEN(64, 1, 0), stride=2, acts=["mish", "relu"],
        tabs=["s", "c"]),
    row("gen_dgrad_s2_linear_odd", "dgrad", 1, [8], 72, 5, 6, GEN(128, 0, 0), stride=2, out_hw=(9, 11), parity=False,
        dest="acc"),
    row("gen_wide_persample", "conv", 2, [8, 24], 72, 5, 8, GEN(128, 1, 0), acts=["none", "relu"], tabs=["s", "c"]),
    row("gen_wide_leaky_persample", "conv", 2, [8, 24], 136, 6, 6, GEN(128, 1, 1), GEN(128, 1, 0), acts=["leakyrelu", "none"],
        tabs=["s", None], dest="split", split=72),
    # ---- wgrad_halo_kernel<TWL, QTR>: row length a multiple of 16, H in {1, 2, 3, 5, 6, 9}; 16 output x 8 input channels -------
    row("wh_w32", "wgrad3", 2, [8], 16, 6, 32, WH(5, 1), acts=["relu"], tabs=["c"]),
    row("wh_w16_plain", "wgrad3", 1, [8], 16, 6, 16, WH(4, 0)),
    row("wh_w16_mish", "wgrad3", 1, [8], 16, 2, 16, WH(4, 2), WH(4, 1), acts=["mish"], tabs=["c"]),
    row("wh_w16_overhang_persample", "wgrad3", 2, [8], 16, 5, 16, WH(4, 1), acts=["relu"], tabs=["s"]),
    row("wh_w32_one_row", "wgrad3", 1, [8], 16, 1, 32, WH(5, 0)),
    row("wh_w32_elu", "wgrad3", 2, [8], 16, 3, 32, WH(5, 2), WH(5, 1), acts=["elu"]),
    # ---- wgrad_halo9_kernel<TWL, QTR>: all nine taps per workgroup ----------------------------------------------------------------
    row("w9_w12", "wgrad3", 1, [8], 16, 16, 12, W9(2, 1), acts=["relu"], tabs=["c"]),
    row("w9_w4_plain", "wgrad3", 2, [8], 16, 8, 4, W9(2, 0)),
    row("w9_w12_mish_persample", "wgrad3", 1, [12], 20, 8, 12, W9(2, 2), W9(2, 1), acts=["mish"], tabs=["s"]),
    row("w9_w8_plain", "wgrad3", 1, [8], 16, 4, 8, W9(3, 0)),
    row("w9_w8_overhang_persample", "wgrad3", 2, [8], 16, 10, 8, W9(3, 1), acts=["relu"], tabs=["s"]),
    row("w9_w24_leaky", "wgrad3", 1, [8], 16, 8, 24, W9(3, 2), W9(3, 1), acts=["leakyrelu"], tabs=["c"]),
    row("w9_two_sources", "wgrad3", 1, [64, 8], 8, 4, 8, W9(3, 1), acts=["relu", "none"], tabs=["c", None]),
    # ---- wgrad_kernel<KW, GA, PS>: the generic kernel ---------------------------------------------------------------------------
    row("wg_persample", "wgrad3", 2, [8], 16, 10, 14, WG(3, 0, 1), acts=["relu"], tabs=["s"]),
    row("wg_persample_mish", "wgrad3", 2, [8], 16, 10, 14, WG(3, 1, 1), WG(3, 0, 1), acts=["mish"], tabs=["s"]),
    row("wg_two_sources", "wgrad3", 2, [8, 8], 16, 8, 8, WG(3, 0, 0), acts=["relu", "none"], tabs=["c", None]),
    row("wg_two_sources_s2_elu", "wgrad3", 1, [8, 8], 16, 3, 4, WG(3, 1, 0), WG(3, 0, 0), stride=2, q_hw=(5, 7),
        acts=["elu", "none"]),
    row("wg_convT_persample_P", "wgrad2", 2, [8], 16, 6, 10, WG(2, 0, 1), pact="relu", ptab="s"),
    row("wg_convT_persample_mish_P", "wgrad2", 2, [8], 16, 6, 10, WG(2, 1, 1), WG(2, 0, 1), pact="mish", ptab="s"),
    row("wg_convT_two_sources", "wgrad2", 1, [8, 8], 16, 3, 5, WG(2, 0, 0)),
    row("wg_convT_two_sources_elu_P", "wgrad2", 1, [8, 8], 16, 3, 5, WG(2, 1, 0), WG(2, 0, 0), pact="elu", ptab="c"),
    # ---- wgrad_fast_kernel<KW, PTR, QTR>: linear 32-pixel steps ------------------------------------------------------------------
    row("wf_s2_plain", "wgrad3", 1, [8], 16, 4, 8, WF(3, 0, 0), stride=2),
    row("wf_odd_affine", "wgrad3", 2, [8], 16, 5, 6, WF(3, 0, 1), acts=["relu"], tabs=["c"]),
    row("wf_s2_mish_persample", "wgrad3", 1, [16], 8, 4, 8, WF(3, 0, 2), WF(3, 0, 1), stride=2, acts=["mish"], tabs=["s"]),
    row("wf_convT_plain", "wgrad2", 2, [8], 16, 3, 5, WF(2, 0, 0)),
    row("wf_convT_persample_P", "wgrad2", 1, [8], 16, 4, 8, WF(2, 1, 0), pact="relu", ptab="s"),
    row("wf_convT_mish_P", "wgrad2", 1, [8], 16, 4, 8, WF(2, 2, 0), WF(2, 1, 0), pact="mish", ptab="c"),     # 16 -> 8 channels
    row("wf_P1_Q0", "wgrad3", 1, [8], 16, 6, 6, WF(3, 1, 0), pact="relu", ptab="c"),
    row("wf_P1_Q1", "wgrad3", 2, [8], 16, 4, 8, WF(3, 1, 1), pact="none", ptab="s", acts=["relu"], tabs=["c"]),
    row("wf_P1_Q2", "wgrad3", 1, [8], 16, 5, 7, WF(3, 1, 2), WF(3, 1, 1), pact="relu", acts=["mish"]),
    row("wf_P2_Q0", "wgrad3", 1, [8], 16, 4, 4, WF(3, 2, 0), WF(3, 1, 0), pact="elu"),
    row("wf_P2_Q1_s2", "wgrad3", 1, [8], 16, 3, 4, WF(3, 2, 1), WF(3, 1, 1), stride=2, pact="mish", ptab="c", acts=["relu"]),
    row("wf_P2_Q2", "wgrad3", 1, [8], 8, 6, 10, WF(3, 2, 2), WF(3, 1, 1), pact="leakyrelu", acts=["mish"], tabs=["c"]),
    # (a ConvTranspose output gradient that is transformed on load: not issued by the networks, reachable through the C ABI)
    row("wf_convT_Q1", "wgrad2", 1, [8], 16, 4, 8, WF(2, 0, 1), acts=["relu"], tabs=["c"]),
    row("wf_convT_Q2", "wgrad2", 2, [8], 16, 3, 5, WF(2, 0, 2), WF(2, 0, 1), acts=["mish"]),
    row("wf_convT_P1_Q1", "wgrad2", 1, [8], 16, 4, 8, WF(2, 1, 1), pact="relu", ptab="s", acts=["relu"]),
    row("wf_convT_P1_Q2", "wgrad2", 1, [8], 8, 5, 6, WF(2, 1, 2), WF(2, 1, 1), pact="relu", acts=["elu"], tabs=["c"]),
    row("wf_convT_P2_Q1", "wgrad2", 2, [8], 16, 2, 6, WF(2, 2, 1), WF(2, 1, 1), pact="mish", tabs=["c"]),
    row("wf_convT_P2_Q2", "wgrad2", 1, [12], 8, 4, 8, WF(2, 2, 2), WF(2, 1, 1), pact="elu", ptab="c", acts=["leakyrelu"]),
    # ---- the reductions behind the weight gradients, selected by `splits` in the descriptor --------------------------------------
    row("wred_few_splits", "wgrad3", 2, [8], 16, 8, 8, WF(3, 0, 0), stride=2, splits=3),          # wgrad_reduce_kernel<4>
    row("wred_many_splits_store5", "wgrad3", 2, [8], 16, 32, 32, W9(3, 1), acts=["relu"], tabs=["c"], splits=32,
        nch_store=5),                                                                              # wgrad_reduce_many_kernel
    # workspace 4 bytes off 16-byte alignment; 20 channels = one full group of 16 and a tail of 4, 18 of them stored
    row("wred_many_splits_unaligned_ws", "wgrad3", 2, [20], 16, 32, 32, W9(3, 1), acts=["relu"], tabs=["c"], splits=32,
        nch_store=18, ws_off=4),                                                                   # wgrad_reduce_kernel<16>
]
ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)

# every fp32 instantiation the dispatch can reach
REACHABLE = (
    [HALO(bn, tr) for bn in (64, 128) for tr in (0, 1, 2)]
    + [FAST(bn, tr, ps, sb) for bn in (64, 128) for tr in (0, 1, 2) for ps in ((0,) if tr == 0 else (0, 1)) for sb in (0, 1)]
    + [GEN(bn, ps, ga) for bn in (64, 128) for ps in (0, 1) for ga in (0, 1)]
    # wgrad_halo_kernel<2, *> and <3, *> are dead (module docstring): not listed
    + [WH(t, q) for t in (4, 5) for q in (0, 1, 2)]
    + [W9(t, q) for t in (2, 3) for q in (0, 1, 2)]
    + [WG(kw, ga, ps) for kw in (3, 2) for ga in (0, 1) for ps in (0, 1)]
    + [WF(kw, p, q) for kw in (3, 2) for p in (0, 1, 2) for q in (0, 1, 2)]
)


# =================================================================================================================================
# no device needed: the table against the dispatch
# =================================================================================================================================
@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_row_names_its_kernel(r):
    """the dispatch takes the kernel the table says, in both modes and for every activation of the float mode"""
    xa, xp = exact_acts(r)
    got = engine_query(r, xa, xp)
    assert got is not None and got.name == r.xkernel, (r.id, "exact", got)
    for acts, pact in float_variants(r):
        got = engine_query(r, acts, pact)
        assert got is not None and got.name == r.kernel, (r.id, acts, pact, got)


def test_table_covers_every_reachable_instantiation():
    named = {r.kernel for r in ROWS} | {r.xkernel for r in ROWS}
    missing = [k for k in REACHABLE if k not in named]
    assert not missing, "reachable instantiations without a row: " + ", ".join(missing)
    unknown = sorted(named - set(REACHABLE))
    assert not unknown, "rows expect kernels that are not in the reachable list: " + ", ".join(unknown)
    modes = {epilogue_row_mode(r) for r in ROWS if not is_wgrad(r)}
    assert modes == {0, 1, 2, 3, 4}, f"igemm_epilogue row modes without a row: {sorted({0, 1, 2, 3, 4} - modes)}"
    # each row mode on the kernel family that uses it in the networks: scatter (2, 0) and parity (0, 3) on the fast kernel,
    # the straddling tile (4) on the generic one
    by = {r.id: r for r in ROWS}
    assert epilogue_row_mode(by["fast_convT_persample"]) == 2 and epilogue_row_mode(by["fast_convT_wide_mish_w32"]) == 0
    assert epilogue_row_mode(by["fast_parity_w32"]) == 0 and epilogue_row_mode(by["fast_parity_w16"]) == 3
    assert epilogue_row_mode(by["gen_parity_straddle"]) == 4
    widths = set()
    for r in ROWS:
        if r.kernel.startswith("igemm_halo_kernel"):
            tw = 64
            while r.W % tw:
                tw //= 2
            widths.add(tw)
    assert widths == {4, 8, 16, 32, 64}, widths


def test_dead_wgrad_halo_instantiations():
    """wgrad_halo_kernel<2, *> / <3, *> are never chosen: for W % 16 != 0 the all-taps kernel applies the same 80 % rule to
    the same block shape and wins.  Every small shape is asked; W % 16 == 0 does reach <4, *> / <5, *>."""
    seen = set()
    for W in range(4, 132, 4):
        for H in range(1, 70):
            for N in (1, 3):
                r = row("probe", "wgrad3", N, [8], 16, H, W, "")
                seen.add(engine_query(r, ["none"], "none").name)
    assert any(k.startswith("wgrad_halo_kernel<4") for k in seen) and any(k.startswith("wgrad_halo_kernel<5") for k in seen)
    assert not [k for k in seen if k.startswith("wgrad_halo_kernel<2") or k.startswith("wgrad_halo_kernel<3")], seen


# =================================================================================================================================
# the tests
# =================================================================================================================================
@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _eng()[2]


def _seed(r, extra=0):
    return 1000 * ROW_IDS.index(r.id) + extra if r.id in ROW_IDS else extra


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_exact(gpu, r):
    """small integers: the result equals the int64 reference bit for bit, every sentinel is intact"""
    acts, pact = exact_acts(r)
    d = make_data(r, "exact", acts, pact, _seed(r))
    got = launch(r, d, r.xkernel).astype(np.float64)
    ref = d["ref"].astype(np.float64)
    wrong = np.argwhere(~(got == ref))                      # a NaN left in the destination is wrong too
    assert wrong.shape[0] == 0, (f"{r.id}: {wrong.shape[0]} of {ref.size} elements differ; first at {wrong[0].tolist()}: "
                                 f"got {got[tuple(wrong[0])]}, expected {ref[tuple(wrong[0])]}")


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_float(gpu, r):
    """random operands: per element within max(4 e_ref, floor) and within the worst-case dot-product bound, relative to S"""
    bound = (geom(r)["dot"] + 32) * U
    floor = FLOOR[family(r.kernel)] * U
    for i, (acts, pact) in enumerate(float_variants(r)):
        d = make_data(r, "float", acts, pact, _seed(r, 1 + i))
        got = launch(r, d, r.kernel).astype(np.float64)
        S = np.maximum(d["S"], TINY)
        e = np.abs(got - d["ref"]) / S
        e_ref = float((np.abs(torch_fp32(r, d).astype(np.float64) - d["ref"]) / S).max())
        worst = np.unravel_index(np.argmax(np.where(np.isnan(e), np.inf, e)), e.shape)
        print(f"CONVFP32 {r.id} {family(r.kernel)} acts={','.join(acts)}/{pact} e_hip={e.max() / U:.3f}u "
              f"e_ref={e_ref / U:.3f}u bound={bound / U:.0f}u")
        assert not np.isnan(got).any(), f"{r.id}: NaN left in the destination at {worst}"
        assert e.max() <= max(4 * e_ref, floor), \
            f"{r.id} {acts}/{pact}: e = {e.max() / U:.2f} u at {worst} (torch fp32 {e_ref / U:.2f} u, floor {floor / U:.2f} u)"
        assert e.max() <= bound, f"{r.id} {acts}/{pact}: e = {e.max() / U:.2f} u at {worst} beyond the bound {bound / U:.0f} u"


@pytest.mark.gpu
def test_refused_descriptors_write_nothing(gpu):
    """MSEG_EINVAL means nothing was launched: the destination (NaN body and sentinels) is bit-unchanged, for the query and
    the call alike.  Parity order with an odd output height; two sources whose channels do not add up to Cin; a weight
    gradient whose Nch is no multiple of 4 (the only way to wgrad_reduce_kernel<16> with an aligned workspace)."""
    lib = gpu
    by = {r.id: r for r in ROWS}
    # parity order needs even Ho and Wo
    r = by["gen_dgrad_s2_linear_odd"]._replace(dest="plain")
    d = make_data(r, "exact", *exact_acts(r), 1)
    keep = []
    p, dsts = build_igemm(r, d, keep)
    p.morder = 1
    assert _name(lib, lib.mseg_igemm_query, p)[0] == EINVAL
    assert lib.mseg_igemm(C.byref(p), _stream()) == EINVAL
    assert all(b.untouched() for b in dsts)
    p.morder = 0                                            # the same descriptor in linear order is accepted
    assert lib.mseg_igemm(C.byref(p), _stream()) == 0
    assert not dsts[0].untouched()
    # two sources, Cin off by 4
    r = by["halo_two_sources"]
    d = make_data(r, "exact", *exact_acts(r), 2)
    keep = []
    p, dsts = build_igemm(r, d, keep)
    p.Cin += 4
    assert _name(lib, lib.mseg_igemm_query, p)[0] == EINVAL
    assert lib.mseg_igemm(C.byref(p), _stream()) == EINVAL
    assert all(b.untouched() for b in dsts)
    # weight gradient: Nch % 4 != 0 (also with many splits requested)
    r = by["wred_many_splits_store5"]
    d = make_data(r, "exact", *exact_acts(r), 3)
    keep = []
    p, dst = build_wgrad(r, d, keep)
    p.Q[0].C, p.Nch = 6, 6
    assert _name(lib, lib.mseg_wgrad_query, p)[0] == EINVAL
    assert lib.mseg_wgrad(C.byref(p), _stream()) == EINVAL
    assert dst.untouched()
