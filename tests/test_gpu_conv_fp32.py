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
import collections
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
import pointwise_ref as R

U = 2.0 ** -24
TINY = 2.0 ** -100
GUARD = 256
SENT = np.array([0xFFC12345], dtype=np.uint32).view(np.int32)[0]      # a NaN no kernel produces
NANBITS = np.array([0x7FC00000], dtype=np.uint32).view(np.int32)[0]
EINVAL = -1
GENERIC = ("leakyrelu", "elu", "mish")

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
def _b(v):
    return "true" if v else "false"


def HALO(bn, tr): return f"igemm_halo_kernel<{bn}, {tr}>"
def FAST(bn, tr, ps, sb): return f"igemm_fast_kernel<128, {bn}, {tr}, {_b(ps)}, {_b(sb)}>"
def GEN(bn, ps, ga): return f"igemm_kernel<128, {bn}, {_b(ps)}, {_b(ga)}>"
def WH(t, q): return f"wgrad_halo_kernel<{t}, {q}>"
def W9(t, q): return f"wgrad_halo9_kernel<{t}, {q}>"
def WG(kw, ga, ps): return f"wgrad_kernel<{kw}, {_b(ga)}, {_b(ps)}>"
def WF(kw, p, q): return f"wgrad_fast_kernel<{kw}, {p}, {q}>"


Row = collections.namedtuple("Row", "id op N cs Co H W stride acts tabs dest kernel xkernel opt")


def row(id, op, N, cs, Co, H, W, kernel, xkernel=None, stride=1, acts=None, tabs=None, dest="plain", **opt):
    """op: conv (3x3 forward), dgrad (its data gradient, TCONV), convT (ConvTranspose 2x2, scatter), convT_dgrad, wgrad3
    (3x3 weight gradient), wgrad2 (ConvTranspose weight gradient).  cs: channels of the GEMM's sources (for the weight
    gradients: of Q); Co: output channels (convT: Cq; weight gradients: channels of P).  H, W: size of the sources (weight
    gradients: of P).  acts / tabs: per source the activation and the table kind (None, "c" per channel, "s" per sample).
    dest: plain | ld (padded leading dimension, opt ldpad) | acc | split (opt split: first part accumulates, second does not).
    opt: pact / ptab (transform of P), out_hw / q_hw (size of the output / of Q where it is not the default), parity, splits,
    nch_store, bias, ws_off (bytes the weight-gradient workspace is moved off its 16-byte alignment)."""
    acts = list(acts) if acts else ["none"] * len(cs)
    tabs = list(tabs) if tabs else [None] * len(cs)
    assert len(acts) == len(cs) == len(tabs)
    return Row(id, op, N, list(cs), Co, H, W, stride, acts, tabs, dest, kernel, xkernel or kernel, opt)


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
# geometry of a row
# =================================================================================================================================
def is_wgrad(r):
    return r.op.startswith("wgrad")


def geom(r):
    g = {}
    if r.op == "conv":
        g.update(Hi=r.H, Wi=r.W, Ho=CR.out_size(r.H, r.stride), Wo=CR.out_size(r.W, r.stride), K=3, stride=r.stride, pad=1,
                 mode=0, Ngemm=r.Co, epi=0, Cq=0, T=9)
    elif r.op == "dgrad":
        Ho, Wo = r.opt.get("out_hw", (r.H, r.W) if r.stride == 1 else (2 * r.H, 2 * r.W))
        g.update(Hi=r.H, Wi=r.W, Ho=Ho, Wo=Wo, K=3, stride=r.stride, pad=1, mode=1, Ngemm=r.Co, epi=0, Cq=0, T=9)
    elif r.op == "convT":
        g.update(Hi=r.H, Wi=r.W, Ho=r.H, Wo=r.W, K=1, stride=1, pad=0, mode=0, Ngemm=4 * r.Co, epi=1, Cq=r.Co, T=1)
    elif r.op == "convT_dgrad":
        g.update(Hi=r.H, Wi=r.W, Ho=r.H // 2, Wo=r.W // 2, K=2, stride=2, pad=0, mode=0, Ngemm=r.Co, epi=0, Cq=0, T=4)
    elif r.op == "wgrad3":
        Hq, Wq = r.opt.get("q_hw", (r.H, r.W) if r.stride == 1 else (2 * r.H, 2 * r.W))
        g.update(Hp=r.H, Wp=r.W, Hq=Hq, Wq=Wq, K=3, stride=r.stride, pad=1)
    elif r.op == "wgrad2":
        g.update(Hp=r.H, Wp=r.W, Hq=2 * r.H, Wq=2 * r.W, K=2, stride=2, pad=0)
    else:
        raise ValueError(r.op)
    if not is_wgrad(r):
        g["morder"] = 1 if (r.op == "dgrad" and r.opt.get("parity", r.stride == 2)) else 0
        g["Cin"] = sum(r.cs)
        g["Kpad"], g["Npad"] = -(-g["Cin"] // 32) * 32, -(-g["Ngemm"] // 128) * 128
        g["out_rows"] = r.N * g["Ho"] * g["Wo"] * (4 if r.op == "convT" else 1)
        g["out_cols"] = r.Co
        g["bias"] = r.opt.get("bias", r.op in ("conv", "convT"))
        n = g["Ngemm"]
        if r.dest == "split":
            c0 = r.opt["split"]
            g["dsts"] = [(c0, c0, 1), (n - c0, n - c0, 0)]           # (columns, leading dimension, accumulate)
        elif r.dest == "ld":
            g["dsts"] = [(r.Co, r.Co + r.opt["ldpad"], 0)]
        else:
            g["dsts"] = [(r.Co, r.Co, 1 if r.dest == "acc" else 0)]
        g["dot"] = g["T"] * g["Cin"]
    else:
        g["Nch"] = sum(r.cs)
        g["Nst"] = r.opt.get("nch_store", g["Nch"])
        g["dot"] = r.N * g["Hp"] * g["Wp"]
    return g


def epilogue_row_mode(r):
    """which addressing mode of igemm_epilogue a row's launch uses: 0 affine, 1 halo tiles narrower than 32, 2 scatter over
    rows that are no multiple of 32, 3 parity order inside a class, 4 a 32-row tile straddling two parity classes.
    The library does not report the mode: this RESTATES the selection in microbeseg_amd/csrc/igemm_common.h, igemm_epilogue,
    the block `if (tw_log2 >= 0) ... else if (e_epi == MSEG_EPI_SCATTER2X2) ... else if (e_morder == MSEG_MORDER_PARITY)`
    that sets `mode` (lines 136-167 when this was written), and the tile width of halo_geometry() in igemm.hip (largest
    power of two <= 64 dividing W).  It will not notice a change there: keep the two in step."""
    g = geom(r)
    if r.kernel.startswith("igemm_halo_kernel"):
        tw = 64
        while r.W % tw:
            tw //= 2
        return 0 if tw >= 32 else 1
    if g["epi"] == 1:
        return 0 if g["Wo"] % 32 == 0 else 2
    if g["morder"] == 1:
        if (g["Wo"] // 2) % 32 == 0:
            return 0
        per = r.N * g["Ho"] * g["Wo"] // 4
        return 3 if per % 32 == 0 else 4
    return 0


def float_variants(r):
    """(acts, pact) combinations of the float mode: every activation the row's kernel takes"""
    pact, ptab = r.opt.get("pact", "none"), r.opt.get("ptab")
    allacts = r.acts + [pact]
    if any(a in GENERIC for a in allacts):
        out = []
        for gact in GENERIC:
            v = [gact if a in GENERIC else a for a in allacts]
            out.append((v[:-1], v[-1]))
        return out
    swap = {"none": "relu", "relu": "none"}
    v = [swap[a] if t else a for a, t in zip(allacts, r.tabs + [ptab])]     # a table keeps the transform alive
    out = [(r.acts, pact)]
    if v != allacts:
        out.append((v[:-1], v[-1]))
    return out


def exact_acts(r):
    fix = lambda a: "relu" if a in GENERIC else a
    return [fix(a) for a in r.acts], fix(r.opt.get("pact", "none"))


# =================================================================================================================================
# descriptors
# =================================================================================================================================
def _eng():
    from microbeseg_amd import engine, _lib
    return engine, _lib, _lib.load()


def _src(ptr, Cc, act, tab, scale_ptr=256, shift_ptr=256):
    from microbeseg_amd._lib import MsegSrc, ACT
    s = MsegSrc()
    s.ptr, s.C, s.act, s.dtype = ptr, Cc, ACT[act], 0
    if tab:
        s.scale, s.shift, s.ss = scale_ptr, shift_ptr, (Cc if tab == "s" else 0)
    return s


def engine_query(r, acts, pact):
    """engine.igemm_query / engine.wgrad_query for the row (placeholder pointers: needs the library, no device)"""
    engine, _, _ = _eng()
    g = geom(r)
    srcs = [_src(256, c, a, t) for c, a, t in zip(r.cs, acts, r.tabs)]
    if is_wgrad(r):
        P = _src(256, r.Co, pact, r.opt.get("ptab"))
        return engine.wgrad_query(P, srcs, r.N, g["Hp"], g["Wp"], g["Hq"], g["Wq"], g["K"], g["K"], g["stride"], g["pad"],
                                  nch_store=g["Nst"], precision="f32")
    d = g["dsts"]
    return engine.igemm_query(srcs, g["Kpad"], g["Npad"], r.N, g["Hi"], g["Wi"], g["Ho"], g["Wo"], g["K"], g["K"], g["stride"],
                              g["pad"], g["mode"], g["Ngemm"], d[0][1], acc0=d[0][2], ld1=d[1][1] if len(d) > 1 else 0,
                              acc1=0, split=d[0][0] if len(d) > 1 else None, epi=g["epi"], Cq=g["Cq"], morder=g["morder"],
                              precision="f32", bias=g["bias"])


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
# data and references
# =================================================================================================================================
def _tables(rng, mode, tab, N, Cc):
    if not tab:
        return None, None
    shape = (N, Cc) if tab == "s" else (Cc,)
    if mode == "exact":
        sc = rng.choice([-2, -1, 1, 2, 3], size=shape)
        sh = rng.choice([-2, -1, 1, 2], size=shape)             # never 0: a transformed padding pixel is not 0
    else:
        sc, sh = 1.0 + 0.3 * rng.normal(size=shape), 0.5 * rng.normal(size=shape)
    return sc.astype(np.float32), sh.astype(np.float32)


def _draw(rng, mode, shape, sigma=1.0):
    if mode == "exact":
        return rng.integers(-3, 4, size=shape).astype(np.float32)
    return (sigma * rng.normal(size=shape)).astype(np.float32)


def make_data(r, mode, acts, pact, seed):
    """host arrays of one launch (fp32 values, what the device gets) and the reference of conv_ref: fp64, or int64 in the
    exact mode -> dict"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = geom(r)
    d = {"acts": acts, "pact": pact, "mode": mode}
    sizes = [(g["Hq"], g["Wq"])] * len(r.cs) if is_wgrad(r) else [(g["Hi"], g["Wi"])] * len(r.cs)
    d["z"], d["sc"], d["sh"] = [], [], []
    for i, (c, t, hw) in enumerate(zip(r.cs, r.tabs, sizes)):
        z = _draw(rng, mode, (r.N, hw[0], hw[1], c))
        if mode == "float" and i == 0:
            z[..., 0] += np.float32(1.5)
        sc, sh = _tables(rng, mode, t, r.N, c)
        d["z"].append(z), d["sc"].append(sc), d["sh"].append(sh)
    cast = CR.as_exact if mode == "exact" else (lambda v: v)
    ops = [cast(CR.operand(z, a, sc, sh)) for z, a, sc, sh in zip(d["z"], acts, d["sc"], d["sh"])]
    if is_wgrad(r):
        d["pz"] = _draw(rng, mode, (r.N, g["Hp"], g["Wp"], r.Co))
        d["psc"], d["psh"] = _tables(rng, mode, r.opt.get("ptab"), r.N, r.Co)
        P = cast(CR.operand(d["pz"], pact, d["psc"], d["psh"]))
        d["ref"], d["S"] = CR.wgrad(P, ops, g["K"], g["stride"], g["Nst"])
    else:
        Cin, n = g["Cin"], g["Ngemm"]
        sig = 1.0 if mode == "exact" else 1.0 / np.sqrt(g["T"] * Cin)
        wshape = {"conv": (r.Co, Cin, 3, 3), "dgrad": (Cin, r.Co, 3, 3), "convT": (Cin, r.Co, 2, 2),
                  "convT_dgrad": (r.Co, Cin, 2, 2)}[r.op]
        d["w"] = w = _draw(rng, mode, wshape, sig)
        d["bias"] = bias = _draw(rng, mode, (r.Co,)) if g["bias"] else None
        rows, cols = g["out_rows"], g["out_cols"]
        base = np.zeros((rows, cols), dtype=np.float32)
        c = 0
        for (k, _, acc) in g["dsts"]:
            if acc:
                base[:, c:c + k] = _draw(rng, mode, (rows, k))
            c += k
        d["base"] = base
        oshape = (r.N, g["Ho"] * (2 if r.op == "convT" else 1), g["Wo"] * (2 if r.op == "convT" else 1), r.Co)
        wc, bc, basec = cast(w), (None if bias is None else cast(bias)), cast(base).reshape(oshape)
        if r.op == "conv":
            ref = CR.conv_fwd(ops, wc, bc, r.stride, basec)
        elif r.op == "dgrad":
            ref = CR.conv_dgrad(np.concatenate(ops, 3), wc, r.stride, g["Ho"], g["Wo"], basec)
        elif r.op == "convT":
            ref = CR.convT_fwd(np.concatenate(ops, 3), wc, bc, basec)
        else:
            ref = CR.convT_dgrad(np.concatenate(ops, 3), wc, basec)
        d["ref"], d["S"] = ref[0].reshape(rows, cols), ref[1].reshape(rows, cols)
    if mode == "exact":
        CR.assert_exact(d["S"])
    return d


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _op32(z, act, sc, sh):
    """the operand as fp32 arithmetic computes it, NCHW"""
    a = R.activation(_t32(z), act, dtype=torch.float32)
    if sc is not None:
        s, h = _t32(sc), _t32(sh)
        if s.dim() == 1:
            s, h = s[None], h[None]
        a = a * s[:, None, None, :] + h[:, None, None, :]
    return a.permute(0, 3, 1, 2).contiguous()


def torch_fp32(r, d):
    """torch's CPU fp32 result of the same operation on the same inputs, shaped like d['ref']"""
    g = geom(r)
    x = torch.cat([_op32(z, a, sc, sh) for z, a, sc, sh in zip(d["z"], d["acts"], d["sc"], d["sh"])], 1)
    if is_wgrad(r):
        P = _op32(d["pz"], d["pact"], d["psc"], d["psh"])
        if r.op == "wgrad3":
            w = torch.zeros(r.Co, g["Nch"], 3, 3, requires_grad=True)
            F.conv2d(x, w, None, stride=r.stride, padding=1).backward(P)
        else:
            w = torch.zeros(r.Co, g["Nch"], 2, 2, requires_grad=True)
            F.conv_transpose2d(P, w, None, stride=2).backward(x)
        return w.grad[:, :g["Nst"]].numpy()
    w = _t32(d["w"])
    b = None if d["bias"] is None else _t32(d["bias"])
    if r.op == "conv":
        y = F.conv2d(x, w, b, stride=r.stride, padding=1)
    elif r.op == "dgrad":
        xin = torch.zeros(r.N, r.Co, g["Ho"], g["Wo"], requires_grad=True)
        F.conv2d(xin, w, None, stride=r.stride, padding=1).backward(x)
        y = xin.grad
    elif r.op == "convT":
        y = F.conv_transpose2d(x, w, b, stride=2)
    else:
        xin = torch.zeros(r.N, r.Co, g["Ho"], g["Wo"], requires_grad=True)
        F.conv_transpose2d(xin, w, None, stride=2).backward(x)
        y = xin.grad
    y = y.detach().permute(0, 2, 3, 1).reshape(g["out_rows"], g["out_cols"])
    return (y + _t32(d["base"])).numpy()


def pack_weight(r, w):
    """[T][Npad][Kpad] GEMM operand of include/mseg_hip.h, zero filled, from the torch-layout weight"""
    g = geom(r)
    perm = {"conv": (2, 3, 0, 1), "dgrad": (2, 3, 1, 0), "convT": (2, 3, 1, 0), "convT_dgrad": (2, 3, 0, 1)}[r.op]
    T = 1 if r.op == "convT" else g["K"] * g["K"]
    core = np.transpose(w, perm).reshape(T, g["Ngemm"], g["Cin"])
    wp = np.zeros((T, g["Npad"], g["Kpad"]), dtype=np.float32)
    wp[:, :g["Ngemm"], :g["Cin"]] = core
    return wp


# =================================================================================================================================
# guarded buffers and launches
# =================================================================================================================================
def _sync():
    """wait for the device; a HIP error here (a faulted kernel) ends the whole session: nothing more is started on that device"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error after a launch, stopping: {e}", returncode=3)


class Guarded:
    """rows x cols values at leading dimension ld inside sentinels: GUARD words before and after, and the columns cols .. ld"""

    def __init__(self, rows, cols, ld, init=None):
        self.rows, self.cols, self.ld = rows, cols, ld
        host = np.full(GUARD + rows * ld + GUARD, SENT, dtype=np.int32)
        body = host[GUARD:GUARD + rows * ld].reshape(rows, ld)
        body[:, :cols] = NANBITS if init is None else np.ascontiguousarray(init, dtype=np.float32).view(np.int32)
        self.before = host.copy()
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + 4 * GUARD

    def take(self):
        """-> the values (fp32, host) after checking every sentinel bit for bit"""
        _sync()
        after = self.dev.cpu().numpy()
        mask = np.ones(after.shape, dtype=bool)
        mask[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols] = False
        bad = np.nonzero(mask & (after != self.before))[0]
        assert bad.size == 0, f"{bad.size} sentinel words overwritten, first at word {int(bad[0]) - GUARD} of the destination"
        return after[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols].copy().view(np.float32)

    def untouched(self):
        _sync()
        return np.array_equal(self.dev.cpu().numpy(), self.before)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _name(lib, fn, p):
    from microbeseg_amd._lib import MsegKernelInfo
    info = MsegKernelInfo()
    rc = fn(C.byref(p), C.byref(info))
    return rc, info


def _dev_srcs(r, d, keep):
    out = []
    for c, z, a, t, sc, sh in zip(r.cs, d["z"], d["acts"], r.tabs, d["sc"], d["sh"]):
        zt = _t32(z).cuda()
        keep.append(zt)
        if t:
            st, ht = _t32(sc).cuda(), _t32(sh).cuda()
            keep += [st, ht]
            out.append(_src(zt.data_ptr(), c, a, t, st.data_ptr(), ht.data_ptr()))
        else:
            out.append(_src(zt.data_ptr(), c, a, None))
    return out


def build_igemm(r, d, keep):
    """the descriptor the way engine.igemm builds it (split-K scratch from mseg_igemm_workspace_bytes included) -> (p, dsts)"""
    _, L, lib = _eng()
    g = geom(r)
    p = L.MsegIgemm()
    for i, s in enumerate(_dev_srcs(r, d, keep)):
        p.src[i] = s
    p.nsrc, p.Cin, p.Kpad, p.Npad = len(r.cs), g["Cin"], g["Kpad"], g["Npad"]
    p.NB, p.Hi, p.Wi, p.Ho, p.Wo = r.N, g["Hi"], g["Wi"], g["Ho"], g["Wo"]
    p.KH = p.KW = g["K"]
    p.stride, p.pad, p.mode, p.morder = g["stride"], g["pad"], g["mode"], g["morder"]
    p.Ngemm, p.epi, p.Cq = g["Ngemm"], g["epi"], g["Cq"]
    wt = _t32(pack_weight(r, d["w"])).cuda()
    keep.append(wt)
    p.w = wt.data_ptr()
    if d["bias"] is not None:
        bt = _t32(d["bias"]).cuda()
        keep.append(bt)
        p.bias = bt.data_ptr()
    dsts, c = [], 0
    for (k, ld, acc) in g["dsts"]:
        dsts.append(Guarded(g["out_rows"], k, ld, d["base"][:, c:c + k] if acc else None))
        c += k
    p.dst0, p.ld0, p.acc0 = dsts[0].ptr, g["dsts"][0][1], g["dsts"][0][2]
    p.split = g["Ngemm"]
    if len(dsts) > 1:
        p.dst1, p.ld1, p.acc1, p.split = dsts[1].ptr, g["dsts"][1][1], g["dsts"][1][2], g["dsts"][0][0]
    need = lib.mseg_igemm_workspace_bytes(C.byref(p))
    assert (need > 0) == ("splitk" in r.opt), f"split-K scratch {need} bytes"
    if need:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        keep.append(ws)
        p.ws, p.ws_bytes = ws.data_ptr(), need
    return p, dsts


def run_igemm(r, d, want):
    _, L, lib = _eng()
    keep = []
    p, dsts = build_igemm(r, d, keep)
    rc, info = _name(lib, lib.mseg_igemm_query, p)
    assert rc == 0 and info.name.decode() == want, (rc, info.name)
    if "splitk" in r.opt:
        want_ws = r.opt["splitk"] * geom(r)["out_rows"] * geom(r)["Ngemm"] * 4        # one fp32 partial result per split
        assert info.launches >= 2 and info.workspace == want_ws == p.ws_bytes, (info.launches, info.workspace, p.ws_bytes)
    rc = lib.mseg_igemm(C.byref(p), _stream())
    assert rc == 0, f"mseg_igemm returned {rc} (hipError {lib.mseg_last_hip_error()})"
    assert lib.mseg_last_kernel().decode() == want
    return np.concatenate([b.take() for b in dsts], axis=1)


def build_wgrad(r, d, keep):
    _, L, lib = _eng()
    g = geom(r)
    p = L.MsegWgrad()
    pz = _t32(d["pz"]).cuda()
    keep.append(pz)
    ptab = r.opt.get("ptab")
    if ptab:
        st, ht = _t32(d["psc"]).cuda(), _t32(d["psh"]).cuda()
        keep += [st, ht]
        p.P = _src(pz.data_ptr(), r.Co, d["pact"], ptab, st.data_ptr(), ht.data_ptr())
    else:
        p.P = _src(pz.data_ptr(), r.Co, d["pact"], None)
    for i, s in enumerate(_dev_srcs(r, d, keep)):
        p.Q[i] = s
    p.nq, p.Nch, p.Nch_store = len(r.cs), g["Nch"], g["Nst"]
    p.NB, p.Hp, p.Wp, p.Hq, p.Wq = r.N, g["Hp"], g["Wp"], g["Hq"], g["Wq"]
    p.KH = p.KW = g["K"]
    p.stride, p.pad = g["stride"], g["pad"]
    p.splits = r.opt.get("splits", 0)
    need = lib.mseg_wgrad_workspace_bytes(C.byref(p))
    assert need > 0
    off = r.opt.get("ws_off", 0)
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    keep.append(ws)
    assert ws.data_ptr() % 16 == 0 and off % 4 == 0
    p.ws = ws.data_ptr() + off
    dst = Guarded(r.Co, g["Nst"] * g["K"] * g["K"], g["Nst"] * g["K"] * g["K"])
    p.dst = dst.ptr
    if "splits" in r.opt:       # the reduction is chosen by the number of splits the plan ends up with
        per = g["K"] * g["K"] * r.Co * g["Nch"] * 4
        assert need % per == 0 and (need // per >= 32) == (r.opt["splits"] >= 32), need // per
    return p, dst


def run_wgrad(r, d, want):
    _, L, lib = _eng()
    keep = []
    p, dst = build_wgrad(r, d, keep)
    g = geom(r)
    rc, info = _name(lib, lib.mseg_wgrad_query, p)
    assert rc == 0 and info.name.decode() == want, (rc, info.name)
    rc = lib.mseg_wgrad(C.byref(p), _stream())
    assert rc == 0, f"mseg_wgrad returned {rc} (hipError {lib.mseg_last_hip_error()})"
    assert lib.mseg_last_kernel().decode() == want
    return dst.take().reshape(r.Co, g["Nst"], g["K"], g["K"])


def launch(r, d, want):
    return run_wgrad(r, d, want) if is_wgrad(r) else run_igemm(r, d, want)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _eng()[2]


def _seed(r, extra=0):
    return 1000 * ROW_IDS.index(r.id) + extra if r.id in ROW_IDS else extra


# =================================================================================================================================
# the tests
# =================================================================================================================================
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


def family(kernel):
    return kernel.split("<")[0]


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
