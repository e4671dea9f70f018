"""GPU (MI355X): every bf16 instantiation of the convolution family (microbeseg_amd/csrc/igemm.hip, igemm_p8.hip, wgrad.hip)
through the C ABI, pinned to its kernel and compared element by element with the plain references of tests/conv_ref.py.
The method is that of tests/test_gpu_conv_fp32.py, row for row (shared machinery: tests/conv_table.py).

ONE table (ROWS).  A row names the operation, the shapes, the storage of the sources and of the destinations (fp32 or
bf16), how each source is transformed on load, the destination form and the kernel instantiation the dispatch must take.
Before a launch engine.igemm_query / engine.wgrad_query and mseg_*_query on the very descriptor must name exactly that
kernel, after it mseg_last_kernel() must too.  Rows select kernels through shapes only: a module fixture sets the three
process-wide switches to their defaults (persistent 1, wide tiles 1, p8 1) and MSEG_P8 must not be in the environment.
The persistent kernels are gated on tile counts against the 256 compute units (which the query assumes without a device
too), so their rows have the size of the gate: c64p >= 1024 tiles of 128 pixels, m512 >= 512 tiles of 512 pixels, w4m >=
512 tiles of 256 pixels, p8 >= 256 tiles of 256 / 512 pixels, ctp M / 128 >= 1024, ctp2 M / 64 >= 256, ctd M / 64 >= 1024;
where the gate allows it a few tiles more, so that the last round of the persistent workgroups is ragged.

Two modes per row, no element exempt:

  exact   integer operands |v| <= 3 with every third zero a -0.0, integer scales (negative ones too) and nonzero integer
          shifts, activations none / relu (an any-activation row runs its relu sibling, column `xkernel`): every transformed
          operand is an integer of magnitude <= 11, which bf16 holds exactly, and conv_ref.assert_exact keeps the sum of
          magnitudes below 2^24, so the fp32 accumulators are exact.  An fp32 destination must equal the int64 reference
          bit for bit, a bf16 destination round_bf16 of it bit for bit.  For a bf16 destination the bias (257 .. 319 in
          magnitude) and the old content of an accumulating destination (258 .. 318, even) lift the sums beyond 256, where
          odd sums are rounding ties: a store that truncates or rounds half up gives other bits on hundreds of elements
          of every such row.
  float   N(0, 1) operands (+1.5 on channel 0 of the first source; bf16 tensors hold their bf16 rounding), scale ~ 1, random
          shift, every activation the row's kernel takes.  The reference is fp64 on the operands rounded the way the kernels
          round them (conv_ref.operand_bf16): weights and plain sources directly, a transformed source as
          bf16(fma(act(x), scale, shift)) with the fma in fp32.  Where such a value lies so near a bf16 tie that a correct
          kernel may round either way the operand is AMBIGUOUS; the field A (one bf16 ulp there, 0 elsewhere) convolved with
          |w| is the WIDENING of an output element.  tests/test_conv_ref_host.py asserts for every row and seed used here
          that the widening stays within a quarter of the element's mean term (S / 4K): a condition, not a measurement.
          Per element, e = |got - ref64| / max(S, 2^-100):
              e <= max(4 e_ref, FLOOR[family]) + widening / S   and   e <= (K + 32) 2^-24 + widening / S
          e_ref = torch's CPU fp32 result on the same rounded operands, K as in the fp32 table (T * Cin; pixels summed over
          for the weight gradients).  A bf16 destination adds half a bf16 ulp of the stored value, bf16_ulp(got) / 2S: between
          2^-9 |got| / S (just below a power of two) and 2^-8 |got| / S (at one).  The flat 2^-9 |ref| / S is that lower end: a
          correctly rounded store exceeds it for every value in the lower half of a binade (measured here: by up to 2e4 u
          in each of the 37 float runs with a bf16 destination, while the exact mode finds every stored bit right).

Buffers: conv_table.Guarded — 256 sentinel words before and after every destination and sentinel columns where ld exceeds
the channels; for bf16 destinations 16-bit sentinels checked per 2-byte word (the channel-pair stores must not touch the
neighbouring half word).  Destinations that are not accumulated into start as NaN.  Rows whose query reports stats_rows > 0
get a sentinel-filled statistics buffer of exactly that many rows: every word of it must be written, the guards not, and
the reduced sums must match the fp64 sums of act(z) and act(z)^2 over the output the kernel itself stored — which the same
test has just verified element by element — within (count + 32) 2^-24 sum |term|.  A row with `stats` whose kernel takes
none must leave the buffer untouched.

Dead instantiations: igemm_halo_bf16_kernel<128, *, *> is compiled (MSEG_HALO16 takes BN as a parameter) but every wide
launch of the halo shape goes to igemm_halo_bf16w4_kernel or one of the persistent kernels
(test_dead_bf16_halo_instantiations asks the dispatch for every small wide shape).  They are listed here, not removed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import conv_ref as CR
import pointwise_ref as R
from conv_table import (EINVAL, U, TINY, _b, row, is_wgrad, geom, float_variants, exact_acts, engine_query, make_data,
                        torch_fp32, build_igemm, build_wgrad, launch, family, _eng, _name, _stream)

# float mode: FLOOR[family] in units of 2^-24, about twice the largest e net of its allowances (widening / S and, for a bf16
# destination, half a bf16 ulp of the stored value) the kernels of the family showed on the MI355X over all float runs of
# this table (229 launches); beside it what torch's CPU fp32 showed on the same rounded operands and the largest share of
# the worst-case bound (K + 32) 2^-24 any element used.  All relative to S:
#   family                        runs   e_hip    e_ref    e_hip / bound
#   igemm_halo_bf16_kernel         18    1.80     1.79     0.007
#   igemm_halo_bf16w4_kernel       13    1.67     2.46     0.016
#   igemm_halo_bf16w4m_kernel       6    2.29     2.84     0.008
#   igemm_halo_bf16m512_kernel     12    2.41     1.14     0.002
#   igemm_c64p_bf16_kernel         12    2.12     1.41     0.003
#   igemm_p8_kernel                27    2.37     2.69     0.007
#   igemm_ctp_bf16_kernel          12    2.59     4.47     0.016
#   igemm_ctp2_bf16_kernel         12    2.30     4.40     0.008
#   igemm_ctd_bf16_kernel           2    2.27     1.23     0.008
#   igemm_fast_bf16_kernel         43    1.46     3.05     0.029
#   wgrad_halo_bf16_kernel         72    2.00     6.20     0.025
# (the products of bf16 operands are exact in fp32, so only the accumulation rounds: the kernels stay below torch's fp32
# on most families).  No kernel needed more than 3 % of the hard bound.
FLOOR = {"igemm_halo_bf16_kernel": 3.6, "igemm_halo_bf16w4_kernel": 3.4, "igemm_halo_bf16w4m_kernel": 4.6,
         "igemm_halo_bf16m512_kernel": 4.8, "igemm_c64p_bf16_kernel": 4.3, "igemm_p8_kernel": 4.8,
         "igemm_ctp_bf16_kernel": 5.2, "igemm_ctp2_bf16_kernel": 4.6, "igemm_ctd_bf16_kernel": 4.6,
         "igemm_fast_bf16_kernel": 3.0, "wgrad_halo_bf16_kernel": 4.0}


# =================================================================================================================================
# the table
# =================================================================================================================================
def HB(tr, s16): return f"igemm_halo_bf16_kernel<64, {tr}, {_b(s16)}>"
def W4(tr, s16): return f"igemm_halo_bf16w4_kernel<{tr}, {_b(s16)}>"
def W4M(tr): return f"igemm_halo_bf16w4m_kernel<{tr}, true>"
def M512(tr, s16): return f"igemm_halo_bf16m512_kernel<{tr}, {_b(s16)}>"
def C64P(tr, d16): return f"igemm_c64p_bf16_kernel<{tr}, {_b(d16)}>"
def P8(bm, bn, tr, st): return f"igemm_p8_kernel<{bm}, {bn}, {tr}, {_b(st)}>"
def CTP(tr, d16): return f"igemm_ctp_bf16_kernel<{tr}, {_b(d16)}>"
def CTP2(tr, d16): return f"igemm_ctp2_bf16_kernel<{tr}, {_b(d16)}>"
def CTD(d16): return f"igemm_ctd_bf16_kernel<{_b(d16)}>"
def FB(bn, tr, ps, s16): return f"igemm_fast_bf16_kernel<128, {bn}, {tr}, {_b(ps)}, {_b(s16)}>"
def WB(t, q, stride, kw, p, s16): return f"wgrad_halo_bf16_kernel<{t}, {q}, {stride}, {kw}, {p}, {_b(s16)}>"


def brow(id, op, N, cs, Co, H, W, kernel, xkernel=None, s=0, d=0, **kw):
    """a row of the bf16 table: s / d = 1 for bf16 storage of the sources / of the destinations"""
    return row(id, op, N, cs, Co, H, W, kernel, xkernel, prec="bf16", sdt="bf16" if s else "f32", ddt="bf16" if d else "f32", **kw)


ROWS = [
    # ---- igemm_halo_bf16_kernel<64, TR, S16>: 3x3 stride 1, <= 64 output channels, 128-pixel tiles of width 32 .. 4 ---------------
    brow("hb_w32_plain", "conv", 1, [40], 24, 8, 32, HB(0, 0)),
    brow("hb_w16_overhang_affine_acc16", "conv", 1, [72], 40, 12, 16, HB(1, 0), acts=["relu"], tabs=["c"], dest="acc", d=1),
    brow("hb_w8_mish_persample", "conv", 2, [16], 16, 16, 8, HB(2, 0), HB(1, 0), acts=["mish"], tabs=["s"]),
    brow("hb_w4_overhang_ld16", "conv", 1, [8], 6, 28, 12, HB(0, 1), s=1, d=1, dest="ld", ldpad=2),
    brow("hb_two_sources_split16", "conv", 2, [32, 8], 16, 8, 16, HB(1, 1), s=1, d=1, acts=["relu", "none"], tabs=["c", "s"],
         dest="split", split=8),
    brow("hb_dgrad_elu", "dgrad", 1, [96], 24, 8, 16, HB(2, 1), HB(1, 1), s=1, acts=["elu"], tabs=["c"]),
    brow("hb_concat64_half_rows", "conv", 1, [64, 8], 40, 4, 32 // 2, HB(1, 0), acts=["none", "relu"], tabs=["c", None]),   # 50 %
    brow("hb_splitk", "conv", 1, [128], 8, 8, 16, HB(0, 1), s=1, dest="split", split=4, splitk=2),
    brow("hb_splitk_ld16", "dgrad", 1, [128], 12, 8, 16, HB(1, 0), d=1, acts=["relu"], tabs=["c"], dest="ld", ldpad=4, splitk=2),
    brow("hb_stats_not_taken", "conv", 1, [8], 8, 8, 16, HB(0, 1), s=1, d=1, stats="relu"),
    # ---- igemm_halo_bf16w4_kernel<TR, S16>: > 64 output channels, too few tiles for the persistent kernels -----------------------
    brow("w4_w32_plain", "conv", 1, [8], 72, 8, 32, W4(0, 0)),
    brow("w4_dgrad_persample_split", "dgrad", 2, [40], 136, 8, 16, W4(1, 0), acts=["relu"], tabs=["s"], dest="split", split=72),
    brow("w4_w8_mish", "conv", 1, [8], 160, 16, 8, W4(2, 0), W4(1, 0), acts=["mish"], tabs=["c"]),
    brow("w4_half_rows_16", "conv", 1, [8], 72, 4, 16, W4(0, 1), s=1, d=1),
    brow("w4_two_sources_acc16", "conv", 2, [32, 8], 136, 16, 8, W4(1, 1), s=1, d=1, acts=["relu", "none"], tabs=["c", "s"],
         dest="acc"),
    brow("w4_w4_dgrad_leaky", "dgrad", 1, [72], 160, 16, 12, W4(2, 1), W4(1, 1), s=1, acts=["leakyrelu"], tabs=["c"]),
    brow("w4_m_fastest_splitk", "conv", 1, [512], 256, 8, 16, W4(0, 0), splitk=8),     # weights > 2 MB, two N tiles
    # ---- igemm_halo_bf16w4m_kernel<TR, true>: >= 512 tiles of 256 pixels, Cin or Ngemm off the p8 kernel's multiples -------------
    brow("w4m_plain", "conv", 1, [8], 136, 252, 256, W4M(0), s=1, d=1),
    brow("w4m_dgrad_persample_split", "dgrad", 4, [40], 160, 128, 128, W4M(1), s=1, d=1, acts=["relu"], tabs=["s"],
         dest="split", split=96),
    brow("w4m_w8_elu", "conv", 8, [72], 136, 352, 24, W4M(2), W4M(1), s=1, acts=["elu"], tabs=["c"], reseed=(1, 1, 2)),
    # ---- igemm_halo_bf16m512_kernel<TR, S16>: <= 64 output channels, >= 128 input channels, >= 512 tiles of 512 pixels -----------
    brow("m512_plain", "conv", 4, [128], 8, 250, 256, M512(0, 0)),
    brow("m512_concat64_16", "conv", 4, [64, 64], 40, 256, 256, M512(1, 0), d=1, acts=["relu", "none"], tabs=["c", "c"]),
    brow("m512_mish_persample", "conv", 4, [128], 8, 256, 256, M512(2, 0), M512(1, 0), acts=["mish"], tabs=["s"],
         reseed=(1, 1, 1)),
    brow("m512_w16_dgrad_acc16", "dgrad", 2, [128], 64, 500, 272, M512(0, 1), s=1, d=1, dest="acc"),
    brow("m512_concat96_persample", "conv", 4, [96, 32], 16, 256, 256, M512(1, 1), s=1, acts=["relu", "none"], tabs=["s", "c"]),
    brow("m512_leaky", "conv", 4, [128], 8, 256, 256, M512(2, 1), M512(1, 1), s=1, acts=["leakyrelu"], tabs=["c"], reseed=(0, 0, 5)),
    # ---- igemm_c64p_bf16_kernel<TR, D16>: 64 input channels on bf16 tensors, >= 1024 tiles of 128 pixels -------------------------
    brow("c64p_plain", "conv", 8, [64], 64, 128, 128, C64P(0, 0), s=1),
    brow("c64p_dgrad_ld16", "dgrad", 2, [64], 40, 250, 288, C64P(0, 1), s=1, d=1, dest="ld", ldpad=8),
    brow("c64p_persample_acc", "conv", 8, [64], 24, 128, 128, C64P(1, 0), s=1, acts=["relu"], tabs=["s"], dest="acc"),
    brow("c64p_w16_affine16", "conv", 1, [64], 64, 908, 144, C64P(1, 1), s=1, d=1, tabs=["c"]),
    brow("c64p_elu", "conv", 8, [64], 16, 128, 128, C64P(2, 0), C64P(1, 0), s=1, acts=["elu"], tabs=["c"], reseed=(1, 0, 1)),
    brow("c64p_w8_mish_acc16", "conv", 8, [64], 8, 128, 136, C64P(2, 1), C64P(1, 1), s=1, d=1, acts=["mish"], tabs=["s"],
         dest="acc"),
    # ---- igemm_p8_kernel<BM, BN, TR, STATS>: >= 128 output channels on bf16 tensors, >= 256 tiles --------------------------------
    brow("p8_256x256_plain", "conv", 1, [32], 256, 264, 256, P8(256, 256, 0, 0), s=1),
    brow("p8_256x256_concat_split16", "dgrad", 4, [32, 32], 256, 128, 128, P8(256, 256, 1, 0), s=1, d=1,
         acts=["relu", "none"], tabs=["c", "s"], dest="split", split=128),
    brow("p8_256x256_w16_mish", "conv", 1, [32], 256, 1376, 48, P8(256, 256, 2, 0), P8(256, 256, 1, 0), s=1, acts=["mish"],
         tabs=["c"], reseed=(1, 0, 0)),
    brow("p8_256x256_stats", "conv", 4, [32], 256, 128, 128, P8(256, 256, 0, 1), s=1, stats="none"),
    brow("p8_256x256_stats_relu16", "conv", 4, [32], 256, 130, 128, P8(256, 256, 1, 1), s=1, d=1, acts=["relu"], tabs=["c"],
         stats="relu"),
    brow("p8_512x128_plain", "conv", 1, [32], 192, 256, 256, P8(512, 128, 0, 0), s=1),
    brow("p8_512x128_persample_ld", "conv", 2, [32], 192, 128, 256, P8(512, 128, 1, 0), s=1, acts=["relu"], tabs=["s"],
         dest="ld", ldpad=8),
    brow("p8_512x128_dgrad_elu", "dgrad", 1, [32], 192, 264, 256, P8(512, 128, 2, 0), P8(512, 128, 1, 0), s=1, d=1,
         acts=["elu"], tabs=["c"], reseed=(0, 0, 1)),
    brow("p8_512x128_stats16", "conv", 1, [32], 128, 512, 256, P8(512, 128, 0, 1), s=1, d=1, stats="relu"),
    brow("p8_512x128_stats_affine", "conv", 1, [32], 192, 256, 256, P8(512, 128, 1, 1), s=1, tabs=["c"], stats="none"),
    brow("p8_256x128_w16_plain", "conv", 1, [32], 192, 688, 48, P8(256, 128, 0, 0), s=1),
    brow("p8_256x128_w20_dgrad_persample", "dgrad", 2, [32], 128, 1536, 20, P8(256, 128, 1, 0), s=1, d=1, acts=["relu"],
         tabs=["s"], dest="acc"),
    brow("p8_256x128_w16_mish", "conv", 1, [32], 192, 688, 48, P8(256, 128, 2, 0), P8(256, 128, 1, 0), s=1, acts=["mish"],
         tabs=["c"]),
    brow("p8_256x128_stats16", "conv", 1, [32], 192, 688, 48, P8(256, 128, 0, 1), s=1, d=1, stats="none"),
    brow("p8_256x128_stats_relu", "conv", 1, [32], 192, 690, 48, P8(256, 128, 1, 1), s=1, acts=["relu"], tabs=["c"],
         stats="relu"),
    # ---- igemm_ctp_bf16_kernel<TR, D16>: ConvTranspose 128 -> 64 on bf16 tensors, M / 128 >= 1024 --------------------------------
    brow("ctp_plain", "convT", 8, [128], 64, 128, 128, CTP(0, 0), s=1),
    brow("ctp_plain16", "convT", 1, [128], 64, 258, 512, CTP(0, 1), s=1, d=1),
    brow("ctp_persample", "convT", 8, [128], 64, 128, 128, CTP(1, 0), s=1, acts=["relu"], tabs=["s"]),
    brow("ctp_affine16", "convT", 2, [128], 64, 516, 128, CTP(1, 1), s=1, d=1, tabs=["c"]),
    brow("ctp_mish", "convT", 8, [128], 64, 128, 128, CTP(2, 0), CTP(1, 0), s=1, acts=["mish"], tabs=["c"]),
    brow("ctp_elu_persample16", "convT", 8, [128], 64, 128, 128, CTP(2, 1), CTP(1, 1), s=1, d=1, acts=["elu"], tabs=["s"]),
    # ---- igemm_ctp2_bf16_kernel<TR, D16>: ConvTranspose 256 -> 128 on bf16 tensors, M / 64 >= 256 --------------------------------
    brow("ctp2_plain", "convT", 1, [256], 128, 130, 128, CTP2(0, 0), s=1),
    brow("ctp2_w48_plain16", "convT", 1, [256], 128, 352, 48, CTP2(0, 1), s=1, d=1),              # scatter with Wo % 32 != 0
    brow("ctp2_persample", "convT", 4, [256], 128, 64, 64, CTP2(1, 0), s=1, acts=["relu"], tabs=["s"]),
    brow("ctp2_affine16", "convT", 1, [256], 128, 128, 128, CTP2(1, 1), s=1, d=1, tabs=["c"]),
    brow("ctp2_w48_leaky", "convT", 1, [256], 128, 352, 48, CTP2(2, 0), CTP2(1, 0), s=1, acts=["leakyrelu"], tabs=["c"], reseed=(2, 0, 1)),
    brow("ctp2_mish_persample16", "convT", 2, [256], 128, 132, 64, CTP2(2, 1), CTP2(1, 1), s=1, d=1, acts=["mish"],
         tabs=["s"]),
    # ---- igemm_ctd_bf16_kernel<D16>: data gradient of ConvTranspose 128 -> 64 on bf16 tensors, M / 64 >= 1024 --------------------
    brow("ctd_plain", "convT_dgrad", 4, [64], 128, 256, 256, CTD(0), s=1),
    brow("ctd_plain16", "convT_dgrad", 1, [64], 128, 520, 512, CTD(1), s=1, d=1),
    # ---- igemm_fast_bf16_kernel<128, BN, TR, PS, S16>: the gather kernel (stride 2, ConvTranspose, shapes that are no halo shape) --
    brow("fb_s2_odd_plain", "conv", 2, [8], 8, 9, 7, FB(64, 0, 0, 0), stride=2),
    brow("fb_parity_split16", "dgrad", 1, [8], 8, 16, 16, FB(64, 0, 0, 1), s=1, d=1, stride=2, dest="split", split=4),
    brow("fb_odd_affine", "conv", 1, [40], 24, 5, 7, FB(64, 1, 0, 0), acts=["relu"], tabs=["c"]),
    brow("fb_convT_affine16", "convT", 1, [16], 8, 5, 7, FB(64, 1, 0, 1), s=1, d=1, acts=["relu"], tabs=["c"]),
    brow("fb_two_sources_persample", "conv", 2, [32, 8], 40, 6, 10, FB(64, 1, 1, 0), acts=["relu", "none"], tabs=["s", "c"]),
    brow("fb_convT_persample16", "convT", 3, [16], 6, 6, 10, FB(64, 1, 1, 1), s=1, d=1, tabs=["s"]),
    brow("fb_s2_mish", "conv", 1, [8], 8, 5, 7, FB(64, 2, 0, 0), FB(64, 1, 0, 0), stride=2, acts=["mish"], tabs=["c"]),
    brow("fb_convT_dgrad_elu_acc16", "convT_dgrad", 2, [8], 8, 6, 10, FB(64, 2, 0, 1), FB(64, 1, 0, 1), s=1, d=1, acts=["elu"],
         tabs=["c"], dest="acc"),
    brow("fb_s2_mish_persample", "conv", 2, [16], 24, 8, 8, FB(64, 2, 1, 0), FB(64, 1, 1, 0), stride=2, acts=["mish"],
         tabs=["s"]),
    brow("fb_convT_leaky_persample", "convT", 2, [8], 12, 4, 6, FB(64, 2, 1, 1), FB(64, 1, 1, 1), s=1, acts=["leakyrelu"],
         tabs=["s"]),
    brow("fb_wide_dgrad_acc", "dgrad", 1, [72], 136, 12, 21, FB(128, 0, 0, 0), dest="acc"),
    brow("fb_wide_convT_dgrad16", "convT_dgrad", 1, [8], 72, 8, 12, FB(128, 0, 0, 1), s=1, d=1, bias=True),
    brow("fb_wide_s2_relu", "conv", 1, [8], 72, 10, 14, FB(128, 1, 0, 0), stride=2, acts=["relu"]),
    brow("fb_wide_convT_w32_16", "convT", 1, [16], 40, 4, 32, FB(128, 1, 0, 1), s=1, d=1, tabs=["c"]),
    brow("fb_wide_s2_persample_ld", "conv", 2, [8], 72, 6, 10, FB(128, 1, 1, 0), stride=2, tabs=["s"], dest="ld", ldpad=4),
    brow("fb_wide_parity_persample_ld16", "dgrad", 2, [16], 96, 16, 8, FB(128, 1, 1, 1), s=1, d=1, stride=2, acts=["relu"],
         tabs=["s"], dest="ld", ldpad=6, bias=True),
    brow("fb_wide_elu", "conv", 1, [8], 68, 6, 10, FB(128, 2, 0, 0), FB(128, 1, 0, 0), acts=["elu"]),
    brow("fb_wide_convT_mish", "convT", 1, [16], 40, 5, 6, FB(128, 2, 0, 1), FB(128, 1, 0, 1), s=1, acts=["mish"], tabs=["c"]),
    brow("fb_wide_s2_mish_persample", "conv", 2, [8], 68, 7, 9, FB(128, 2, 1, 0), FB(128, 1, 1, 0), stride=2, acts=["mish"],
         tabs=["s"]),
    brow("fb_wide_convT_leaky_persample16", "convT", 2, [16], 40, 2, 6, FB(128, 2, 1, 1), FB(128, 1, 1, 1), s=1, d=1,
         acts=["leakyrelu"], tabs=["s"]),
]

# ---- wgrad_halo_bf16_kernel<T, Q, stride, KW, P, S16>: 3x3 stride 1 (64-pixel blocks 8 x 8 / 16 x 4), 3x3 stride 2 and
# ConvTranspose 2x2 (32-pixel blocks 4 x 8 / 8 x 4); T = 3: rows of 8, T = 2: rows of 4; block rows hang over down to 50 % -----
_TRF = {0: dict(), 1: dict(act="relu", tab="c"), 2: dict(act="mish", tab="s")}
for s16 in (0, 1):
    sfx = "16" if s16 else ""
    c8 = 8 if s16 else 4                                   # bf16 tensors: channel counts are multiples of 8
    for tr in (0, 1, 2):
        a, t = _TRF[tr].get("act", "none"), _TRF[tr].get("tab")
        xq = min(tr, 1)
        # 3x3 stride 1: (N, Q channels, P channels, H, W) for rows of 8 and rows of 4
        for T, (N, cs, Co, H, W) in ((3, [(1, [8], 16, 8, 8), (2, [40], 24, 12, 16), (1, [2 * c8], 16, 4, 24)][tr]),
                                     (2, [(2, [8], 16, 16, 4), (1, [64, 8], 8, 8, 12), (1, [3 * c8], 24, 24, 12)][tr])):
            ROWS.append(brow(f"wb3_t{T}_q{tr}{sfx}", "wgrad3", N, cs, Co, H, W, WB(T, tr, 1, 3, 0, s16), WB(T, xq, 1, 3, 0, s16),
                             s=s16, acts=[a] + ["none"] * (len(cs) - 1), tabs=[t] + [None] * (len(cs) - 1)))
        # 3x3 stride 2: one source
        for T, (N, c, Co, H, W) in ((3, [(1, 8, 16, 4, 8), (2, 8, 16, 6, 16), (1, 16, 8, 2, 8)][tr]),
                                    (2, [(1, 8, 16, 8, 4), (2, 2 * c8, 8, 12, 12), (1, 8, 24, 4, 4)][tr])):
            ROWS.append(brow(f"wb4_t{T}_q{tr}{sfx}", "wgrad3", N, [c], Co, H, W, WB(T, tr, 2, 3, 0, s16), WB(T, xq, 2, 3, 0, s16),
                             s=s16, stride=2, acts=[a], tabs=[t]))
        # ConvTranspose 2x2: P (the layer's input) is the transformed operand, Q (the output gradient) is plain
        for T, (N, c, Co, H, W) in ((3, [(2, 8, 16, 4, 8), (1, 16, 8, 6, 16), (1, 8, 24, 2, 8)][tr]),
                                    (2, [(1, 8, 16, 8, 4), (1, 8, 8, 12, 12), (2, 2 * c8, 16, 4, 4)][tr])):
            ROWS.append(brow(f"wb5_t{T}_p{tr}{sfx}", "wgrad2", N, [c], Co, H, W, WB(T, 0, 2, 2, tr, s16), WB(T, 0, 2, 2, xq, s16),
                             s=s16, pact=a, ptab=t))
ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)

# every bf16 instantiation the dispatch can reach (igemm_dispatch, igemm_p8_try, wgrad_dispatch)
_TB = ((0, 1, 2), (0, 1))
REACHABLE = (
    # igemm_halo_bf16_kernel<128, *, *> is dead (module docstring): not listed
    [HB(tr, s) for tr in _TB[0] for s in _TB[1]]
    + [W4(tr, s) for tr in _TB[0] for s in _TB[1]]
    + [W4M(tr) for tr in _TB[0]]
    + [M512(tr, s) for tr in _TB[0] for s in _TB[1]]
    + [C64P(tr, d) for tr in _TB[0] for d in _TB[1]]
    + [P8(bm, bn, tr, 0) for bm, bn in ((256, 256), (512, 128), (256, 128)) for tr in _TB[0]]
    + [P8(bm, bn, tr, 1) for bm, bn in ((256, 256), (512, 128), (256, 128)) for tr in (0, 1)]
    + [CTP(tr, d) for tr in _TB[0] for d in _TB[1]]
    + [CTP2(tr, d) for tr in _TB[0] for d in _TB[1]]
    + [CTD(d) for d in _TB[1]]
    + [FB(bn, tr, ps, s) for bn in (64, 128) for tr in _TB[0] for ps in ((0,) if tr == 0 else (0, 1)) for s in _TB[1]]
    + [WB(t, q, 1, 3, 0, s) for t in (2, 3) for q in _TB[0] for s in _TB[1]]
    + [WB(t, q, 2, 3, 0, s) for t in (2, 3) for q in _TB[0] for s in _TB[1]]
    + [WB(t, 0, 2, 2, p, s) for t in (2, 3) for p in _TB[0] for s in _TB[1]]
)


def transformed(r, acts, pact):
    """does any operand of the launch go through act / scale / shift (only then can an operand be ambiguous)"""
    return any(a != "none" for a in acts) or pact != "none" or any(r.tabs) or bool(r.opt.get("ptab"))


def _seed(r, extra=0):
    """opt `reseed` (one number per float variant): another seed for a draw that broke the widening condition or came
    within a fifth of its cap (tests/test_conv_ref_host.py; machines differ in the last bit of an fp64 activation)"""
    rs = r.opt.get("reseed", ())
    bump = rs[extra - 1] if 0 < extra <= len(rs) else 0
    return 1000 * ROW_IDS.index(r.id) + 500000 + 17 * bump + extra if r.id in ROW_IDS else extra


@pytest.fixture(scope="module", autouse=True)
def switches():
    """the three process-wide switches at their defaults before anything else; rows select kernels through shapes only"""
    assert "MSEG_P8" not in os.environ, "MSEG_P8 in the environment would change which kernels the rows reach"
    lib = _eng()[2]
    assert lib.mseg_igemm_set_persistent(1) == 0 and lib.mseg_igemm_set_wide_tiles(1) == 0 and lib.mseg_igemm_set_p8(1) == 0
    yield


# =================================================================================================================================
# no device needed: the table against the dispatch
# =================================================================================================================================
@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_row_names_its_kernel(r):
    """the dispatch takes the kernel the table says, in both modes and for every activation of the float mode; the query on
    a full descriptor (placeholder pointers, the row's statistics request included) agrees"""
    xa, xp = exact_acts(r)
    got = engine_query(r, xa, xp)
    nostats = lambda k: k.replace(", true>", ", false>") if k.startswith("igemm_p8_kernel") else k   # engine query: no stats asked
    want_x = nostats(r.xkernel)
    assert got is not None and got.name == want_x and got.bf16, (r.id, "exact", got)
    for acts, pact in float_variants(r):
        got = engine_query(r, acts, pact)
        want = nostats(r.kernel)
        assert got is not None and got.name == want and got.bf16, (r.id, acts, pact, got)
    if r.opt.get("stats"):
        rc, info = _name(_eng()[2], _eng()[2].mseg_igemm_query, _placeholder_igemm(r, xa))
        assert rc == 0 and info.name.decode() == r.xkernel, (r.id, info.name)
        assert (info.stats_rows > 0) == r.kernel.startswith("igemm_p8_kernel"), (r.id, info.stats_rows)


def _placeholder_igemm(r, acts):
    """the row's MsegIgemm with placeholder pointers (16-byte aligned), statistics request included: for the query only"""
    from conv_table import _src, _st
    L = _eng()[1]
    g = geom(r)
    p = L.MsegIgemm()
    for i, (c, a, t) in enumerate(zip(r.cs, acts, r.tabs)):
        p.src[i] = _src(256, c, a, t, dtype=_st(r, "sdt"))
    p.nsrc, p.Cin, p.Kpad, p.Npad = len(r.cs), g["Cin"], g["Kpad"], g["Npad"]
    p.NB, p.Hi, p.Wi, p.Ho, p.Wo = r.N, g["Hi"], g["Wi"], g["Ho"], g["Wo"]
    p.KH = p.KW = g["K"]
    p.stride, p.pad, p.mode, p.morder = g["stride"], g["pad"], g["mode"], g["morder"]
    p.Ngemm, p.epi, p.Cq, p.split = g["Ngemm"], g["epi"], g["Cq"], g["Ngemm"]
    p.precision, p.dst_dtype = 1, _st(r, "ddt")
    p.w = p.dst0 = 256
    p.bias = 256 if g["bias"] else None
    p.ld0, p.acc0 = g["dsts"][0][1], g["dsts"][0][2]
    if len(g["dsts"]) > 1:
        p.dst1, p.ld1, p.split = 256, g["dsts"][1][1], g["dsts"][0][0]
    if r.opt.get("stats"):
        p.stats, p.stats_act = 256, L.ACT[r.opt["stats"]]
    return p


def test_table_covers_every_reachable_instantiation():
    named = {r.kernel for r in ROWS} | {r.xkernel for r in ROWS}
    missing = [k for k in REACHABLE if k not in named]
    assert not missing, "reachable instantiations without a row: " + ", ".join(missing)
    unknown = sorted(named - set(REACHABLE))
    assert not unknown, "rows expect kernels that are not in the reachable list: " + ", ".join(unknown)
    assert len(REACHABLE) == len(set(REACHABLE)) == 112
    # what the rows are to cover besides the instantiations
    ig = [r for r in ROWS if not is_wgrad(r)]
    assert {40, 72, 96} <= {sum(r.cs) for r in ig} and {24, 72, 136, 160} <= {geom(r)["Ngemm"] for r in ig}
    widths = set()
    for r in ROWS:
        if family(r.kernel) in ("igemm_halo_bf16_kernel", "igemm_halo_bf16w4_kernel"):
            tw = 32
            while r.W % tw:
                tw //= 2
            widths.add(tw)
            assert 2 * r.H >= -(-r.H // (128 // tw)) * (128 // tw)
    assert widths == {4, 8, 16, 32}, widths
    assert any(2 * r.H == -(-r.H // (128 // 16)) * (128 // 16) and r.W == 16 for r in ROWS if r.id.startswith(("hb_", "w4_")))
    assert {32, 64} <= {r.cs[0] for r in ig if len(r.cs) == 2}                       # concat boundary
    assert {"c", "s"} <= {t for r in ROWS for t in r.tabs if t}
    sk = [r for r in ROWS if "splitk" in r.opt]
    assert {r.opt["ddt"] for r in sk} == {"f32", "bf16"}
    assert any(r.dest == "acc" and r.opt["ddt"] == "bf16" for r in ig) and any(r.dest == "split" and r.opt["ddt"] == "bf16" for r in ig)
    assert any(9 * geom(r)["Kpad"] * geom(r)["Ngemm"] * 2 > (2 << 20) and geom(r)["Ngemm"] > 128 for r in ig)      # m_fastest
    assert any(geom(r)["morder"] == 1 and geom(r)["out_rows"] % 512 == 0 for r in ig)
    assert any(r.op == "convT" and r.W % 32 != 0 for r in ig) and any(r.op == "convT" and r.W % 32 == 0 for r in ig)


def test_dead_bf16_halo_instantiations():
    """igemm_halo_bf16_kernel<128, *, *> is never chosen: every wide halo launch takes the w4 kernel (or, large enough, a
    persistent one).  Every small wide shape is asked, for both storages and all three operand forms; the same sweep with
    <= 64 output channels does reach igemm_halo_bf16_kernel<64, ...>."""
    seen = set()
    for W in range(4, 68, 4):
        for H in (1, 2, 3, 5, 8, 13, 16, 31, 32, 40):
            for Co in (8, 64, 72, 128, 136, 256):
                for s16 in (0, 1):
                    for act, tab in (("none", None), ("relu", "c"), ("mish", "s")):
                        for cs in ([8], [128], [32, 8]):
                            r = brow("probe", "conv", 2, cs, Co, H, W, "", s=s16, acts=[act] + ["none"] * (len(cs) - 1),
                                     tabs=[tab] + [None] * (len(cs) - 1))
                            got = engine_query(r, r.acts, "none")
                            assert got is not None, (cs, Co, H, W)
                            seen.add(got.name)
    assert any(k.startswith("igemm_halo_bf16_kernel<64") for k in seen) and any(k.startswith("igemm_halo_bf16w4_kernel") for k in seen)
    assert not [k for k in seen if k.startswith("igemm_halo_bf16_kernel<128")], seen


# =================================================================================================================================
# the tests
# =================================================================================================================================
@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _eng()[2]


def _d16(r):
    return r.opt["ddt"] == "bf16"


def check_stats(r, d, got, st):
    """the statistics rows of a launch against the fp64 sums over the output the kernel stored (verified by the caller)"""
    if not r.opt.get("stats"):
        return
    want_rows = r.kernel.startswith("igemm_p8_kernel")
    assert (st["rows"] > 0) == want_rows, (r.id, st["rows"])
    if st["part"] is None:
        return
    z = got.astype(np.float64)
    a = np.maximum(z, 0.0) if r.opt["stats"] == "relu" else z
    count = z.shape[0]
    tol = (count + 32) * U
    part = st["part"].astype(np.float64)
    s1, s2 = part[:, 0, :].sum(0), part[:, 1, :].sum(0)
    e1 = np.abs(s1 - a.sum(0)) / np.maximum(np.abs(a).sum(0), TINY)
    e2 = np.abs(s2 - (a * a).sum(0)) / np.maximum((a * a).sum(0), TINY)
    print(f"CONVBF16STATS {r.id} rows={st['rows']} e_sum={e1.max() / U:.2f}u e_sq={e2.max() / U:.2f}u tol={tol / U:.0f}u")
    assert e1.max() <= tol and e2.max() <= tol, (r.id, e1.max() / U, e2.max() / U)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_exact(gpu, r):
    """small integers: an fp32 destination equals the int64 reference bit for bit, a bf16 one its round-to-nearest-even;
    every sentinel is intact"""
    acts, pact = exact_acts(r)
    d = make_data(r, "exact", acts, pact, _seed(r))
    st = {}
    got = launch(r, d, r.xkernel, st).astype(np.float64)
    ref = d["ref"].astype(np.float64)
    if not is_wgrad(r) and _d16(r):
        ref = CR.round_bf16(ref)
    wrong = np.argwhere(~(got == ref))                      # a NaN left in the destination is wrong too
    assert wrong.shape[0] == 0, (f"{r.id}: {wrong.shape[0]} of {ref.size} elements differ; first at {wrong[0].tolist()}: "
                                 f"got {got[tuple(wrong[0])]}, expected {ref[tuple(wrong[0])]}")
    check_stats(r, d, got, st)


@pytest.mark.gpu
@pytest.mark.parametrize("r", ROWS, ids=ROW_IDS)
def test_float(gpu, r):
    """random operands: per element within max(4 e_ref, floor) and within the worst-case dot-product bound, relative to S,
    each widened by the element's ambiguous operands and, for a bf16 destination, by half a bf16 ulp of the value"""
    K = geom(r)["dot"]
    bound = (K + 32) * U
    floor = FLOOR[family(r.kernel)] * U
    for i, (acts, pact) in enumerate(float_variants(r)):
        d = make_data(r, "float", acts, pact, _seed(r, 1 + i))
        st = {}
        got = launch(r, d, r.kernel, st).astype(np.float64)
        S = np.maximum(d["S"], TINY)
        assert (d["wid"] <= 0.25 * S / K).all(), f"{r.id}: the widening condition does not hold (another seed, never a wider band)"
        allow = d["wid"] / S
        if not is_wgrad(r) and _d16(r):
            allow = allow + 0.5 * CR.bf16_ulp(got) / S               # half a bf16 ulp of the stored value (module docstring)
        e = np.abs(got - d["ref"]) / S
        e_ref = float((np.abs(torch_fp32(r, d).astype(np.float64) - d["ref"]) / S).max())
        net = np.where(np.isnan(e), np.inf, e - allow)
        worst = np.unravel_index(np.argmax(net), e.shape)
        print(f"CONVBF16 {r.id} {family(r.kernel)} acts={','.join(acts)}/{pact} e_hip={e.max() / U:.3f}u "
              f"net={net.max() / U:.3f}u e_ref={e_ref / U:.3f}u bound={bound / U:.0f}u widened={int((d['wid'] > 0).sum())}")
        assert not np.isnan(got).any(), f"{r.id}: NaN left in the destination at {worst}"
        assert net.max() <= max(4 * e_ref, floor), \
            f"{r.id} {acts}/{pact}: e - allowance = {net.max() / U:.2f} u at {worst} (torch fp32 {e_ref / U:.2f} u, floor {floor / U:.2f} u)"
        assert net.max() <= bound, f"{r.id} {acts}/{pact}: e - allowance = {net.max() / U:.2f} u at {worst} beyond {bound / U:.0f} u"
        check_stats(r, d, got, st)


def _refused(lib, p, dsts):
    assert _name(lib, lib.mseg_igemm_query, p)[0] == EINVAL
    assert lib.mseg_igemm(C.byref(p), _stream()) == EINVAL
    assert all(b.untouched() for b in dsts)


@pytest.mark.gpu
def test_refused_descriptors_write_nothing(gpu):
    """MSEG_EINVAL means nothing was launched: every byte of the guarded destinations is unchanged, for the query and the
    call alike.  Each case is one change to a descriptor that is accepted without it (launched last, to show that)."""
    lib = gpu
    by = {r.id: r for r in ROWS}

    def fresh(r, seed):
        d = make_data(r, "exact", *exact_acts(r), seed)
        keep = []
        p, dsts = build_igemm(r, d, keep)
        return p, dsts, keep

    # the generic-kernel shape: a concat boundary that is no multiple of 32 has no bf16 kernel
    r = by["hb_two_sources_split16"]._replace(cs=[8, 32])
    p, dsts, keep = fresh(r, 1)
    _refused(lib, p, dsts)
    # bf16 destination: odd Ngemm, odd ld0, odd split, dst not 4-byte aligned
    r = by["hb_two_sources_split16"]
    for field, value in (("Ngemm", 15), ("ld0", 9), ("split", 7), ("dst0", None), ("dst1", None)):
        p, dsts, keep = fresh(r, 2)
        setattr(p, field, getattr(p, field) + 2 if value is None else value)
        _refused(lib, p, dsts)
    p, dsts, keep = fresh(r, 2)
    assert lib.mseg_igemm(C.byref(p), _stream()) == 0 and not dsts[0].untouched()
    # mixed source storage
    p, dsts, keep = fresh(r, 3)
    p.src[1].dtype = 0
    _refused(lib, p, dsts)
    # bf16 storage with fp32 precision: sources, destination
    p, dsts, keep = fresh(r, 4)
    p.precision = 0
    _refused(lib, p, dsts)
    r = by["hb_w16_overhang_affine_acc16"]                  # fp32 sources, bf16 destination
    p, dsts, keep = fresh(r, 5)
    p.precision = 0
    _refused(lib, p, dsts)
    # stride-2 data gradient in parity order with M % 512 != 0
    r = by["fb_parity_split16"]._replace(H=6, W=10)
    p, dsts, keep = fresh(r, 6)
    assert (p.NB * p.Ho * p.Wo) % 512 != 0
    _refused(lib, p, dsts)
    # weight gradients: mixed storage; bf16 tensors with fp32 precision; a transformed P of the 3x3 forms
    r = by["wb3_t3_q116"]
    for change in ("mixed", "f32", "pact"):
        d = make_data(r, "exact", *exact_acts(r), 7)
        keep = []
        p, dst = build_wgrad(r, d, keep)
        if change == "mixed":
            p.Q[0].dtype = 0
        elif change == "f32":
            p.precision = 0
        else:
            p.P.act = 1
        assert _name(lib, lib.mseg_wgrad_query, p)[0] == EINVAL
        assert lib.mseg_wgrad(C.byref(p), _stream()) == EINVAL
        assert dst.untouched()
