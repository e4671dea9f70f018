// midline.hip — per-cell midline integers of a segmented stack: every cell thinned alone, then counted.
// An extension of the per-cell table (cells.hip, §6l; hull.hip, §6p).
//
// The rule (the authority is the restatement in include/mseg_hip.h).  A cell is the set of pixels of frame t with id l,
// 1 <= l <= K_t; everything else (other cells, ids outside the table, the outside of the frame) is 0 for it.  Thinning is
// Guo & Hall 1989, A1: neighbours clockwise from north, P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW,
//   C  = (!P2 & (P3 | P4)) + (!P4 & (P5 | P6)) + (!P6 & (P7 | P8)) + (!P8 & (P9 | P2))
//   N  = min((P9 | P2) + (P3 | P4) + (P5 | P6) + (P7 | P8),  (P2 | P3) + (P4 | P5) + (P6 | P7) + (P8 | P9))
//   m0 = (P6 | P7 | !P9) & P8,  m1 = (P2 | P3 | !P5) & P4
// sub-pass k deletes every pixel with C == 1, 2 <= N <= 3, m_k == 0, all decisions on the state before the sub-pass; a round
// is sub-pass 0 then 1; rounds repeat until one deletes nothing.
//
// A cell's pixels are bits: (r1 - r0 + 2) rows of ceil((c1 - c0 + 2) / 64) 64-bit words, pixel (y, x) = bit (x - c0 + 1) of
// row (y - r0 + 1), bit b of word j = column 64 j + b.  The ring of one empty pixel around the box means no edge cases.
//   md_fill_kernel  labels [T][H][W], read once, 8 pixels per lane: 64-bit atomicOr of a lane's stretch of one word
//   md_thin_kernel  one group (one wave) per cell slot: the rule on 64 pixels per lane at a time (the neighbours are the shifted words
//                   of the three rows, the sums are bit-sliced: "exactly one of four", "two or more of four"), ping-pong
//                   between the two buffers — in LDS when both fit, in the workspace otherwise — one barrier per sub-pass and
//                   one OR-fold per round; then, on the final bits, the counts, the end points, the scatter of the skeleton
//                   image, and the distance search over the grown box in the labels themselves.
// Integers only, order-free atomics (or / add / min / max): bit-identical from run to run.
#include "cell_common.h"

#define MD_BLOCK 256               // lanes per group of the fill pass
#define MD_GROUP 64                // lanes per group of the thin pass, one group per cell: a typical cell has ~20 words, larger
                                   // ones loop (measured, DESIGN.md 6q: 0.019 ms per frame against 0.037 with 256 lanes)
#define MD_PPL 8                   // consecutive pixels per lane of the fill pass
#define MD_LDS_WORDS 512           // cells of up to this many words are thinned in LDS (2 x 4 KiB)

namespace {

// the bit rows of one cell slot, from the box and the word table; ok: a present cell whose box and words are consistent
struct MdCell {
  int r0, c0, r1, c1;
  int64_t wo;                      // first word
  int nr, nw;                      // rows and words per row, the empty ring included: nr * nw < 2^31 as H * W is
  bool present, ok;
};

__device__ __forceinline__ MdCell md_cell(const int32_t* __restrict__ bbox, const int64_t* __restrict__ word_off, int64_t s,
                                          int64_t n_words, int H, int W) {
  MdCell c;
  const int32_t* bp = bbox + 4 * s;
  c.r0 = bp[0]; c.c0 = bp[1]; c.r1 = bp[2]; c.c1 = bp[3];
  c.present = c.r1 > c.r0 && c.c1 > c.c0;
  c.wo = word_off[s];
  c.nr = c.present ? c.r1 - c.r0 + 2 : 0;
  c.nw = c.present ? (int)(((int64_t)c.c1 - c.c0 + 2 + 63) >> 6) : 0;
  c.ok = c.present && c.r0 >= 0 && c.c0 >= 0 && c.r1 <= H && c.c1 <= W && c.wo >= 0 &&
         word_off[s + 1] - c.wo == (int64_t)c.nr * c.nw && c.wo + (int64_t)c.nr * c.nw <= n_words;
  return c;
}

// ---- a. fill pass -------------------------------------------------------------------------------------------------------
// A lane owns 8 consecutive pixels of a frame (flat order).  The bits of a stretch that falls into one word of one cell go
// out in one atomicOr.  A pixel outside the box given for its cell, or of a cell whose words do not match its box, is skipped
// and sets bit 0 of the status word.
template <typename L>
__global__ void __launch_bounds__(MD_BLOCK) md_fill_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                           const int64_t* __restrict__ loff,
                                                           const int32_t* __restrict__ bbox,
                                                           const int64_t* __restrict__ word_off, int64_t n_words,
                                                           u64* __restrict__ bits, int32_t* __restrict__ status) {
  const int HW = H * W;
  const int64_t groups = ((int64_t)HW + MD_PPL - 1) / MD_PPL;
  const int64_t g = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
  if (g >= (int64_t)T * groups) return;
  const int t = (int)(g / groups);
  const int p0 = (int)(g - (int64_t)t * groups) * MD_PPL;
  const int64_t base = loff[t], K = loff[t + 1] - base;
  int e[MD_PPL];
  cell_load8<L>(lab + (int64_t)t * HW, p0, HW, e);
  bool any = false;
#pragma unroll
  for (int k = 0; k < MD_PPL; ++k) {
    e[k] = cell_id(e[k], K);
    any |= e[k] > 0;
  }
  if (!any) return;
  int y = p0 / W, x = p0 - y * W;
  int cur = 0;
  MdCell c = {};
  int64_t pw = -1;
  u64 pm = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < MD_PPL; ++k) {
    const int l = e[k];
    if (l > 0) {
      if (l != cur) {
        c = md_cell(bbox, word_off, base + l - 1, n_words, H, W);
        cur = l;
      }
      if (c.ok && y >= c.r0 && y < c.r1 && x >= c.c0 && x < c.c1) {
        const int col = x - c.c0 + 1;
        const int64_t w = c.wo + (int64_t)(y - c.r0 + 1) * c.nw + (col >> 6);
        if (w != pw) {
          if (pm) atomicOr(&bits[pw], pm);
          pw = w;
          pm = 0;
        }
        pm |= 1ull << (col & 63);
      } else {
        bad = true;
      }
    }
    if (++x == W) { x = 0; ++y; }
  }
  if (pm) atomicOr(&bits[pw], pm);
  if (bad) atomicOr(status, 1);
}

// ---- b. thin and measure ------------------------------------------------------------------------------------------------
// the word (r, j) of a cell's bit rows and its eight neighbour words: bit b of P4 is the pixel right of bit b, and so on
struct MdNb {
  u64 c, P2, P3, P4, P5, P6, P7, P8, P9;
};

__device__ __forceinline__ u64 md_east(const u64* row, int j, int nw) {
  return (row[j] >> 1) | (j + 1 < nw ? row[j + 1] << 63 : 0ull);
}
__device__ __forceinline__ u64 md_west(const u64* row, int j) { return (row[j] << 1) | (j > 0 ? row[j - 1] >> 63 : 0ull); }

__device__ __forceinline__ MdNb md_neighbours(const u64* buf, int r, int j, int nw) {
  const u64 *up = buf + (r - 1) * nw, *mid = buf + r * nw, *dn = buf + (r + 1) * nw;
  MdNb n;
  n.c = mid[j];
  n.P2 = up[j];  n.P3 = md_east(up, j, nw);  n.P9 = md_west(up, j);
  n.P4 = md_east(mid, j, nw);                n.P8 = md_west(mid, j);
  n.P6 = dn[j];  n.P5 = md_east(dn, j, nw);  n.P7 = md_west(dn, j);
  return n;
}

__device__ __forceinline__ u64 md_two_or_more(u64 a, u64 b, u64 c, u64 d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }

// the pixels sub-pass k deletes from word n.c
__device__ __forceinline__ u64 md_deletable(const MdNb& n, int k) {
  const u64 a = n.P9 | n.P2, b = n.P3 | n.P4, c = n.P5 | n.P6, d = n.P7 | n.P8;             // the terms of N1
  const u64 e = n.P2 | n.P3, f = n.P4 | n.P5, g = n.P6 | n.P7, h = n.P8 | n.P9;             // the terms of N2
  const u64 t1 = ~n.P2 & b, t2 = ~n.P4 & c, t3 = ~n.P6 & d, t4 = ~n.P8 & a;                 // the terms of C
  const u64 c_is_1 = (t1 ^ t2 ^ t3 ^ t4) & ~md_two_or_more(t1, t2, t3, t4);                 // odd and below two
  // 2 <= min(N1, N2) <= 3: both sums reach 2 and not both are 4
  const u64 n_ok = md_two_or_more(a, b, c, d) & md_two_or_more(e, f, g, h) & ~(a & b & c & d & e & f & g & h);
  const u64 keep = k == 0 ? (n.P6 | n.P7 | ~n.P9) & n.P8 : (n.P2 | n.P3 | ~n.P5) & n.P4;
  return n.c & c_is_1 & n_ok & ~keep;
}

// one sub-pass over the inner rows of a cell: src -> dst; true: this lane deleted something
__device__ __forceinline__ bool md_subpass(const u64* src, u64* dst, int nr, int nw, int k) {
  bool deleted = false;
  const int inner = (nr - 2) * nw;
  for (int i = threadIdx.x; i < inner; i += MD_GROUP) {
    const int r = 1 + i / nw, j = i - (r - 1) * nw;
    u64 v = src[r * nw + j];
    if (v) {
      const u64 del = md_deletable(md_neighbours(src, r, j, nw), k);
      deleted |= del != 0;
      v &= ~del;
    }
    dst[r * nw + j] = v;
  }
  return deleted;
}

// rounds until one deletes nothing, at most cap of them; the survivors end in a.  -> rounds run, 0: the cap was hit
__device__ __forceinline__ int64_t md_thin(u64* a, u64* b, int nr, int nw, int64_t cap) {
  for (int i = threadIdx.x; i < nw; i += MD_GROUP) {            // the ring rows of b; a has them from the fill pass
    b[i] = 0;
    b[(nr - 1) * nw + i] = 0;
  }
  __syncthreads();
  for (int64_t rounds = 1; rounds <= cap; ++rounds) {
    bool deleted = md_subpass(a, b, nr, nw, 0);
    __syncthreads();
    deleted |= md_subpass(b, a, nr, nw, 1);
    if (!__syncthreads_or(deleted)) return rounds;
  }
  return 0;
}

struct MdSums {                     // folded over the group in LDS
  unsigned long long skel_n, n_orth, n_diag, n_end, n_branch;
  unsigned long long first_end, last_end, first_pix;              // keys: row * 64 nw + column of the bit rows
  unsigned long long d2[2];
};

// the counts and the end points of the final bits S; the skeleton image, if asked for
__device__ __forceinline__ void md_count(const u64* S, const MdCell& c, MdSums* sums, uint8_t* __restrict__ skel_frame, int W) {
  unsigned n = 0, orth = 0, diag = 0, ends = 0, branch = 0;
  u64 kmin = ~0ull, kmax = 0, pmin = ~0ull;
  const int inner = (c.nr - 2) * c.nw;
  for (int i = threadIdx.x; i < inner; i += MD_GROUP) {
    const int r = 1 + i / c.nw, j = i - (r - 1) * c.nw;
    if (S[r * c.nw + j] == 0) continue;
    const MdNb q = md_neighbours(S, r, j, c.nw);
    const u64 P[8] = {q.P2, q.P3, q.P4, q.P5, q.P6, q.P7, q.P8, q.P9};
    n += __popcll(q.c);
    orth += __popcll(q.c & q.P4) + __popcll(q.c & q.P6);            // every pair once: with the right and the lower pixel
    diag += __popcll(q.c & q.P5 & ~q.P4 & ~q.P6) + __popcll(q.c & q.P7 & ~q.P8 & ~q.P6);
    u64 one = 0, more = 0;                                          // one: odd number of neighbours, more: two or more
    u64 b0 = 0, b1 = 0, four = 0;                                   // the 0 -> 1 steps round the pixel, counted in two bits
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      more |= one & P[k];
      one ^= P[k];
      const u64 step = ~P[k] & P[(k + 1) & 7];
      const u64 carry = b0 & step;
      b0 ^= step;
      four |= b1 & carry;
      b1 ^= carry;
    }
    const u64 e = q.c & one & ~more;
    ends += __popcll(e);
    branch += __popcll(q.c & (four | (b1 & b0)));
    const u64 key = (u64)r * (u64)(64ll * c.nw) + (u64)(64ll * j);
    if (e) {
      kmin = min(kmin, key + (u64)(__ffsll((long long)e) - 1));
      kmax = max(kmax, key + (u64)(63 - __clzll((long long)e)));
    }
    pmin = min(pmin, key + (u64)(__ffsll((long long)q.c) - 1));
    if (skel_frame) {
      const int64_t y = (int64_t)c.r0 + r - 1;
      for (u64 m = q.c; m; m &= m - 1) {
        const int64_t x = (int64_t)c.c0 - 1 + 64ll * j + (__ffsll((long long)m) - 1);
        skel_frame[y * W + x] = 1;                                  // inside the box: the fill pass sets no other bit
      }
    }
  }
  if (n) {
    atomicAdd(&sums->skel_n, (unsigned long long)n);
    atomicMin(&sums->first_pix, pmin);
    if (orth) atomicAdd(&sums->n_orth, (unsigned long long)orth);
    if (diag) atomicAdd(&sums->n_diag, (unsigned long long)diag);
    if (branch) atomicAdd(&sums->n_branch, (unsigned long long)branch);
    if (ends) {
      atomicAdd(&sums->n_end, (unsigned long long)ends);
      atomicMin(&sums->first_end, kmin);
      atomicMax(&sums->last_end, kmax);
    }
  }
}

// One group per cell slot.
template <typename L>
__global__ void __launch_bounds__(MD_GROUP) md_thin_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                           const int64_t* __restrict__ loff, int64_t n,
                                                           const int32_t* __restrict__ bbox,
                                                           const int64_t* __restrict__ word_off, int64_t n_words,
                                                           u64* bits_a, u64* bits_b,
                                                           int64_t* __restrict__ out, uint8_t* __restrict__ skeleton,
                                                           int32_t* __restrict__ status) {
  __shared__ u64 lds_a[MD_LDS_WORDS], lds_b[MD_LDS_WORDS];
  __shared__ MdSums sums;
  const int64_t s = blockIdx.x;
  const MdCell c = md_cell(bbox, word_off, s, n_words, H, W);       // group-uniform
  if (!c.ok) {
    for (int p = threadIdx.x; p < 12; p += MD_GROUP) out[(int64_t)p * n + s] = 0;
    if (c.present && threadIdx.x == 0) atomicOr(status, 1);
    return;
  }
  int t = 0;                                                        // the frame of slot s: loff[t] <= s < loff[t + 1]
  for (int lo = 0, hi = T; hi - lo > 1;) {
    const int mid = (lo + hi) >> 1;
    if (loff[mid] <= s) lo = mid; else hi = mid;
    t = lo;
  }
  const int l = (int)(s - loff[t]) + 1;
  if (threadIdx.x == 0) {
    sums.skel_n = sums.n_orth = sums.n_diag = sums.n_end = sums.n_branch = 0;
    sums.first_end = sums.first_pix = ~0ull;
    sums.last_end = 0;
    sums.d2[0] = sums.d2[1] = ~0ull;
  }
  const int words = c.nr * c.nw;
  const int64_t cap = (int64_t)(c.r1 - c.r0) + (c.c1 - c.c0) + 2;
  u64* ga = bits_a + c.wo;
  u64* gb = bits_b + c.wo;
  uint8_t* skel_frame = skeleton ? skeleton + (int64_t)t * H * W : nullptr;
  int64_t rounds;
  if (words <= MD_LDS_WORDS) {
    for (int i = threadIdx.x; i < words; i += MD_GROUP) lds_a[i] = ga[i];
    rounds = md_thin(lds_a, lds_b, c.nr, c.nw, cap);                // begins with a barrier
    md_count(lds_a, c, &sums, skel_frame, W);
  } else {
    __syncthreads();                                                // sums is set
    rounds = md_thin(ga, gb, c.nr, c.nw, cap);
    md_count(ga, c, &sums, skel_frame, W);
  }
  __syncthreads();
  const bool one_pixel = sums.skel_n == 1;
  const bool has_ends = one_pixel || sums.n_end > 0;
  const u64 stride = (u64)(64ll * c.nw);
  const u64 k0 = one_pixel ? sums.first_pix : sums.first_end, k1 = one_pixel ? sums.first_pix : sums.last_end;
  const int64_t y0 = c.r0 - 1 + (int64_t)(k0 / stride), x0 = c.c0 - 1 + (int64_t)(k0 % stride);
  const int64_t y1 = c.r0 - 1 + (int64_t)(k1 / stride), x1 = c.c0 - 1 + (int64_t)(k1 % stride);
  if (has_ends) {
    // the nearest position that is not of the cell, over the box grown by one pixel (it holds one: DESIGN.md §6q)
    const L* frame = lab + (int64_t)t * H * W;
    const int64_t cols = (int64_t)c.c1 - c.c0 + 2, total = (int64_t)c.nr * cols;
    u64 d0 = ~0ull, d1 = ~0ull;
    for (int64_t i = threadIdx.x; i < total; i += MD_GROUP) {
      const int64_t y = c.r0 - 1 + i / cols, x = c.c0 - 1 + i % cols;
      if (y >= 0 && y < H && x >= 0 && x < W && (int)frame[y * W + x] == l) continue;
      d0 = min(d0, (u64)((y - y0) * (y - y0) + (x - x0) * (x - x0)));
      d1 = min(d1, (u64)((y - y1) * (y - y1) + (x - x1) * (x - x1)));
    }
    if (d0 != ~0ull) {
      atomicMin(&sums.d2[0], d0);
      atomicMin(&sums.d2[1], d1);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0 * n + s] = (int64_t)sums.skel_n;
    out[1 * n + s] = (int64_t)sums.n_orth;
    out[2 * n + s] = (int64_t)sums.n_diag;
    out[3 * n + s] = (int64_t)sums.n_end;
    out[4 * n + s] = (int64_t)sums.n_branch;
    out[5 * n + s] = rounds;
    out[6 * n + s] = has_ends ? y0 : 0;
    out[7 * n + s] = has_ends ? x0 : 0;
    out[8 * n + s] = has_ends ? (int64_t)sums.d2[0] : 0;
    out[9 * n + s] = has_ends ? y1 : 0;
    out[10 * n + s] = has_ends ? x1 : 0;
    out[11 * n + s] = has_ends ? (int64_t)sums.d2[1] : 0;
    if (rounds == 0) atomicOr(status, 2);
  }
}

}  // namespace

// ---- entry points -------------------------------------------------------------------------------------------------------
extern "C" size_t mseg_cell_midline_workspace_bytes(int64_t n_labels, int64_t n_words) {
  if (n_labels < 0 || n_words < 0 || n_words > (1ll << 40)) return 0;
  return 2 * mseg_align256((size_t)(n_words > 0 ? n_words : 1) * sizeof(u64));
}

extern "C" int mseg_cell_midline(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off,
                                 int64_t n_labels, const int32_t* bbox, const int64_t* word_off, int64_t n_words,
                                 int64_t* out, uint8_t* skeleton, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!cell_stack_ok(labels, label_off, dtype, T, H, W, 512) || !status || !ws || n_labels < 0 || n_words < 0) return MSEG_EINVAL;
  if (n_labels > 0 && (!bbox || !word_off || !out)) return MSEG_EINVAL;
  const size_t need = mseg_cell_midline_workspace_bytes(n_labels, n_words);
  if (need == 0) return MSEG_EINVAL;
  const int64_t lanes = (int64_t)T * (((int64_t)H * W + MD_PPL - 1) / MD_PPL);
  if ((lanes + MD_BLOCK - 1) / MD_BLOCK > 0x7FFFFFFFll || n_labels > 0x7FFFFFFFll) return MSEG_EINVAL;
  if (ws_bytes < need) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return MSEG_ELAUNCH;
  if (skeleton && hipMemsetAsync(skeleton, 0, (size_t)T * H * W, st) != hipSuccess) return MSEG_ELAUNCH;
  if (n_labels == 0) return MSEG_OK;                                // no cell, no kernel
  u64* bits_a = (u64*)ws;
  u64* bits_b = (u64*)((char*)ws + need / 2);
  if (hipMemsetAsync(bits_a, 0, need / 2, st) != hipSuccess) return MSEG_ELAUNCH;
  cell_dispatch(dtype, [&](auto l) {
    typedef decltype(l) L;
    hipLaunchKernelGGL(md_fill_kernel<L>, dim3(mseg_blocks(lanes, MD_BLOCK)), dim3(MD_BLOCK), 0, st, (const L*)labels, T, H, W,
                       label_off, bbox, word_off, n_words, bits_a, status);
    hipLaunchKernelGGL(md_thin_kernel<L>, dim3((unsigned)n_labels), dim3(MD_GROUP), 0, st, (const L*)labels, T, H, W,
                       label_off, n_labels, bbox, word_off, n_words, bits_a, bits_b, out, skeleton, status);
  });
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
