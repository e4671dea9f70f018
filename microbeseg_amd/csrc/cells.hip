// cells.hip — the per-cell table of a segmented stack: shape and intensity sums per cell, overlap links between frames
// (DESIGN.md §6l).  An extension: the reference stops at the per-frame means of mseg_region_stats (analysis.hip).
//
//   mseg_cell_measure  labels [T][H][W] (+ C channels of the image, read in place through four strides) -> per cell the
//                      integer sums of a regionprops row (area, first / second coordinate moments, bounding box) and per
//                      cell and channel sum / sum of squares / min / max; the same per frame over the background
//   mseg_cell_links    per cell of frame t the label of frame t - 1 that shares the most pixels with it
//   mseg_cell_links_shifted  the same with frame t - 1 moved by a per-pair integer shift (drift compensation, §6o)
//   mseg_cell_links_field    the same with one integer shift per tile of frame t (tile-wise displacement field, §6v)
//   mseg_cell_links_gap      the same against frame t - gap, between flagged cells only (gap closing, §6w)
// Everything is integer arithmetic with order-free 64-bit atomics: bit-identical from run to run.
#include "cell_common.h"

#define CM_BLOCK 256
#define CM_WAVES (CM_BLOCK / 64)
#define CM_PPL 8                  // consecutive pixels per lane: 16 bytes of uint16 labels or image, two loads of int32
#define CM_CHUNK (64 * CM_PPL)    // pixels of one wave step
#define CM_MAXC 4                 // channels per launch; more channels go in groups (the labels are read once per group)
#define CL_MIN_CAP 64

namespace {

// ---- a. measure ---------------------------------------------------------------------------------------------------------
struct CmOut {
  u64* shape;          // [6][n]: area, sum_y, sum_x, sum_yy, sum_xx, sum_xy
  int32_t* bbox;       // [n][4]
  u64* ch_sums;        // [2][C][n]: sum, sum_sq
  uint32_t* ch_mm;     // [2][C][n]: min, max
  u64* bg_sums;        // [3][T][C]: count, sum, sum_sq
  uint32_t* bg_mm;     // [2][T][C]: min, max
  int64_t n;
  int T, C;
};

template <int NC>
struct CmAcc {                      // intensity part of a run (or of a lane's background pixels)
  unsigned cnt;
  u64 s[NC > 0 ? NC : 1], q[NC > 0 ? NC : 1];
  uint32_t mn[NC > 0 ? NC : 1], mx[NC > 0 ? NC : 1];
  __device__ __forceinline__ void clear() {
    cnt = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) { s[c] = 0; q[c] = 0; mn[c] = 0xFFFFFFFFu; mx[c] = 0; }
  }
  __device__ __forceinline__ void merge(const CmAcc& o) {
    cnt += o.cnt;
#pragma unroll
    for (int c = 0; c < NC; ++c) { s[c] += o.s[c]; q[c] += o.q[c]; mn[c] = min(mn[c], o.mn[c]); mx[c] = max(mx[c], o.mx[c]); }
  }
  __device__ __forceinline__ CmAcc down(int d) const {
    CmAcc r;
    r.cnt = __shfl_down(cnt, d, 64);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      r.s[c] = __shfl_down(s[c], d, 64); r.q[c] = __shfl_down(q[c], d, 64);
      r.mn[c] = __shfl_down(mn[c], d, 64); r.mx[c] = __shfl_down(mx[c], d, 64);
    }
    return r;
  }
};

// One horizontal run of label l (row y, columns x0 .. x0 + cnt - 1) into slot s: the closed forms of rs_runs_kernel
template <int NC>
__device__ __forceinline__ void cm_flush_run(const CmOut& o, int64_t s, int y, int x0, const CmAcc<NC>& r, int ch0,
                                             bool shape) {
  const u64 len = r.cnt;
  if (shape) {
    const u64 yy = (u64)y, a = (u64)x0, b = a + len - 1;
    const u64 sx = (a + b) * len / 2;
    const int64_t n = o.n;
    atomicAdd(&o.shape[s], len);
    atomicAdd(&o.shape[n + s], yy * len);
    atomicAdd(&o.shape[2 * n + s], sx);
    atomicAdd(&o.shape[3 * n + s], yy * yy * len);
    atomicAdd(&o.shape[4 * n + s], run_sum_sq(a, b));
    atomicAdd(&o.shape[5 * n + s], yy * sx);
    int32_t* bb = o.bbox + 4 * s;
    atomicMin(&bb[0], y);
    atomicMin(&bb[1], x0);
    atomicMax(&bb[2], y + 1);
    atomicMax(&bb[3], x0 + (int)len);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int64_t e = (int64_t)(ch0 + c) * o.n + s, plane = (int64_t)o.C * o.n;
    atomicAdd(&o.ch_sums[e], r.s[c]);
    atomicAdd(&o.ch_sums[plane + e], r.q[c]);
    atomicMin(&o.ch_mm[e], r.mn[c]);
    atomicMax(&o.ch_mm[plane + e], r.mx[c]);
  }
}

// the wave's background pixels of frame t: folded over the lanes, one lane adds them
template <int NC>
__device__ __forceinline__ void cm_flush_bg(const CmOut& o, int t, u64 cnt, const CmAcc<NC>& b, int ch0) {
  if (NC == 0) return;
  u64 n = cnt;
  CmAcc<NC> r = b;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    n += __shfl_xor(n, d, 64);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      r.s[c] += __shfl_xor(r.s[c], d, 64); r.q[c] += __shfl_xor(r.q[c], d, 64);
      r.mn[c] = min(r.mn[c], (uint32_t)__shfl_xor(r.mn[c], d, 64));
      r.mx[c] = max(r.mx[c], (uint32_t)__shfl_xor(r.mx[c], d, 64));
    }
  }
  if ((threadIdx.x & 63) != 0 || n == 0) return;
  const int64_t plane = (int64_t)o.T * o.C;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int64_t e = (int64_t)t * o.C + ch0 + c;
    atomicAdd(&o.bg_sums[e], n);
    atomicAdd(&o.bg_sums[plane + e], r.s[c]);
    atomicAdd(&o.bg_sums[2 * plane + e], r.q[c]);
    atomicMin(&o.bg_mm[e], r.mn[c]);
    atomicMax(&o.bg_mm[plane + e], r.mx[c]);
  }
}

// A wave owns a contiguous range of (frame, 512-pixel chunk) steps; a chunk never leaves its frame.  A lane folds its 8
// pixels into horizontal runs of one label (a run ends at the row end).  Runs that stay inside the lane are added by the
// lane; the piece at the lane's start that continues the previous lane's run ("head") is handed to the lane where that run
// begins by a segmented suffix scan over the wave, so a run that spans lanes costs one set of atomics.  A run is cut at the
// wave's first and last lane.  Background pixels (label 0) collect in lane registers until the wave changes frame.
template <typename L, typename P, int NC>
__global__ void __launch_bounds__(CM_BLOCK) cm_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                      const int64_t* __restrict__ loff, const P* __restrict__ img,
                                                      int64_t fs, int64_t cs, int64_t rs, int64_t ps, int ch0, int shape,
                                                      CmOut o) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * CM_BLOCK + threadIdx.x) >> 6, nwaves = (int64_t)gridDim.x * CM_WAVES;
  const int HW = H * W;
  const int64_t chunks = ((int64_t)HW + CM_CHUNK - 1) / CM_CHUNK, steps = (int64_t)T * chunks;
  const int64_t per = (steps + nwaves - 1) / nwaves;
  const int64_t it0 = wave * per, it1 = min(steps, it0 + per);
  const bool img_flat = ps == 1 && rs == W;      // a frame's channel plane is contiguous: vector loads where aligned
  int tcur = -1;
  int64_t K = 0, base = 0;
  u64 bg_cnt = 0;
  CmAcc<NC> bg;
  bg.clear();
  for (int64_t it = it0; it < it1; ++it) {
    const int t = (int)(it / chunks);
    const int p0 = (int)(it - (int64_t)t * chunks) * CM_CHUNK + lane * CM_PPL;
    if (t != tcur) {
      if (tcur >= 0) cm_flush_bg<NC>(o, tcur, bg_cnt, bg, ch0);
      bg_cnt = 0;
      bg.clear();
      tcur = t;
      base = loff[t];
      K = loff[t + 1] - base;
    }
    const int nvalid = max(0, min(CM_PPL, HW - p0));
    int l[CM_PPL];
    cell_load8<L>(lab + (int64_t)t * HW, p0, HW, l);
    int y = nvalid ? p0 / W : 0, x = nvalid ? p0 - y * W : 0;
    const int y_first = y, x_first = x;
    int v[NC > 0 ? NC : 1][CM_PPL];
    if (NC > 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const P* ip = img + (int64_t)t * fs + (int64_t)(ch0 + c) * cs;
        if (img_flat) {
          cell_load8<P>(ip, p0, HW, v[c]);
        } else {
          int yy = y, xx = x;
#pragma unroll
          for (int k = 0; k < CM_PPL; ++k) {
            v[c][k] = k < nvalid ? (int)ip[(int64_t)yy * rs + (int64_t)xx * ps] : 0;
            if (++xx == W) { xx = 0; ++yy; }
          }
        }
      }
    }
    // run label of a pixel: its id if the frame's table holds it, else 0 (no run); background is the raw label 0
    int e[CM_PPL];
#pragma unroll
    for (int k = 0; k < CM_PPL; ++k) e[k] = cell_id(l[k], K);       // 0 past the frame's end
    const int prev_last = __shfl_up(e[CM_PPL - 1], 1, 64);
    const bool link_in = lane > 0 && e[0] > 0 && prev_last == e[0] && x_first != 0;
    const unsigned long long links = __ballot(link_in);
    const bool link_out = lane < 63 && ((links >> (lane + 1)) & 1ull);

    CmAcc<NC> cur, head;
    cur.clear();
    head.clear();
    int cur_l = 0, cur_y = y_first, cur_x0 = x_first;
    bool cur_is_head = false;
#pragma unroll
    for (int k = 0; k < CM_PPL; ++k) {
      if (k > 0 && (e[k] != cur_l || x == 0) && cur_l > 0) {     // the run ends before pixel k
        if (cur_is_head) head = cur;
        else cm_flush_run<NC>(o, base + cur_l - 1, cur_y, cur_x0, cur, ch0, shape != 0);
        cur_l = 0;
      }
      if (e[k] > 0) {
        if (cur_l == 0) {
          cur.clear();
          cur_l = e[k]; cur_y = y; cur_x0 = x;
          cur_is_head = k == 0 && link_in;
        }
        cur.cnt += 1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const uint32_t pv = (uint32_t)v[c][k];
          cur.s[c] += pv; cur.q[c] += (u64)pv * pv; cur.mn[c] = min(cur.mn[c], pv); cur.mx[c] = max(cur.mx[c], pv);
        }
      } else if (NC > 0 && k < nvalid && l[k] == 0) {
        bg_cnt += 1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const uint32_t pv = (uint32_t)v[c][k];
          bg.s[c] += pv; bg.q[c] += (u64)pv * pv; bg.mn[c] = min(bg.mn[c], pv); bg.mx[c] = max(bg.mx[c], pv);
        }
      }
      if (++x == W) { x = 0; ++y; }
    }
    // here cur is the lane's last run if cur_l > 0; a lane that is one run from a linked start to its end is all head
    const bool whole_is_head = cur_l > 0 && cur_is_head;
    if (whole_is_head) head = cur;
    if (links) {                                                   // wave-uniform
      // R(lane) = the run piece from this lane's first pixel to the run's end: head + (run goes on ? R(lane + 1) : 0)
      CmAcc<NC> R = head;
      bool go = whole_is_head && link_out;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const CmAcc<NC> Rd = R.down(d);
        const int god = __shfl_down((int)go, d, 64);
        if (go) { R.merge(Rd); go = god != 0; }
      }
      const CmAcc<NC> Rn = R.down(1);
      if (cur_l > 0 && !cur_is_head && link_out) cur.merge(Rn);
    }
    if (cur_l > 0 && !cur_is_head) cm_flush_run<NC>(o, base + cur_l - 1, cur_y, cur_x0, cur, ch0, shape != 0);
  }
  if (tcur >= 0) cm_flush_bg<NC>(o, tcur, bg_cnt, bg, ch0);
}

__global__ void cm_init_kernel(CmOut o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = o.n, nc = (int64_t)o.C * n, tc = (int64_t)o.T * o.C;
  if (i < 6 * n) o.shape[i] = 0;
  if (i < 4 * n) o.bbox[i] = (i & 3) < 2 ? INT32_MAX : 0;
  if (i < 2 * nc) { o.ch_sums[i] = 0; o.ch_mm[i] = i < nc ? 0xFFFFFFFFu : 0u; }
  if (i < 3 * tc) o.bg_sums[i] = 0;
  if (i < 2 * tc) o.bg_mm[i] = i < tc ? 0xFFFFFFFFu : 0u;
}

// absent cells (area 0) and frames without background: bounding box and minimum 0 instead of the identity elements
__global__ void cm_finish_kernel(CmOut o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < o.n && o.shape[i] == 0) {
    o.bbox[4 * i] = 0; o.bbox[4 * i + 1] = 0;
    for (int c = 0; c < o.C; ++c) o.ch_mm[(int64_t)c * o.n + i] = 0;
  }
  if (i < (int64_t)o.T * o.C && o.bg_sums[i] == 0) o.bg_mm[i] = 0;
}

template <typename L, typename P>
void cm_launch(int nc, unsigned grid, hipStream_t st, const void* lab, int T, int H, int W, const int64_t* loff,
               const void* img, int64_t fs, int64_t cs, int64_t rs, int64_t ps, int ch0, int shape, const CmOut& o) {
#define CM_GO(N)                                                                                                        \
  hipLaunchKernelGGL((cm_kernel<L, P, N>), dim3(grid), dim3(CM_BLOCK), 0, st, (const L*)lab, T, H, W, loff, (const P*)img, \
                     fs, cs, rs, ps, ch0, shape, o)
  switch (nc) {
    case 0: CM_GO(0); break;
    case 1: CM_GO(1); break;
    case 2: CM_GO(2); break;
    case 3: CM_GO(3); break;
    default: CM_GO(4); break;
  }
#undef CM_GO
}

// ---- b. links -------------------------------------------------------------------------------------------------------------
// len pixels of the pair (l, m) into the open-addressing table of one frame pair; a full table sets the pair's status
__device__ __forceinline__ void cl_insert(u64* __restrict__ keys, uint32_t* __restrict__ cnt, uint32_t mask, uint32_t l,
                                          uint32_t m, uint32_t len, int32_t* __restrict__ status) {
  const uint32_t h = cell_pair_slot<false>(keys, mask, l, m, status);
  if (h <= mask) atomicAdd(&cnt[h], len);
}

// a lane's 8 pixels of frame t (l) and the pixels of frame t - 1 under them (m), folded into runs of one pair of cells: one
// insert per run.  Pixels past the frame's (the row's) end are 0 in l.
__device__ __forceinline__ void cl_fold8(const int (&l)[CM_PPL], const int (&m)[CM_PPL], const int64_t* __restrict__ loff,
                                         int t, u64* __restrict__ keys, uint32_t* __restrict__ cnt, uint32_t cap,
                                         int32_t* __restrict__ status) {
  const int64_t Kl = loff[t + 1] - loff[t], Km = loff[t] - loff[t - 1];
  u64* kt = keys + (size_t)(t - 1) * cap;
  uint32_t* ct = cnt + (size_t)(t - 1) * cap;
  int cl = 0, cm = 0;
  uint32_t len = 0;
#pragma unroll
  for (int k = 0; k < CM_PPL; ++k) {
    const bool ok = cell_id(l[k], Kl) && cell_id(m[k], Km);
    if (len && (!ok || l[k] != cl || m[k] != cm)) { cl_insert(kt, ct, cap - 1, cl, cm, len, status + t); len = 0; }
    if (ok) { cl = l[k]; cm = m[k]; ++len; }
  }
  if (len) cl_insert(kt, ct, cap - 1, cl, cm, len, status + t);
}

// A lane folds 8 consecutive pixels of frames t - 1 and t (flat order: both loads are aligned whenever the frames are)
template <typename L>
__global__ void __launch_bounds__(CM_BLOCK) cl_pairs_kernel(const L* __restrict__ lab, int T, int HW,
                                                            const int64_t* __restrict__ loff, u64* __restrict__ keys,
                                                            uint32_t* __restrict__ cnt, uint32_t cap,
                                                            int32_t* __restrict__ status) {
  const int64_t groups = ((int64_t)HW + CM_PPL - 1) / CM_PPL;
  const int64_t g = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
  if (g >= (int64_t)(T - 1) * groups) return;
  const int t = (int)(g / groups) + 1;
  const int p0 = (int)(g - (int64_t)(t - 1) * groups) * CM_PPL;
  int l[CM_PPL], m[CM_PPL];
  cell_load8<L>(lab + (int64_t)t * HW, p0, HW, l);
  cell_load8<L>(lab + (int64_t)(t - 1) * HW, p0, HW, m);
  cl_fold8(l, m, loff, t, keys, cnt, cap, status);
}

// The pairs under a per-pair shift: pixel (y, x) of frame t pairs with (y - dy_t, x - dx_t) of frame t - 1.  A lane folds 8
// consecutive pixels of ONE row of frame t (the shifted source is contiguous within a row only, so a run never crosses a
// row end); the frame t - 1 pixels are in general unaligned and partly outside the frame: scalar loads under a bounds test.
// FIELD: shift is [T][ty][tx][2], one (dy, dx) per tile x tile pixels of frame t (§6v); a lane's 8 pixels start at a multiple
// of 8 and the tile is one, so they lie in one tile: the same kernel with a per-lane lookup.
template <typename L, bool FIELD>
__global__ void __launch_bounds__(CM_BLOCK) cl_pairs_shifted_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                                    const int64_t* __restrict__ loff,
                                                                    const int32_t* __restrict__ shift, int tile,
                                                                    u64* __restrict__ keys, uint32_t* __restrict__ cnt,
                                                                    uint32_t cap, int32_t* __restrict__ status) {
  const int64_t per_row = ((int64_t)W + CM_PPL - 1) / CM_PPL, groups = (int64_t)H * per_row;
  const int64_t g = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
  if (g >= (int64_t)(T - 1) * groups) return;
  const int t = (int)(g / groups) + 1;
  const int64_t in_frame = g - (int64_t)(t - 1) * groups;
  const int y = (int)(in_frame / per_row);
  const int x0 = (int)(in_frame - (int64_t)y * per_row) * CM_PPL;
  int64_t at = t;
  if (FIELD) at = ((int64_t)t * ((H + tile - 1) / tile) + y / tile) * ((W + tile - 1) / tile) + x0 / tile;
  const int64_t ys = (int64_t)y - shift[2 * at], xs0 = (int64_t)x0 - shift[2 * at + 1];
  if (ys < 0 || ys >= H || xs0 + CM_PPL <= 0 || xs0 >= W) return;      // no pixel of this lane has a source
  const int nvalid = min(CM_PPL, W - x0);
  const L* pm = lab + ((int64_t)(t - 1) * H + ys) * W;                  // the source row
  int l[CM_PPL], m[CM_PPL];
  cell_load8<L>(lab + ((int64_t)t * H + y) * W, x0, W, l);
#pragma unroll
  for (int k = 0; k < CM_PPL; ++k) {
    const int64_t xs = xs0 + k;
    m[k] = (k < nvalid && xs >= 0 && xs < W) ? (int)pm[xs] : 0;
  }
  cl_fold8(l, m, loff, t, keys, cnt, cap, status);
}

// The pairs across a gap (§6w): pixel (y, x) of frame t pairs with (y - dy, x - dx) of frame t - gap, for the cells of frame t
// flagged in want and the cells of frame t - gap flagged in open only (bytes in label_off order).  The lane layout of the
// shifted kernel, 8 pixels of one row; shift == nullptr: no motion, else one (dy, dx) per frame or (FIELD) per tile of frame t,
// composed over the gap by the caller.  The wanted cells are few: a lane none of whose pixels belongs to one returns
// before it touches frame t - gap, and only wanted pixels load their source.  A flag is read where a run of one id starts, and
// only for an id that cell_id let pass: 1 .. K of its frame, so the index stays inside the frame's part of the array.  The
// table of frame t keeps index t - 1: those of the frames below gap stay empty.
template <typename L, bool FIELD>
__global__ void __launch_bounds__(CM_BLOCK) cl_pairs_gap_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                                const int64_t* __restrict__ loff, int gap,
                                                                const int32_t* __restrict__ shift, int tile,
                                                                const uint8_t* __restrict__ want,
                                                                const uint8_t* __restrict__ open, u64* __restrict__ keys,
                                                                uint32_t* __restrict__ cnt, uint32_t cap,
                                                                int32_t* __restrict__ status) {
  const int64_t per_row = ((int64_t)W + CM_PPL - 1) / CM_PPL, groups = (int64_t)H * per_row;
  const int64_t g = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x;
  if (g >= (int64_t)(T - gap) * groups) return;
  const int t = (int)(g / groups) + gap, ts = t - gap;
  const int64_t in_frame = g - (int64_t)ts * groups;
  const int y = (int)(in_frame / per_row);
  const int x0 = (int)(in_frame - (int64_t)y * per_row) * CM_PPL;
  const int64_t Kl = loff[t + 1] - loff[t], Km = loff[ts + 1] - loff[ts];
  const uint8_t* wt = want + loff[t];
  const uint8_t* os = open + loff[ts];
  int l[CM_PPL], m[CM_PPL];
  cell_load8<L>(lab + ((int64_t)t * H + y) * W, x0, W, l);               // positions past the row's end read as 0
  int run = 0;
  bool flag = false, any = false;
#pragma unroll
  for (int k = 0; k < CM_PPL; ++k) {
    const int v = cell_id(l[k], Kl);
    if (v != run) { run = v; flag = v && wt[v - 1]; }
    l[k] = flag ? v : 0;
    any |= flag;
  }
  if (!any) return;
  int64_t ys = y, xs0 = x0;
  if (shift) {
    int64_t at = t;
    if (FIELD) at = ((int64_t)t * ((H + tile - 1) / tile) + y / tile) * ((W + tile - 1) / tile) + x0 / tile;
    ys -= shift[2 * at];
    xs0 -= shift[2 * at + 1];
  }
  if (ys < 0 || ys >= H || xs0 + CM_PPL <= 0 || xs0 >= W) return;        // no pixel of this lane has a source
  const L* pm = lab + ((int64_t)ts * H + ys) * W;                        // the source row
#pragma unroll
  for (int k = 0; k < CM_PPL; ++k) {
    const int64_t xs = xs0 + k;
    m[k] = (l[k] && xs >= 0 && xs < W) ? cell_id((int)pm[xs], Km) : 0;
  }
  u64* kt = keys + (size_t)(t - 1) * cap;
  uint32_t* ct = cnt + (size_t)(t - 1) * cap;
  int cl = 0, cm = 0;
  uint32_t len = 0;
  run = 0; flag = false;
#pragma unroll
  for (int k = 0; k < CM_PPL; ++k) {
    if (m[k] != run) { run = m[k]; flag = run && os[run - 1]; }
    const bool ok = l[k] && flag;
    if (len && (!ok || l[k] != cl || m[k] != cm)) { cl_insert(kt, ct, cap - 1, cl, cm, len, status + t); len = 0; }
    if (ok) { cl = l[k]; cm = m[k]; ++len; }
  }
  if (len) cl_insert(kt, ct, cap - 1, cl, cm, len, status + t);
}

// every table entry: best[cell] = max(count << 32 | ~m): the largest overlap, ties to the smallest m
__global__ void cl_best_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ cnt, int64_t entries, uint32_t cap,
                               const int64_t* __restrict__ loff, u64* __restrict__ best) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= entries) return;
  const u64 k = keys[i];
  if (k == 0) return;
  const int t = (int)(i / cap) + 1;
  const uint32_t l = (uint32_t)(k >> 32), m = (uint32_t)k;
  atomicMax(&best[loff[t] + l - 1], (u64)cnt[i] << 32 | (uint32_t)~m);
}

__global__ void cl_out_kernel(const u64* __restrict__ best, int64_t n, int32_t* __restrict__ pred,
                              int32_t* __restrict__ overlap) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const u64 b = best[s];
  pred[s] = b ? (int32_t)~(uint32_t)b : 0;
  overlap[s] = (int32_t)(b >> 32);
}

}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------
extern "C" int mseg_cell_measure(const void* labels, int label_dtype, int T, int H, int W, const int64_t* label_off,
                                 int64_t n_labels, const void* img, int img_dtype, int C, int64_t frame_stride,
                                 int64_t chan_stride, int64_t row_stride, int64_t pix_stride, uint64_t* shape,
                                 int32_t* bbox, uint64_t* ch_sums, uint32_t* ch_minmax, uint64_t* bg_sums,
                                 uint32_t* bg_minmax, void* stream) {
  if (!cell_stack_ok(labels, label_off, label_dtype, T, H, W, CM_CHUNK) || n_labels < 0 || C < 0) return MSEG_EINVAL;
  if (!img) C = 0;
  if (C > 0 && !cell_image_ok(img_dtype)) return MSEG_EINVAL;
  if (C > 0 && (!bg_sums || !bg_minmax)) return MSEG_EINVAL;
  if (n_labels > 0 && (!shape || !bbox || (C > 0 && (!ch_sums || !ch_minmax)))) return MSEG_EINVAL;
  if (n_labels == 0 && C == 0) return MSEG_OK;
  hipStream_t st = (hipStream_t)stream;
  CmOut o;
  o.shape = (u64*)shape; o.bbox = bbox; o.ch_sums = (u64*)ch_sums; o.ch_mm = ch_minmax;
  o.bg_sums = (u64*)bg_sums; o.bg_mm = bg_minmax; o.n = n_labels; o.T = T; o.C = C;
  const int64_t tc = (int64_t)T * C;
  int64_t items = 6 * n_labels;
  if (2 * C * n_labels > items) items = 2 * C * n_labels;
  if (3 * tc > items) items = 3 * tc;
  hipLaunchKernelGGL(cm_init_kernel, dim3(mseg_blocks(items, CM_BLOCK)), dim3(CM_BLOCK), 0, st, o);
  const int64_t steps = (int64_t)T * (((int64_t)H * W + CM_CHUNK - 1) / CM_CHUNK);
  // at most 4 workgroups per compute unit's worth of waves: every wave flushes its background sums once per frame it
  // meets, so fewer, longer waves keep those same-address atomics few
  const int64_t want = (steps + CM_WAVES - 1) / CM_WAVES;
  const unsigned grid = (unsigned)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
  int ch0 = 0;
  do {
    const int nc = C - ch0 > CM_MAXC ? CM_MAXC : C - ch0;
    const int sh = ch0 == 0;
    // without channels the image type is not checked and not used: the uint16 instantiation
    cell_dispatch(label_dtype, nc > 0 ? img_dtype : MSEG_PIX_U16, [&](auto l, auto p) {
      cm_launch<decltype(l), decltype(p)>(nc, grid, st, labels, T, H, W, label_off, img, frame_stride, chan_stride,
                                          row_stride, pix_stride, ch0, sh, o);
    });
    ch0 += nc;
  } while (ch0 < C);
  int64_t fin = n_labels > tc ? n_labels : tc;
  hipLaunchKernelGGL(cm_finish_kernel, dim3(mseg_blocks(fin, CM_BLOCK)), dim3(CM_BLOCK), 0, st, o);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

extern "C" size_t mseg_cell_links_workspace_bytes(int T, int64_t n_labels, int64_t table_cap) {
  if (T <= 0 || n_labels < 0 || table_cap < CL_MIN_CAP || table_cap > (1ll << 31) || (table_cap & (table_cap - 1))) return 0;
  const size_t pairs = (size_t)(T > 1 ? T - 1 : 1);
  return mseg_align256(pairs * (size_t)table_cap * sizeof(u64)) + mseg_align256(pairs * (size_t)table_cap * sizeof(uint32_t)) +
         mseg_align256((size_t)(n_labels + 1) * sizeof(u64));
}

// The four links calls.  shift == nullptr: same (y, x) in both frames (cl_pairs_kernel: both frames by vector loads);
// tile == 0: shift is [T][2], one (dy, dx) per frame pair; else [T][ty][tx][2], one per tile x tile pixels of frame t.
// want: frame t against frame t - gap, between the flagged cells only (cl_pairs_gap_kernel); nullptr: gap is 1, all cells
static int cl_links(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                    int64_t table_cap, const int32_t* shift, int tile, int gap, const uint8_t* want, const uint8_t* open,
                    int32_t* pred, int32_t* overlap, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!cell_stack_ok(labels, label_off, dtype, T, H, W, CM_PPL) || !status || !ws || n_labels < 0) return MSEG_EINVAL;
  if (n_labels > 0 && (!pred || !overlap)) return MSEG_EINVAL;
  const size_t need = mseg_cell_links_workspace_bytes(T, n_labels, table_cap);
  if (need == 0) return MSEG_EINVAL;
  if (ws_bytes < need) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)T, st) != hipSuccess) return MSEG_ELAUNCH;
  if (n_labels == 0) return MSEG_OK;
  const size_t pairs = (size_t)(T > 1 ? T - 1 : 1);
  const uint32_t cap = (uint32_t)table_cap;
  char* b = (char*)ws;
  u64* keys = (u64*)b;
  uint32_t* cnt = (uint32_t*)(b + mseg_align256(pairs * (size_t)cap * sizeof(u64)));
  u64* best = (u64*)((char*)cnt + mseg_align256(pairs * (size_t)cap * sizeof(uint32_t)));
  if (hipMemsetAsync(ws, 0, need, st) != hipSuccess) return MSEG_ELAUNCH;
  if (T > gap) {
    // lanes: 8 pixels each, in flat order without a shift, row by row with one and across a gap
    const int64_t lanes = shift || want ? (int64_t)(T - gap) * H * (((int64_t)W + CM_PPL - 1) / CM_PPL)
                                        : (int64_t)(T - 1) * (((int64_t)H * W + CM_PPL - 1) / CM_PPL);
    const dim3 grid(mseg_blocks(lanes, CM_BLOCK)), block(CM_BLOCK);
    cell_dispatch(dtype, [&](auto l) {
      typedef decltype(l) L;
      const L* lab = (const L*)labels;
      if (want && tile)
        hipLaunchKernelGGL((cl_pairs_gap_kernel<L, true>), grid, block, 0, st, lab, T, H, W, label_off, gap, shift, tile, want,
                           open, keys, cnt, cap, status);
      else if (want)
        hipLaunchKernelGGL((cl_pairs_gap_kernel<L, false>), grid, block, 0, st, lab, T, H, W, label_off, gap, shift, tile, want,
                           open, keys, cnt, cap, status);
      else if (!shift)
        hipLaunchKernelGGL(cl_pairs_kernel<L>, grid, block, 0, st, lab, T, H * W, label_off, keys, cnt, cap, status);
      else if (tile)
        hipLaunchKernelGGL((cl_pairs_shifted_kernel<L, true>), grid, block, 0, st, lab, T, H, W, label_off, shift, tile, keys,
                           cnt, cap, status);
      else
        hipLaunchKernelGGL((cl_pairs_shifted_kernel<L, false>), grid, block, 0, st, lab, T, H, W, label_off, shift, tile, keys,
                           cnt, cap, status);
    });
    const int64_t entries = (int64_t)(T - 1) * cap;
    hipLaunchKernelGGL(cl_best_kernel, dim3(mseg_blocks(entries, CM_BLOCK)), block, 0, st, (const u64*)keys,
                       (const uint32_t*)cnt, entries, cap, label_off, best);
  }
  hipLaunchKernelGGL(cl_out_kernel, dim3(mseg_blocks(n_labels, CM_BLOCK)), dim3(CM_BLOCK), 0, st, (const u64*)best, n_labels,
                     pred, overlap);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

extern "C" int mseg_cell_links(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off,
                               int64_t n_labels, int64_t table_cap, int32_t* pred, int32_t* overlap, int32_t* status,
                               void* ws, size_t ws_bytes, void* stream) {
  return cl_links(labels, dtype, T, H, W, label_off, n_labels, table_cap, nullptr, 0, 1, nullptr, nullptr, pred, overlap,
                  status, ws, ws_bytes, stream);
}

extern "C" int mseg_cell_links_shifted(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off,
                                       int64_t n_labels, int64_t table_cap, const int32_t* shift, int32_t* pred,
                                       int32_t* overlap, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!shift) return MSEG_EINVAL;
  return cl_links(labels, dtype, T, H, W, label_off, n_labels, table_cap, shift, 0, 1, nullptr, nullptr, pred, overlap,
                  status, ws, ws_bytes, stream);
}

extern "C" int mseg_cell_links_field(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off,
                                     int64_t n_labels, int64_t table_cap, int tile, const int32_t* field, int32_t* pred,
                                     int32_t* overlap, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!field || (tile != 64 && tile != 128 && tile != 256)) return MSEG_EINVAL;
  return cl_links(labels, dtype, T, H, W, label_off, n_labels, table_cap, field, tile, 1, nullptr, nullptr, pred, overlap,
                  status, ws, ws_bytes, stream);
}

extern "C" int mseg_cell_links_gap(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off,
                                   int64_t n_labels, int64_t table_cap, int gap, int tile, const int32_t* shift,
                                   const uint8_t* want, const uint8_t* open, int32_t* pred, int32_t* overlap,
                                   int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (gap < 1 || gap > 5 || !want || !open) return MSEG_EINVAL;
  if (shift ? (tile != 0 && tile != 64 && tile != 128 && tile != 256) : tile != 0) return MSEG_EINVAL;
  return cl_links(labels, dtype, T, H, W, label_off, n_labels, table_cap, shift, tile, gap, want, open, pred, overlap, status,
                  ws, ws_bytes, stream);
}
