// order_stats.hip — per-cell and per-frame-background order statistics of a segmented stack: the element of a given rank in
// the ascending multiset of a cell's pixel values.  An extension of the per-cell table (cells.hip, §6l).
//
// Exact radix select by histogram: the high byte of a value picks one of 256 bins, a prefix over the bins finds the bin a
// rank falls into and the rank left inside it; for uint16 a second walk counts the low bytes of the pixels of the chosen
// bins only.  uint8 values are their own bin: one walk decides.
//   os_cell_kernel   one wave (one workgroup of 64) per cell slot, channels in a loop; histograms in LDS, no global atomics
//   os_bg_hist_kernel<.., 0>  whole frames: private LDS histogram of the label-0 pixels per workgroup, merged into the
//                    workspace with integer atomics
//   os_bg_pick_kernel   one wave per (frame, channel): the bin and the rank left in it for each of the R ranks
//   os_bg_hist_kernel<.., 1>  uint16: the low-byte histograms of the chosen bins
//   os_bg_low_kernel    one wave per (frame, channel): the values
// Integers only, order-free integer adds: identical bytes from run to run.
#include "cell_common.h"

#define OS_WAVE 64
#define OS_MAXR 16
#define OS_BINS 256
#define OS_BG_BLOCK 256
#define OS_BG_SHARE 65536         // background pixels of one frame and channel a workgroup walks: 256 per thread

namespace {

struct OsSel {                    // where a rank fell in the high-byte histogram
  int32_t bin;                    // the bin, -1: the rank is not in 0 .. m - 1 (or there is no pixel at all)
  uint32_t rem;                   // the rank left inside the bin
  int32_t slot;                   // the low-byte histogram of the bin: the first rank j' <= j with the same bin
  int32_t none;                   // 1: no pixel at all (an absent background): zeros, the rank is not read as a rank
};

struct OsWs {
  uint32_t* hi;                   // [T * C][256]
  uint32_t* low;                  // [T * C][R][256]
  OsSel* sel;                     // [T * C][R]
};

inline OsWs os_carve(void* ws, int T, int C, int R) {
  const size_t tc = (size_t)T * C;
  char* b = (char*)ws;
  OsWs w;
  w.hi = (uint32_t*)b;
  w.low = (uint32_t*)(b + mseg_align256(tc * OS_BINS * 4));
  w.sel = (OsSel*)(b + mseg_align256(tc * OS_BINS * 4) + mseg_align256(tc * R * OS_BINS * 4));
  return w;
}

// 256 counters, lane i holds bins 4 i .. 4 i + 3 in c[]: the exclusive prefix of the lane's first bin and the total
__device__ __forceinline__ void os_scan(const uint32_t (&c)[4], int lane, uint32_t& excl, uint32_t& total) {
  const uint32_t own = c[0] + c[1] + c[2] + c[3];
  uint32_t inc = own;
#pragma unroll
  for (int d = 1; d < OS_WAVE; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, OS_WAVE);
    if (lane >= d) inc += o;
  }
  excl = inc - own;
  total = __shfl(inc, OS_WAVE - 1, OS_WAVE);
}

// the bin of rank r < total among the lane's four bins: (bin, rank left) on exactly one lane, which returns true
__device__ __forceinline__ bool os_find(const uint32_t (&c)[4], uint32_t excl, int lane, uint32_t r, int& bin, uint32_t& rem) {
  uint32_t lo = excl;
  bool hit = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!hit && r >= lo && r - lo < c[k]) { hit = true; bin = 4 * lane + k; rem = r - lo; }
    lo += c[k];
  }
  return hit;
}

// (bin, rem) of the one lane that hit, for all lanes
__device__ __forceinline__ void os_spread(bool hit, int& bin, uint32_t& rem) {
  const unsigned long long m = __ballot(hit);
  const int src = m ? __ffsll((long long)m) - 1 : 0;
  bin = __shfl(bin, src, OS_WAVE);
  rem = __shfl(rem, src, OS_WAVE);
}

// ---- a. cells: one wave per slot --------------------------------------------------------------------------------------------
// The wave walks the cell's box in flat order (cell_walk, cell_common.h).
template <typename L, typename P>
__global__ void __launch_bounds__(OS_WAVE) os_cell_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                          const int64_t* __restrict__ loff, int64_t n,
                                                          const P* __restrict__ img, int C, int64_t fs, int64_t cs, int64_t rs,
                                                          int64_t ps, const int32_t* __restrict__ bbox, int R,
                                                          const int64_t* __restrict__ ranks, uint32_t* __restrict__ values,
                                                          int32_t* __restrict__ status) {
  constexpr bool WIDE = sizeof(P) == 2;
  __shared__ uint32_t hist[OS_BINS];                               // high bytes; on the second walk: bin -> low histogram
  __shared__ uint32_t low[WIDE ? OS_MAXR * OS_BINS : 1];
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  if (s >= n) return;
  const int4 bb = make_int4(bbox[4 * s], bbox[4 * s + 1], bbox[4 * s + 2], bbox[4 * s + 3]);      // r0, c0, r1, c1
  if ((bb.x | bb.y | bb.z | bb.w) == 0) {                           // absent: zeros, the ranks are not read
    for (int e = lane; e < R * C; e += OS_WAVE) values[(int64_t)e * n + s] = 0;
    return;
  }
  const int t = cell_slot_frame(loff, T, s);
  // the box, clipped to the frame (cell_common.h).  A box that misses pixels of the cell shows as a rank beyond the
  // pixels found.
  const CellWalk box = cell_walk_box(bb, H, W, s - loff[t] + 1);
  const L* frame = lab + (int64_t)t * H * W;
  bool bad = false;
  for (int c = 0; c < C; ++c) {
    const P* plane = img + (int64_t)t * fs + (int64_t)c * cs;
#pragma unroll
    for (int k = 0; k < 4; ++k) hist[4 * lane + k] = 0;
    __syncthreads();
    cell_walk(frame, W, box, lane, [&](int y, int x) {
      const unsigned v = plane[(int64_t)y * rs + (int64_t)x * ps];
      atomicAdd(&hist[WIDE ? v >> 8 : v], 1u);
    });
    __syncthreads();
    uint32_t cnt[4], excl, m;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] = hist[4 * lane + k];
    os_scan(cnt, lane, excl, m);
    // lane j keeps the record of rank j
    int my_bin = -1, my_slot = -1;
    uint32_t my_rem = 0;
    for (int j = 0; j < R; ++j) {
      const int64_t r = ranks[(int64_t)j * n + s];
      int bin = -1;
      uint32_t rem = 0;
      if (r >= 0 && r < (int64_t)m) {                               // wave-uniform
        const bool hit = os_find(cnt, excl, lane, (uint32_t)r, bin, rem);
        os_spread(hit, bin, rem);
      } else {
        bad = true;
      }
      if (lane == j) { my_bin = bin; my_rem = rem; }
    }
    if (!WIDE) {
      if (lane < R) values[((int64_t)lane * C + c) * n + s] = my_bin >= 0 ? (uint32_t)my_bin : 0u;
      __syncthreads();                                              // hist is cleared next
      continue;
    }
    // ranks of one bin share the low histogram of the first of them
    for (int j = R - 1; j >= 0; --j) {
      const int bj = __shfl(my_bin, j, OS_WAVE);
      if (lane >= j && my_bin >= 0 && my_bin == bj) my_slot = j;
    }
    __syncthreads();                                                // every lane has read its counters
#pragma unroll
    for (int k = 0; k < 4; ++k) hist[4 * lane + k] = 0xFFFFFFFFu;
    for (int e = lane; e < R * OS_BINS; e += OS_WAVE) low[e] = 0;
    __syncthreads();
    if (lane < R && my_bin >= 0 && my_slot == lane) hist[my_bin] = (uint32_t)lane;
    __syncthreads();
    cell_walk(frame, W, box, lane, [&](int y, int x) {
      const unsigned v = plane[(int64_t)y * rs + (int64_t)x * ps];
      const uint32_t slot = hist[(v >> 8) & 0xFF];
      if (slot < (uint32_t)OS_MAXR) atomicAdd(&low[slot * OS_BINS + (v & 0xFF)], 1u);
    });
    __syncthreads();
    for (int j = 0; j < R; ++j) {
      const int bin = __shfl(my_bin, j, OS_WAVE), slot = __shfl(my_slot, j, OS_WAVE);
      const uint32_t rem = __shfl(my_rem, j, OS_WAVE);
      uint32_t out = 0;
      if (bin >= 0 && slot >= 0 && slot < R) {                      // wave-uniform
        uint32_t lc[4], lex, ltot;
#pragma unroll
        for (int k = 0; k < 4; ++k) lc[k] = low[slot * OS_BINS + 4 * lane + k];
        os_scan(lc, lane, lex, ltot);
        int lb = 0;
        uint32_t lrem = 0;
        const bool hit = rem < ltot && os_find(lc, lex, lane, rem, lb, lrem);
        os_spread(hit, lb, lrem);
        if (rem < ltot) out = ((uint32_t)bin << 8) | (uint32_t)lb;
        else bad = true;                                            // cannot happen: both walks read the same pixels
      }
      if (lane == 0) values[((int64_t)j * C + c) * n + s] = out;
    }
    __syncthreads();
  }
  if (bad && lane == 0) atomicOr(status, 1);
}

// ---- b. background: whole frames ----------------------------------------------------------------------------------------------
// PASS 0: the high-byte (uint8: the value's) histogram of the label-0 pixels.  PASS 1 (uint16): the low-byte histograms of
// the bins the ranks fell into.  Workgroup b of (t, c) walks pixels b * OS_BG_SHARE ... of the frame, a thread every 256th.
template <typename L, typename P, int PASS>
__global__ void __launch_bounds__(OS_BG_BLOCK) os_bg_hist_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                                 const P* __restrict__ img, int C, int64_t fs, int64_t cs,
                                                                 int64_t rs, int64_t ps, int R, unsigned bpf, OsWs w) {
  constexpr bool WIDE = sizeof(P) == 2;
  constexpr int NL = PASS == 0 ? OS_BINS : OS_MAXR * OS_BINS;
  __shared__ uint32_t h[NL];
  __shared__ uint32_t slot_of[PASS == 0 ? 1 : OS_BINS];
  const int tid = threadIdx.x;
  const unsigned tc = blockIdx.x / bpf, b = blockIdx.x - tc * bpf;
  if (tc >= (unsigned)(T * C)) return;
  const int t = (int)(tc / (unsigned)C), c = (int)(tc - (unsigned)t * (unsigned)C);
  const int nl = PASS == 0 ? OS_BINS : R * OS_BINS;
  for (int e = tid; e < nl; e += OS_BG_BLOCK) h[e] = 0;
  if (PASS == 1) {
    slot_of[tid] = 0xFFFFFFFFu;
    __syncthreads();
    if (tid < R) {
      const OsSel sel = w.sel[(size_t)tc * R + tid];
      if (sel.bin >= 0 && sel.bin < OS_BINS && sel.slot == tid) slot_of[sel.bin] = (uint32_t)tid;
    }
  }
  __syncthreads();
  const int HW = H * W;
  const L* frame = lab + (int64_t)t * HW;
  const P* plane = img + (int64_t)t * fs + (int64_t)c * cs;
  const bool flat = ps == 1 && rs == W;
  const int64_t p_end = min((int64_t)HW, ((int64_t)b + 1) * OS_BG_SHARE);
  for (int64_t p = (int64_t)b * OS_BG_SHARE + tid; p - tid < p_end; p += OS_BG_BLOCK) {
    // the bound is the same for all threads: the ballots below need whole waves to the end of the share
    const bool in = p < p_end;
    bool bg = false;
    unsigned v = 0;
    if (in && frame[p] == 0) {
      bg = true;
      if (flat) {
        v = plane[p];
      } else {
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        v = plane[(int64_t)y * rs + (int64_t)x * ps];
      }
    }
    if (PASS == 0) {
      // a dark, flat background puts most of a wave into one bin: one add of the lane count then, not 64 adds in turn
      const unsigned bin = WIDE ? v >> 8 : v;
      const unsigned long long act = __ballot(bg);
      if (act) {
        const unsigned first = __shfl(bin, __ffsll((long long)act) - 1, OS_WAVE);
        const unsigned long long same = __ballot(bg && bin == first);
        if (same == act) {
          if ((tid & 63) == __ffsll((long long)act) - 1) atomicAdd(&h[first], (uint32_t)__popcll(act));
        } else if (bg) {
          atomicAdd(&h[bin], 1u);
        }
      }
    } else if (bg) {
      const uint32_t slot = slot_of[(v >> 8) & 0xFF];
      if (slot < (uint32_t)OS_MAXR) atomicAdd(&h[slot * OS_BINS + (v & 0xFF)], 1u);
    }
  }
  __syncthreads();
  uint32_t* dst = PASS == 0 ? w.hi + (size_t)tc * OS_BINS : w.low + (size_t)tc * R * OS_BINS;
  for (int e = tid; e < nl; e += OS_BG_BLOCK)
    if (h[e]) atomicAdd(&dst[e], h[e]);
}

// one wave per (t, c): where the R ranks fall in the high-byte histogram.  uint8 (WIDE == 0): that is the value.
__global__ void __launch_bounds__(OS_WAVE) os_bg_pick_kernel(int T, int C, int R, int wide, const int64_t* __restrict__ bg_ranks,
                                                             uint32_t* __restrict__ bg_values, int32_t* __restrict__ status,
                                                             OsWs w) {
  const int lane = threadIdx.x;
  const unsigned tc = blockIdx.x;
  const int t = (int)(tc / (unsigned)C), c = (int)(tc - (unsigned)t * (unsigned)C);
  uint32_t cnt[4], excl, m;
#pragma unroll
  for (int k = 0; k < 4; ++k) cnt[k] = w.hi[(size_t)tc * OS_BINS + 4 * lane + k];
  os_scan(cnt, lane, excl, m);
  int my_bin = -1, my_slot = -1;
  uint32_t my_rem = 0;
  bool bad = false;
  for (int j = 0; j < R; ++j) {
    const int64_t r = bg_ranks[(int64_t)j * T + t];
    int bin = -1;
    uint32_t rem = 0;
    if (m == 0) {
      // a frame without background: zeros, the rank is not read as a rank
    } else if (r >= 0 && r < (int64_t)m) {
      const bool hit = os_find(cnt, excl, lane, (uint32_t)r, bin, rem);
      os_spread(hit, bin, rem);
    } else {
      bad = true;
    }
    if (lane == j) { my_bin = bin; my_rem = rem; }
  }
  for (int j = R - 1; j >= 0; --j) {
    const int bj = __shfl(my_bin, j, OS_WAVE);
    if (lane >= j && my_bin >= 0 && my_bin == bj) my_slot = j;
  }
  if (lane < R) {
    OsSel sel;
    sel.bin = my_bin; sel.rem = my_rem; sel.slot = my_slot; sel.none = m == 0;
    w.sel[(size_t)tc * R + lane] = sel;
    if (!wide || my_bin < 0) bg_values[((int64_t)lane * T + t) * C + c] = my_bin >= 0 ? (uint32_t)my_bin : 0u;
  }
  if (bad && lane == 0) atomicOr(status, 1);
}

// one wave per (t, c), uint16: the low byte of every rank that fell into a bin
__global__ void __launch_bounds__(OS_WAVE) os_bg_low_kernel(int T, int C, int R, uint32_t* __restrict__ bg_values,
                                                            int32_t* __restrict__ status, OsWs w) {
  const int lane = threadIdx.x;
  const unsigned tc = blockIdx.x;
  const int t = (int)(tc / (unsigned)C), c = (int)(tc - (unsigned)t * (unsigned)C);
  bool bad = false;
  for (int j = 0; j < R; ++j) {
    const OsSel sel = w.sel[(size_t)tc * R + j];
    if (sel.bin < 0 || sel.slot < 0 || sel.slot >= R) continue;   // pick wrote the zero
    uint32_t lc[4], lex, ltot;
#pragma unroll
    for (int k = 0; k < 4; ++k) lc[k] = w.low[((size_t)tc * R + sel.slot) * OS_BINS + 4 * lane + k];
    os_scan(lc, lane, lex, ltot);
    int lb = 0;
    uint32_t lrem = 0;
    const bool hit = sel.rem < ltot && os_find(lc, lex, lane, sel.rem, lb, lrem);
    os_spread(hit, lb, lrem);
    uint32_t out = 0;
    if (sel.rem < ltot) out = ((uint32_t)sel.bin << 8) | (uint32_t)lb;
    else bad = true;                                                // cannot happen: both passes read the same pixels
    if (lane == 0) bg_values[((int64_t)j * T + t) * C + c] = out;
  }
  if (bad && lane == 0) atomicOr(status, 1);
}

template <typename L, typename P>
void os_launch(hipStream_t st, const void* labels, int T, int H, int W, const int64_t* loff, int64_t n, const void* img, int C,
               int64_t fs, int64_t cs, int64_t rs, int64_t ps, const int32_t* bbox, int R, const int64_t* ranks,
               const int64_t* bg_ranks, uint32_t* values, uint32_t* bg_values, int32_t* status, const OsWs& w) {
  constexpr bool WIDE = sizeof(P) == 2;
  const L* lab = (const L*)labels;
  const P* im = (const P*)img;
  if (n > 0)
    hipLaunchKernelGGL((os_cell_kernel<L, P>), dim3((unsigned)n), dim3(OS_WAVE), 0, st, lab, T, H, W, loff, n, im, C, fs, cs,
                       rs, ps, bbox, R, ranks, values, status);
  const unsigned bpf = (unsigned)(((int64_t)H * W + OS_BG_SHARE - 1) / OS_BG_SHARE);
  const unsigned tc = (unsigned)(T * C);
  hipLaunchKernelGGL((os_bg_hist_kernel<L, P, 0>), dim3(tc * bpf), dim3(OS_BG_BLOCK), 0, st, lab, T, H, W, im, C, fs, cs, rs,
                     ps, R, bpf, w);
  hipLaunchKernelGGL(os_bg_pick_kernel, dim3(tc), dim3(OS_WAVE), 0, st, T, C, R, (int)WIDE, bg_ranks, bg_values, status, w);
  if (WIDE) {
    hipLaunchKernelGGL((os_bg_hist_kernel<L, P, 1>), dim3(tc * bpf), dim3(OS_BG_BLOCK), 0, st, lab, T, H, W, im, C, fs, cs, rs,
                       ps, R, bpf, w);
    hipLaunchKernelGGL(os_bg_low_kernel, dim3(tc), dim3(OS_WAVE), 0, st, T, C, R, bg_values, status, w);
  }
}

}  // namespace

// ---- entry points -------------------------------------------------------------------------------------------------------
extern "C" size_t mseg_cell_order_stats_workspace_bytes(int T, int64_t n_labels, int C, int R) {
  if (T <= 0 || n_labels < 0 || C < 1 || R < 1 || R > OS_MAXR) return 0;
  const size_t tc = (size_t)T * (size_t)C;
  if (tc > (1u << 20)) return 0;
  return mseg_align256(tc * OS_BINS * 4) + mseg_align256(tc * R * OS_BINS * 4) + mseg_align256(tc * R * sizeof(OsSel));
}

extern "C" int mseg_cell_order_stats(const void* labels, int label_dtype, int T, int H, int W, const int64_t* label_off,
                                     int64_t n_labels, const void* img, int img_dtype, int C, int64_t frame_stride,
                                     int64_t chan_stride, int64_t row_stride, int64_t pix_stride, const int32_t* bbox, int R,
                                     const int64_t* ranks, const int64_t* bg_ranks, uint32_t* values, uint32_t* bg_values,
                                     int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!img || !bg_ranks || !bg_values || !status || !ws) return MSEG_EINVAL;
  if (!cell_stack_ok(labels, label_off, label_dtype, T, H, W, 512) || !cell_image_ok(img_dtype)) return MSEG_EINVAL;
  if (n_labels < 0 || C < 1 || R < 1 || R > OS_MAXR) return MSEG_EINVAL;
  if (n_labels > 0 && (!bbox || !ranks || !values)) return MSEG_EINVAL;
  const size_t need = mseg_cell_order_stats_workspace_bytes(T, n_labels, C, R);
  if (need == 0) return MSEG_EINVAL;
  const int64_t bpf = ((int64_t)H * W + OS_BG_SHARE - 1) / OS_BG_SHARE;
  if ((int64_t)T * C * bpf > 0x7FFFFFFFll || n_labels > 0x7FFFFFFFll) return MSEG_EINVAL;
  if (ws_bytes < need) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, need, st) != hipSuccess) return MSEG_ELAUNCH;
  if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return MSEG_ELAUNCH;
  const OsWs w = os_carve(ws, T, C, R);
  cell_dispatch(label_dtype, img_dtype, [&](auto l, auto p) {
    os_launch<decltype(l), decltype(p)>(st, labels, T, H, W, label_off, n_labels, img, C, frame_stride, chan_stride, row_stride,
                                        pix_stride, bbox, R, ranks, bg_ranks, values, bg_values, status, w);
  });
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
