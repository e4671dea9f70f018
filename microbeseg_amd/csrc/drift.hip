// drift.hip — the drift score surface of a segmented stack.  An extension: the reference has no tracking.
//
//   mseg_stack_drift   labels [T][H][W] -> scores uint32 [T - 1][2R + 1][2R + 1]: for every frame pair (t - 1, t) and every
//                      integer shift (dy, dx), |dy|, |dx| <= R, the number of pixels where the foreground of frame t - 1
//                      moved by (dy, dx) lies on the foreground of frame t
//   mseg_stack_flow    the same count per tile of frame t (64 / 128 / 256 px) and per deviation (ey, ex), |ey|, |ex| <= r <= 32,
//                      from a per-pair base shift: the score surfaces of a tile-wise displacement field
// Two kernels each: the labels are packed into one foreground bit per pixel once (dr_pack_kernel), the scores are popcounts of
// ANDed 64-bit words of those bit rows (dr_score_kernel; per tile from LDS: fl_score_kernel), 64 pixels per operation.
// Integer atomics (dr_score_kernel) or one plain store per score (fl_score_kernel): bit-identical from run to run.
#include "cell_common.h"

#define DR_BLOCK 256
#define DR_WAVES (DR_BLOCK / 64)
#define DR_MAX_R 128
// Zero words around the data words of a bit row, so that a shifted read needs no bounds test: with |dx| <= 128 the first
// word read for data word w is w + q, q = floor(-dx / 64) in -2 .. 2, and the second is w + q + 1
#define DR_PAD_L 2
#define DR_PAD_R 3
#define DR_MIN_ROWS 8             // rows of one thread at least (one atomic per thread)
#define DR_TARGET_THREADS (1 << 21)   // 256 compute units x 2048 resident lanes x 4: enough waves to hide the L1 / L2 loads
#define DR_MAX_GRID (1 << 20)
#define FL_MAX_R 32               // below 64: a tile row's window is the tile's words and ONE word on either side

namespace {

inline int dr_words(int W) { return (W + 63) / 64; }
inline int64_t dr_row_stride(int W) { return (int64_t)dr_words(W) + DR_PAD_L + DR_PAD_R; }

// A wave owns one word of a bit row: 64 consecutive pixels -> __ballot(id in 1 .. K_t); bits past the row end and the pad
// words are zero.  bits [T][H][stride]
template <typename L>
__global__ void __launch_bounds__(DR_BLOCK) dr_pack_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                           const int64_t* __restrict__ loff, u64* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const int nw = (W + 63) / 64;
  const int64_t stride = (int64_t)nw + DR_PAD_L + DR_PAD_R;
  const int64_t total = (int64_t)T * H * stride, nwaves = (int64_t)gridDim.x * DR_WAVES;
  for (int64_t i = (int64_t)blockIdx.x * DR_WAVES + (threadIdx.x >> 6); i < total; i += nwaves) {
    const int64_t row = i / stride;               // t * H + y
    const int j = (int)(i - row * stride) - DR_PAD_L;
    u64 word = 0;
    if (j >= 0 && j < nw) {                       // wave-uniform
      const int t = (int)(row / H);
      const int64_t K = loff[t + 1] - loff[t];
      const int x = j * 64 + lane;
      int id = 0;
      if (x < W) id = (int)lab[row * W + x];
      word = __ballot(cell_id(id, K) != 0);
    }
    if (lane == 0) bits[i] = word;
  }
}

// A thread owns one (pair, row chunk, dy, dx), dx fastest: the lanes of a wave hold neighbouring dx, so they load the same
// one or two words of frame t - 1 and the same word of frame t (broadcast from L1).  The word of frame t - 1 that lies
// under data word w of frame t after a move by dx is a funnel shift of the words w + q and w + q + 1, -dx = 64 q + r.
__global__ void __launch_bounds__(DR_BLOCK) dr_score_kernel(const u64* __restrict__ bits, int T, int H, int W, int R,
                                                            int rows, int chunks, uint32_t* __restrict__ scores) {
  const int S = 2 * R + 1;
  const int nw = (W + 63) / 64;
  const int64_t stride = (int64_t)nw + DR_PAD_L + DR_PAD_R;
  const int64_t total = (int64_t)(T - 1) * chunks * S * S, nthreads = (int64_t)gridDim.x * DR_BLOCK;
  for (int64_t g = (int64_t)blockIdx.x * DR_BLOCK + threadIdx.x; g < total; g += nthreads) {
    const int dxi = (int)(g % S);
    int64_t rest = g / S;
    const int dyi = (int)(rest % S);
    rest /= S;
    const int chunk = (int)(rest % chunks);
    const int pair = (int)(rest / chunks);        // frames pair, pair + 1
    const int dy = dyi - R, dx = dxi - R;
    const int s = -dx;
    const int q = s >= 0 ? s >> 6 : -((-s + 63) >> 6);
    const int r = s - q * 64;                     // 0 .. 63
    const int y0 = max(chunk * rows, max(dy, 0)), y1 = min(min((chunk + 1) * rows, H), H + min(dy, 0));
    uint32_t acc = 0;
    for (int y = y0; y < y1; ++y) {
      const u64* __restrict__ b = bits + ((int64_t)(pair + 1) * H + y) * stride + DR_PAD_L;
      const u64* __restrict__ a = bits + ((int64_t)pair * H + (y - dy)) * stride + DR_PAD_L + q;
      u64 lo = a[0];
      for (int w = 0; w < nw; ++w) {
        const u64 hi = a[w + 1];
        const u64 moved = r ? (lo >> r) | (hi << (64 - r)) : lo;
        acc += (uint32_t)__popcll(b[w] & moved);
        lo = hi;
      }
    }
    if (acc) atomicAdd(&scores[((int64_t)pair * S + dyi) * S + dxi], acc);
  }
}

// Two frames of one tile and the deviations around it.  A workgroup owns one (pair, tile) and keeps in LDS
//   cur  the tile's B rows x B / 64 words of frame t (zero rows below the frame), and
//   win  B + 2r rows x B / 64 + 2 words of frame t - 1 MOVED BY THE PAIR'S BASE SHIFT: window word (wy, k) holds the moved
//        frame's row jB - r + wy, columns iB - 64 + 64k .. + 63.  It is bounds-tested and funnel-shifted while it is filled,
//        with zeros outside the frame: the one place that sees |bx| >= 64, negative shifts and sources outside the frame.
// A thread then owns whole deviations (ey, ex), ex fastest, and walks the tile's rows as dr_score_kernel does; with |ex| <=
// 32 the moved word under tile word w starts in window word w or w + 1.  Every (tile, deviation) has one owner: a plain
// store, no atomics, no memset.
template <int NWT>                // words of a tile row
__global__ void __launch_bounds__(DR_BLOCK) fl_score_kernel(const u64* __restrict__ bits, int T, int H, int W, int r,
                                                            const int32_t* __restrict__ base, int ty, int tx,
                                                            uint32_t* __restrict__ scores) {
  extern __shared__ __align__(16) u64 fl_lds[];
  constexpr int B = 64 * NWT, NWW = NWT + 2;
  u64* cur = fl_lds;
  u64* win = fl_lds + B * NWT;
  const int S = 2 * r + 1;
  const int nw = (W + 63) / 64;
  const int64_t stride = (int64_t)nw + DR_PAD_L + DR_PAD_R;
  const int64_t total = (int64_t)(T - 1) * ty * tx;
  for (int64_t wg = blockIdx.x; wg < total; wg += gridDim.x) {      // wg = (pair * ty + j) * tx + i
    const int i = (int)(wg % tx), j = (int)(wg / tx % ty), pair = (int)(wg / tx / ty);
    const int64_t by = base[2 * (pair + 1)], bx = base[2 * (pair + 1) + 1];
    const u64* __restrict__ ft = bits + (int64_t)(pair + 1) * H * stride + DR_PAD_L;
    const u64* __restrict__ fp = bits + (int64_t)pair * H * stride + DR_PAD_L;
    for (int k = threadIdx.x; k < B * NWT; k += blockDim.x) {
      const int ry = k / NWT, iw = i * NWT + (k - ry * NWT);
      const int y = j * B + ry;
      cur[k] = (y < H && iw < nw) ? ft[(int64_t)y * stride + iw] : 0;
    }
    for (int k = threadIdx.x; k < (B + 2 * r) * NWW; k += blockDim.x) {
      const int wy = k / NWW, kw = k - wy * NWW;
      const int64_t ys = (int64_t)j * B - r + wy - by;              // the source row and the source column of bit 0
      const int64_t p = (int64_t)i * B - 64 + 64 * kw - bx;
      const int64_t q = p >> 6;                                     // floor
      const int s = (int)(p & 63);
      u64 v = 0;
      if (ys >= 0 && ys < H) {
        const u64* __restrict__ row = fp + ys * stride;
        const u64 lo = (q >= 0 && q < nw) ? row[q] : 0;
        const u64 hi = (q + 1 >= 0 && q + 1 < nw) ? row[q + 1] : 0;
        v = s ? (lo >> s) | (hi << (64 - s)) : lo;
      }
      win[k] = v;
    }
    __syncthreads();
    const int rows = min(B, H - j * B);                             // the rows below are zero in cur
    for (int e = threadIdx.x; e < S * S; e += blockDim.x) {
      const int eyi = e / S, exi = e - eyi * S;
      const int off = 64 - (exi - r);                               // 32 .. 96: window bit under bit 0 of tile word 0
      const int s = off & 63;
      const u64* a = win + (2 * r - eyi) * NWW + (off >> 6);        // tile row ry lies under window row ry - ey + r
      uint32_t acc = 0;
      for (int ry = 0; ry < rows; ++ry) {
        u64 lo = a[ry * NWW];
#pragma unroll
        for (int w = 0; w < NWT; ++w) {
          const u64 hi = a[ry * NWW + w + 1];
          const u64 moved = s ? (lo >> s) | (hi << (64 - s)) : lo;
          acc += (uint32_t)__popcll(cur[ry * NWT + w] & moved);
          lo = hi;
        }
      }
      scores[(wg * S + eyi) * S + exi] = acc;
    }
    __syncthreads();
  }
}

// labels -> bits [T][H][stride] on the stream
void dr_pack(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, u64* bits, hipStream_t st) {
  const int64_t words = (int64_t)T * H * dr_row_stride(W);
  int64_t grid = (words + DR_WAVES - 1) / DR_WAVES;
  if (grid > DR_MAX_GRID) grid = DR_MAX_GRID;
  cell_dispatch(dtype, [&](auto l) {
    typedef decltype(l) L;
    hipLaunchKernelGGL(dr_pack_kernel<L>, dim3((unsigned)grid), dim3(DR_BLOCK), 0, st, (const L*)labels, T, H, W, label_off,
                       bits);
  });
}

}  // namespace

extern "C" size_t mseg_stack_drift_workspace_bytes(int T, int H, int W) {
  if (T <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31) - 512) return 0;
  return mseg_align256((size_t)T * (size_t)H * (size_t)dr_row_stride(W) * sizeof(u64));
}

extern "C" int mseg_stack_drift(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int max_drift,
                                uint32_t* scores, void* ws, size_t ws_bytes, void* stream) {
  if (!cell_stack_ok(labels, label_off, dtype, T, H, W, 512) || !ws) return MSEG_EINVAL;
  if (max_drift < 0 || max_drift > DR_MAX_R) return MSEG_EINVAL;
  if (T > 1 && !scores) return MSEG_EINVAL;
  if (ws_bytes < mseg_stack_drift_workspace_bytes(T, H, W)) return MSEG_EWORKSPACE;
  if (T == 1) return MSEG_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = 2 * max_drift + 1;
  const int64_t cells = (int64_t)(T - 1) * S * S;
  if (hipMemsetAsync(scores, 0, sizeof(uint32_t) * (size_t)cells, st) != hipSuccess) return MSEG_ELAUNCH;
  u64* bits = (u64*)ws;
  dr_pack(labels, dtype, T, H, W, label_off, bits, st);
  // row chunks: as many as it takes to reach DR_TARGET_THREADS threads, of at least DR_MIN_ROWS rows each
  int64_t chunks = (DR_TARGET_THREADS + cells - 1) / cells;
  const int64_t most = ((int64_t)H + DR_MIN_ROWS - 1) / DR_MIN_ROWS;
  if (chunks > most) chunks = most;
  if (chunks < 1) chunks = 1;
  const int rows = (int)(((int64_t)H + chunks - 1) / chunks);
  chunks = ((int64_t)H + rows - 1) / rows;
  int64_t grid = (cells * chunks + DR_BLOCK - 1) / DR_BLOCK;
  if (grid > DR_MAX_GRID) grid = DR_MAX_GRID;
  hipLaunchKernelGGL(dr_score_kernel, dim3((unsigned)grid), dim3(DR_BLOCK), 0, st, (const u64*)bits, T, H, W, max_drift, rows,
                     (int)chunks, scores);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

extern "C" size_t mseg_stack_flow_workspace_bytes(int T, int H, int W) { return mseg_stack_drift_workspace_bytes(T, H, W); }

extern "C" int mseg_stack_flow(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int tile,
                               int radius, const int32_t* base, uint32_t* scores, void* ws, size_t ws_bytes, void* stream) {
  if (!cell_stack_ok(labels, label_off, dtype, T, H, W, 512) || !base || !ws) return MSEG_EINVAL;
  if (tile != 64 && tile != 128 && tile != 256) return MSEG_EINVAL;
  if (radius < 0 || radius > FL_MAX_R) return MSEG_EINVAL;
  if (T > 1 && !scores) return MSEG_EINVAL;
  if (ws_bytes < mseg_stack_flow_workspace_bytes(T, H, W)) return MSEG_EWORKSPACE;
  if (T == 1) return MSEG_OK;
  hipStream_t st = (hipStream_t)stream;
  u64* bits = (u64*)ws;
  dr_pack(labels, dtype, T, H, W, label_off, bits, st);
  const int ty = (H + tile - 1) / tile, tx = (W + tile - 1) / tile, nwt = tile / 64;
  const int S2 = (2 * radius + 1) * (2 * radius + 1);
  // a thread owns whole deviations: the largest workgroup whose lanes' turns are at least 90 % used (r = 8: 289 deviations
  // are 5 turns of 64 lanes, but 2 of 256 with the second nearly empty), else one wave
  int block = 64;
  for (int b = DR_BLOCK; b > 64; b /= 2)
    if (10 * S2 >= 9 * ((S2 + b - 1) / b * b)) { block = b; break; }
  int64_t grid = (int64_t)(T - 1) * ty * tx;
  if (grid > DR_MAX_GRID) grid = DR_MAX_GRID;
  const size_t lds = sizeof(u64) * ((size_t)tile * nwt + (size_t)(tile + 2 * radius) * (nwt + 2));
#define FL_GO(N)                                                                                                          \
  hipLaunchKernelGGL(fl_score_kernel<N>, dim3((unsigned)grid), dim3(block), lds, st, (const u64*)bits, T, H, W, radius, base, \
                     ty, tx, scores)
  if (nwt == 1) FL_GO(1);
  else if (nwt == 2) FL_GO(2);
  else FL_GO(4);
#undef FL_GO
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
