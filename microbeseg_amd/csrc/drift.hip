// drift.hip — the drift score surface of a segmented stack.  An extension: the reference has no tracking.
//
//   mseg_stack_drift   labels [T][H][W] -> scores uint32 [T - 1][2R + 1][2R + 1]: for every frame pair (t - 1, t) and every
//                      integer shift (dy, dx), |dy|, |dx| <= R, the number of pixels where the foreground of frame t - 1
//                      moved by (dy, dx) lies on the foreground of frame t
// Two kernels: the labels are packed into one foreground bit per pixel once (dr_pack_kernel), the scores are popcounts of
// ANDed 64-bit words of those bit rows (dr_score_kernel), 64 pixels per operation.  Integer atomics only: bit-identical
// from run to run.
#include "common.h"

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

namespace {

typedef unsigned long long u64;

inline size_t dr_align(size_t v) { return (v + 255) / 256 * 256; }
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
      int64_t id = 0;
      if (x < W) id = (int64_t)lab[row * W + x];
      word = __ballot(id > 0 && id <= K);
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

}  // namespace

extern "C" size_t mseg_stack_drift_workspace_bytes(int T, int H, int W) {
  if (T <= 0 || H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31) - 512) return 0;
  return dr_align((size_t)T * (size_t)H * (size_t)dr_row_stride(W) * sizeof(u64));
}

extern "C" int mseg_stack_drift(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off, int max_drift,
                                uint32_t* scores, void* ws, size_t ws_bytes, void* stream) {
  if (!labels || !label_off || !ws || T <= 0 || H <= 0 || W <= 0) return MSEG_EINVAL;
  if ((int64_t)H * W >= (1ll << 31) - 512) return MSEG_EINVAL;
  if (dtype != MSEG_PIX_U16 && dtype != MSEG_PIX_I32) return MSEG_EINVAL;
  if (max_drift < 0 || max_drift > DR_MAX_R) return MSEG_EINVAL;
  if (T > 1 && !scores) return MSEG_EINVAL;
  if (ws_bytes < mseg_stack_drift_workspace_bytes(T, H, W)) return MSEG_EWORKSPACE;
  if (T == 1) return MSEG_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = 2 * max_drift + 1;
  const int64_t cells = (int64_t)(T - 1) * S * S;
  if (hipMemsetAsync(scores, 0, sizeof(uint32_t) * (size_t)cells, st) != hipSuccess) return MSEG_ELAUNCH;
  u64* bits = (u64*)ws;
  const int64_t words = (int64_t)T * H * dr_row_stride(W);
  int64_t grid = (words + DR_WAVES - 1) / DR_WAVES;
  if (grid > DR_MAX_GRID) grid = DR_MAX_GRID;
  if (dtype == MSEG_PIX_U16)
    hipLaunchKernelGGL(dr_pack_kernel<uint16_t>, dim3((unsigned)grid), dim3(DR_BLOCK), 0, st, (const uint16_t*)labels, T, H,
                       W, label_off, bits);
  else
    hipLaunchKernelGGL(dr_pack_kernel<int32_t>, dim3((unsigned)grid), dim3(DR_BLOCK), 0, st, (const int32_t*)labels, T, H, W,
                       label_off, bits);
  // row chunks: as many as it takes to reach DR_TARGET_THREADS threads, of at least DR_MIN_ROWS rows each
  int64_t chunks = (DR_TARGET_THREADS + cells - 1) / cells;
  const int64_t most = ((int64_t)H + DR_MIN_ROWS - 1) / DR_MIN_ROWS;
  if (chunks > most) chunks = most;
  if (chunks < 1) chunks = 1;
  const int rows = (int)(((int64_t)H + chunks - 1) / chunks);
  chunks = ((int64_t)H + rows - 1) / rows;
  grid = (cells * chunks + DR_BLOCK - 1) / DR_BLOCK;
  if (grid > DR_MAX_GRID) grid = DR_MAX_GRID;
  hipLaunchKernelGGL(dr_score_kernel, dim3((unsigned)grid), dim3(DR_BLOCK), 0, st, (const u64*)bits, T, H, W, max_drift, rows,
                     (int)chunks, scores);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
