// profile.hip — per-cell intensity profile along a given integer direction: the cell's pixels are projected on the direction,
// the projected extent is cut into N bins from pole to pole, and every bin gets its pixel count and the sum of every
// channel's values.  An extension of the per-cell table (cells.hip, §6l).
//   pf_cell_kernel   one wave (one workgroup of 64) per cell slot, two walks over the cell's box (cell_walk, cell_common.h):
//                    the extreme projections by a wave reduction, then the bins in LDS; plain stores of the whole slot,
//                    no global atomics, no workspace
// Integers only, order-free integer adds: identical bytes from run to run.
#include "cell_common.h"

#define PF_MAXN 32                // most bins
#define PF_MAXC 8                 // most channels of one call

namespace {

// floor(num / D) for D >= 1 and num < 33 D < 2^63, exact: the fp32 quotient is within 2^-16 of the true one (two roundings to
// 24 bits, the reciprocal, the product, on a quotient below 33), so its integer part is the floor or one beside it, and the
// remainder in 64-bit integers says which.  Outside that range (a dir no orientation gives) the result is some int in 0 .. 33.
__device__ __forceinline__ int pf_quotient(u64 num, u64 D, float rcpD) {
  int b = (int)fminf((float)num * rcpD, (float)PF_MAXN);                    // fminf: a NaN or an infinity becomes 32
  const int64_t r = (int64_t)(num - (u64)b * D);
  if (r < 0) --b;
  else if ((u64)r >= D) ++b;
  return b;
}

template <typename L, typename P>
__global__ void __launch_bounds__(CELL_WAVE) pf_cell_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                            const int64_t* __restrict__ loff, int64_t n,
                                                            const P* __restrict__ img, int C, int64_t fs, int64_t cs, int64_t rs,
                                                            int64_t ps, const int32_t* __restrict__ bbox,
                                                            const int32_t* __restrict__ dir, int N, uint32_t* __restrict__ count,
                                                            u64* __restrict__ sums, int64_t* __restrict__ extent) {
  __shared__ uint32_t cnt[PF_MAXN];
  __shared__ u64 acc[PF_MAXC * PF_MAXN];
  const int lane = threadIdx.x;
  const int64_t s = blockIdx.x;
  if (s >= n) return;
  const int4 bb = make_int4(bbox[4 * s], bbox[4 * s + 1], bbox[4 * s + 2], bbox[4 * s + 3]);      // r0, c0, r1, c1
  const int64_t uy = dir[2 * s], ux = dir[2 * s + 1];
  const int t = cell_slot_frame(loff, T, s);
  // an absent cell (an all-zero box) has no elements: both walks are empty and zeros are stored
  const CellWalk box = cell_walk_box(bb, H, W, s - loff[t] + 1);
  const L* frame = lab + (int64_t)t * H * W;
  const P* planes = img + (int64_t)t * fs;

  // first walk: the extreme projections.  |uy y + ux x| < 2^63 for every int32 uy, ux and y, x < 2^31
  int64_t qmin = 0x7FFFFFFFFFFFFFFFll, qmax = -0x7FFFFFFFFFFFFFFFll - 1;
  cell_walk(frame, W, box, lane, [&](int y, int x) {
    const int64_t q = uy * y + ux * x;
    qmin = min(qmin, q); qmax = max(qmax, q);
  });
#pragma unroll
  for (int d = 1; d < CELL_WAVE; d <<= 1) {
    qmin = min(qmin, (int64_t)__shfl_xor((long long)qmin, d, CELL_WAVE));
    qmax = max(qmax, (int64_t)__shfl_xor((long long)qmax, d, CELL_WAVE));
  }
  if (qmax < qmin) qmin = qmax = 0;                                          // no pixel of the cell inside the box
  // unsigned from here: a dir beyond what an orientation gives may wrap, it cannot leave the arrays (the clamp below)
  const u64 D = (u64)qmax - (u64)qmin + 1;
  const float rcpD = 1.0f / (float)D;

  if (lane < PF_MAXN) cnt[lane] = 0;
  for (int e = lane; e < C * PF_MAXN; e += CELL_WAVE) acc[e] = 0;
  __syncthreads();
  // second walk: the bin of every pixel
  cell_walk(frame, W, box, lane, [&](int y, int x) {
    const u64 num = ((u64)(uy * y + ux * x) - (u64)qmin) * (u64)N;
    const int b = min(max(pf_quotient(num, D, rcpD), 0), N - 1);
    atomicAdd(&cnt[b], 1u);
    const P* p = planes + (int64_t)y * rs + (int64_t)x * ps;
    for (int c = 0; c < C; ++c) atomicAdd(&acc[c * PF_MAXN + b], (u64)p[(int64_t)c * cs]);
  });
  __syncthreads();
  if (lane < N) count[(int64_t)lane * n + s] = cnt[lane];
  for (int e = lane; e < C * N; e += CELL_WAVE) {
    const int c = e / N, b = e - c * N;
    sums[((int64_t)c * N + b) * n + s] = acc[c * PF_MAXN + b];
  }
  if (lane == 0) { extent[s] = qmin; extent[n + s] = qmax; }
}

}  // namespace

// ---- entry point ----------------------------------------------------------------------------------------------------------
extern "C" int mseg_cell_profile(const void* labels, int label_dtype, int T, int H, int W, const int64_t* label_off,
                                 int64_t n_labels, const void* img, int img_dtype, int C, int64_t frame_stride,
                                 int64_t chan_stride, int64_t row_stride, int64_t pix_stride, const int32_t* bbox,
                                 const int32_t* dir, int N, uint32_t* count, uint64_t* sums, int64_t* extent, void* stream) {
  if (!img) return MSEG_EINVAL;
  if (!cell_stack_ok(labels, label_off, label_dtype, T, H, W, 512) || !cell_image_ok(img_dtype)) return MSEG_EINVAL;
  if (n_labels < 0 || n_labels > 0x7FFFFFFFll || C < 1 || C > PF_MAXC || N < 2 || N > PF_MAXN) return MSEG_EINVAL;
  if (n_labels > 0 && (!bbox || !dir || !count || !sums || !extent)) return MSEG_EINVAL;
  if (n_labels == 0) return MSEG_OK;
  hipStream_t st = (hipStream_t)stream;
  cell_dispatch(label_dtype, img_dtype, [&](auto l, auto p) {
    typedef decltype(l) L;
    typedef decltype(p) P;
    hipLaunchKernelGGL((pf_cell_kernel<L, P>), dim3((unsigned)n_labels), dim3(CELL_WAVE), 0, st, (const L*)labels, T, H, W,
                       label_off, n_labels, (const P*)img, C, frame_stride, chan_stride, row_stride, pix_stride, bbox, dir, N,
                       count, (u64*)sums, extent);
  });
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
