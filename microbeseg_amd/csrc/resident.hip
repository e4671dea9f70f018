// resident.hip — one training batch out of a training set that lives in HBM.
// The reference (src/training/training_dataset.py:40-63, train.py:365-371) reads every crop of every epoch from its TIFF
// files inside DataLoader workers; with `TrainWorker.resident` the planes of the set (images uint16, distance labels fp32,
// boundary labels uint8) are uploaded once and a step's batch is an index list and one gather per plane.  The gather also
// does the conversion the consumer wants: the raw copy for DeviceAugment, ToTensor's normalisation for validation, the
// int64 / fp32 widening of the boundary label.  Pure bandwidth: each element is read once and written once.
#include "common.h"

namespace {

// MODE: what one source element becomes
enum { G_COPY = 0, G_NORM = 1, G_WIDEN = 2 };

template <typename S, typename D, int MODE>
__device__ __forceinline__ D gather_px(S v, float lo, float hi, float range) {
  if (MODE == G_NORM) {
    // utils.min_max_normalization: np.clip on the uint16 values, then 2 * (f32(v) - lo) / (hi - lo) - 1 in fp32, each
    // operation rounded on its own (no FMA contraction, IEEE division) — the arithmetic of raw_frame_norm (common.h)
    const float f = fminf(fmaxf((float)v, lo), hi);
    return (D)__fsub_rn(__fdiv_rn(__fmul_rn(2.f, __fsub_rn(f, lo)), range), 1.f);
  }
  return (D)v;
}

// One workgroup row (blockIdx.y, strided) per batch entry j; G source elements per lane and step.  A crop whose source
// address is a multiple of G * sizeof(S) and whose destination address is a multiple of 16 moves in vector accesses: one
// load of G * sizeof(S) bytes, G * sizeof(D) / 16 stores of 16 bytes, the HW % G last elements one by one.  Any other
// crop (odd HW puts every second crop of a 16-bit plane on an odd element) moves element by element, still coalesced.
template <typename S, typename D, int MODE, int G>
__global__ __launch_bounds__(256) void set_gather_kernel(const S* __restrict__ src, long long HW,
                                                         const int32_t* __restrict__ idx, int N, D* __restrict__ dst,
                                                         float lo, float hi, float range) {
  typedef S SV __attribute__((ext_vector_type(G)));
  typedef D DV __attribute__((ext_vector_type(16 / sizeof(D))));
  constexpr int LB = G * (int)sizeof(S);             // bytes per load
  constexpr int NS = G * (int)sizeof(D) / 16;        // 16-byte stores per load
  constexpr int PER = 16 / (int)sizeof(D);           // destination elements per store
  static_assert(NS >= 1 && NS * PER == G, "G elements fill whole 16-byte stores");
  const long long groups = HW / G;
  for (int j = blockIdx.y; j < N; j += gridDim.y) {
    const S* s = src + (long long)idx[j] * HW;        // 64-bit offsets: a plane may exceed 2^31 elements
    D* d = dst + (long long)j * HW;
    const bool wide = ((uintptr_t)s % LB) == 0 && ((uintptr_t)d % 16) == 0;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    if (wide) {
      for (long long g = t0; g < groups; g += step) {
        const SV in = *reinterpret_cast<const SV*>(s + g * G);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          DV out;
#pragma unroll
          for (int i = 0; i < PER; ++i) out[i] = gather_px<S, D, MODE>(in[k * PER + i], lo, hi, range);
          *reinterpret_cast<DV*>(d + g * G + k * PER) = out;
        }
      }
      for (long long t = groups * G + t0; t < HW; t += step) d[t] = gather_px<S, D, MODE>(s[t], lo, hi, range);
    } else {
      for (long long t = t0; t < HW; t += step) d[t] = gather_px<S, D, MODE>(s[t], lo, hi, range);
    }
  }
}

template <typename S, typename D, int MODE, int G>
int launch_gather(const void* src, long long HW, const int32_t* idx, int N, void* dst, float lo, float hi, hipStream_t st) {
  long long bx = (HW / G + 255) / 256;
  bx = bx < 1 ? 1 : (bx > 1024 ? 1024 : bx);
  const dim3 grid((unsigned)bx, (unsigned)(N < 65535 ? N : 65535));
  hipLaunchKernelGGL((set_gather_kernel<S, D, MODE, G>), grid, dim3(256), 0, st, reinterpret_cast<const S*>(src), HW, idx, N,
                     reinterpret_cast<D*>(dst), lo, hi, hi - lo);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

}  // namespace

extern "C" int mseg_set_gather(const void* src, int src_dtype, long long n, long long HW, const int32_t* idx_dev, int N,
                               void* dst, int dst_mode, float lo, float hi, void* stream) {
  const bool pair = (src_dtype == MSEG_PIX_U16 && (dst_mode == MSEG_GATHER_RAW || dst_mode == MSEG_GATHER_NORM)) ||
                    (src_dtype == MSEG_PIX_F32 && dst_mode == MSEG_GATHER_RAW) ||
                    (src_dtype == MSEG_PIX_U8 && (dst_mode == MSEG_GATHER_I64 || dst_mode == MSEG_GATHER_F32));
  if (!pair || n <= 0 || HW <= 0 || N < 0) return MSEG_EINVAL;
  if (dst_mode == MSEG_GATHER_NORM && !(hi > lo)) return MSEG_EINVAL;
  if (N == 0) return MSEG_OK;
  if (!src || !idx_dev || !dst) return MSEG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == MSEG_PIX_U16 && dst_mode == MSEG_GATHER_RAW)
    return launch_gather<uint16_t, uint16_t, G_COPY, 8>(src, HW, idx_dev, N, dst, lo, hi, st);
  if (src_dtype == MSEG_PIX_U16)
    return launch_gather<uint16_t, float, G_NORM, 8>(src, HW, idx_dev, N, dst, lo, hi, st);
  if (src_dtype == MSEG_PIX_F32)
    return launch_gather<float, float, G_COPY, 4>(src, HW, idx_dev, N, dst, lo, hi, st);
  if (dst_mode == MSEG_GATHER_I64)
    return launch_gather<uint8_t, int64_t, G_WIDEN, 2>(src, HW, idx_dev, N, dst, lo, hi, st);
  return launch_gather<uint8_t, float, G_WIDEN, 4>(src, HW, idx_dev, N, dst, lo, hi, st);
}
