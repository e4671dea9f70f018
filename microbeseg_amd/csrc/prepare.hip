// prepare.hip — training-set preparation on the device: frame statistics, crop extraction with the three
// normalisations of the reference, the per-crop cell census of the import and the crop overlay.
// Reference: DataCropWorker.next_crop (src/utils/data_cropping.py:157-264), DataImportWorker.import_data
// (src/utils/data_import.py:125-194), DataExportWorker.export_data (src/utils/data_export.py:100-101).
#include "common.h"

__device__ __forceinline__ unsigned pix_load(const void* __restrict__ p, int dtype, size_t i) {
  return dtype == MSEG_PIX_U8 ? reinterpret_cast<const uint8_t*>(p)[i] : reinterpret_cast<const uint16_t*>(p)[i];
}

// ---- mseg_frame_stats: {min, max, sum v, sum v^2} of one frame, exact ---------------------------------------------------
// np.mean / np.std (data_cropping.py:172) are fp64 pairwise sums; integer sums are exact and independent of the order the
// blocks finish in, and a double accumulator would already be wrong at sum v^2 > 2^53 (a 2048^2 frame of 65535s).
// A thread sees at most 2^31 / 256 values below 2^32 each: its 64-bit sums cannot overflow before the grid's do.
__global__ __launch_bounds__(256) void frame_stats_kernel(const void* __restrict__ raw, int dtype, size_t n,
                                                          unsigned long long* __restrict__ out) {
  unsigned lo = 0xffffffffu, hi = 0u;
  unsigned long long s = 0ull, q = 0ull;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned v = pix_load(raw, dtype, i);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
    s += v;
    q += (unsigned long long)v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  __shared__ unsigned sh_lo[4], sh_hi[4];
  __shared__ unsigned long long sh_s[4], sh_q[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh_lo[wave] = lo; sh_hi[wave] = hi; sh_s[wave] = s; sh_q[wave] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      lo = sh_lo[w] < lo ? sh_lo[w] : lo;
      hi = sh_hi[w] > hi ? sh_hi[w] : hi;
      s += sh_s[w];
      q += sh_q[w];
    }
    if (lo <= hi) {                      // a block without pixels (never launched: blocks <= ceil(n / 256)) adds nothing
      atomicMin(out, (unsigned long long)lo);
      atomicMax(out + 1, (unsigned long long)hi);
      atomicAdd(out + 2, s);
      atomicAdd(out + 3, q);
    }
  }
}

extern "C" int mseg_frame_stats(const void* raw, int dtype, size_t npix, uint64_t* out, void* stream) {
  if (!raw || !out || npix == 0 || npix >= ((size_t)1 << 31) || (dtype != MSEG_PIX_U8 && dtype != MSEG_PIX_U16))
    return MSEG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0xff, sizeof(uint64_t), st) != hipSuccess) return MSEG_ELAUNCH;          // min starts at 2^64 - 1
  if (hipMemsetAsync(out + 1, 0, 3 * sizeof(uint64_t), st) != hipSuccess) return MSEG_ELAUNCH;
  size_t blocks = (npix + 256 * 16 - 1) / (256 * 16);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(frame_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, raw, dtype, npix,
                     reinterpret_cast<unsigned long long*>(out));
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

// ---- mseg_crops_extract --------------------------------------------------------------------------------------------------
// blockIdx.y = crop, one pixel per thread.  numpy evaluates `c * (crop.astype(np.float32) - min) / (max - min)` on a float32
// array with integer scalars: subtract, multiply, divide, each rounded to fp32 — the explicit _rn operations below (no
// contraction into a fused multiply-add, no reciprocal).  65535 * 65535 is not a float32 number: multiplying before
// dividing, as the reference does, keeps its rounding.
__global__ __launch_bounds__(256) void crops_extract_kernel(const void* __restrict__ raw, int dtype, int H, int W,
                                                            const int32_t* __restrict__ origin_yx, int S, unsigned pad_value,
                                                            float fmin, float frange, void* __restrict__ crops_raw,
                                                            uint8_t* __restrict__ crops_show,
                                                            uint16_t* __restrict__ crops_u16, float* __restrict__ x) {
  const size_t n = (size_t)S * S;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int k = blockIdx.y;
  const int r = (int)(p / S), c = (int)(p - (size_t)r * S);
  const long long yy = (long long)origin_yx[2 * k] + r, xx = (long long)origin_yx[2 * k + 1] + c;
  unsigned v = pad_value;
  if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = pix_load(raw, dtype, (size_t)yy * W + (size_t)xx);
  const size_t o = (size_t)k * n + p;
  if (crops_raw) {
    if (dtype == MSEG_PIX_U8) reinterpret_cast<uint8_t*>(crops_raw)[o] = (uint8_t)v;
    else reinterpret_cast<uint16_t*>(crops_raw)[o] = (uint16_t)v;
  }
  const float d = __fsub_rn((float)v, fmin);
  if (crops_show) crops_show[o] = (uint8_t)(int)__fdiv_rn(__fmul_rn(255.f, d), frange);
  if (crops_u16) {
    float t = __fdiv_rn(__fmul_rn(65535.f, d), frange);
    t = t < 0.f ? 0.f : (t > 65535.f ? 65535.f : t);
    crops_u16[o] = (uint16_t)(int)t;
  }
  if (x) x[o] = raw_frame_norm(v, fmin, frange);
}

extern "C" int mseg_crops_extract(const void* raw, int dtype, int H, int W, int K, const int32_t* origin_yx, int S,
                                  int pad_value, int lo, int hi, void* crops_raw, uint8_t* crops_show, uint16_t* crops_u16,
                                  float* x, void* stream) {
  const int vmax = dtype == MSEG_PIX_U8 ? 255 : 65535;
  if (!raw || !origin_yx || (dtype != MSEG_PIX_U8 && dtype != MSEG_PIX_U16) || H <= 0 || W <= 0 || K <= 0 || K > 65535 ||
      S <= 0 || S > 16384 || pad_value < 0 || pad_value > vmax || lo < 0 || hi > 65535 || hi <= lo)
    return MSEG_EINVAL;
  const size_t n = (size_t)S * S;
  hipLaunchKernelGGL(crops_extract_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)K), dim3(256), 0, (hipStream_t)stream,
                     raw, dtype, H, W, origin_yx, S, (unsigned)pad_value, (float)lo, (float)(hi - lo), crops_raw, crops_show,
                     crops_u16, x);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

// ---- mseg_crop_census ----------------------------------------------------------------------------------------------------
// One workgroup per crop.  Ids run up to 65535: a presence bitmap of 64 Kbit (8 KiB of LDS) replaces np.unique; the crop's
// bitmap is then OR-ed into the region's bitmap in the workspace (only its non-zero words), and a second, one-workgroup
// kernel counts that one.  Integer atomics only: the result does not depend on the order of the workgroups.
#define CENSUS_WORDS 2048
__global__ __launch_bounds__(256) void crop_census_kernel(const void* __restrict__ mask, int dtype, int W, int y0, int x0,
                                                          int nx, int S, int ncrops, int32_t* __restrict__ cells,
                                                          unsigned long long* __restrict__ area,
                                                          uint32_t* __restrict__ region_bits) {
  __shared__ uint32_t bits[CENSUS_WORDS];
  __shared__ unsigned sh_cnt[4];
  __shared__ unsigned long long sh_area[4];
  const int crop = blockIdx.x;
  const int cy = crop / nx, cx = crop - cy * nx;
  for (int w = threadIdx.x; w < CENSUS_WORDS; w += 256) bits[w] = 0u;
  __syncthreads();
  const size_t n = (size_t)S * S;
  const size_t base = (size_t)(y0 + (size_t)cy * S) * W + x0 + (size_t)cx * S;
  unsigned long long a = 0ull;
  for (size_t p = threadIdx.x; p < n; p += 256) {
    const int r = (int)(p / S), c = (int)(p - (size_t)r * S);
    const unsigned v = pix_load(mask, dtype, base + (size_t)r * W + c);
    if (v) {
      ++a;
      const uint32_t bit = 1u << (v & 31u);
      if (!(reinterpret_cast<volatile uint32_t*>(bits)[v >> 5] & bit)) atomicOr(&bits[v >> 5], bit);
    }
  }
  __syncthreads();
  unsigned cnt = 0u;
  for (int w = threadIdx.x; w < CENSUS_WORDS; w += 256) {
    const uint32_t b = bits[w];
    if (b) {
      cnt += __popc(b);
      atomicOr(&region_bits[w], b);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    a += __shfl_xor(a, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh_cnt[wave] = cnt; sh_area[wave] = a; }
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
    a = sh_area[0] + sh_area[1] + sh_area[2] + sh_area[3];
    cells[crop] = (int32_t)cnt;
    area[crop] = a;
    atomicAdd(&area[ncrops], a);
  }
}

__global__ __launch_bounds__(256) void crop_census_region_kernel(const uint32_t* __restrict__ region_bits,
                                                                 int32_t* __restrict__ cells_region) {
  __shared__ unsigned sh_cnt[4];
  unsigned cnt = 0u;
  for (int w = threadIdx.x; w < CENSUS_WORDS; w += 256) cnt += __popc(region_bits[w]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) sh_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) *cells_region = (int32_t)(sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3]);
}

extern "C" size_t mseg_crop_census_workspace_bytes(void) { return CENSUS_WORDS * sizeof(uint32_t); }

extern "C" int mseg_crop_census(const void* mask, int dtype, int H, int W, int y0, int x0, int ny, int nx, int S,
                                int32_t* cells, int64_t* area, void* ws, size_t ws_bytes, void* stream) {
  if (!mask || !cells || !area || !ws || ws_bytes < mseg_crop_census_workspace_bytes() ||
      (dtype != MSEG_PIX_U8 && dtype != MSEG_PIX_U16) || H <= 0 || W <= 0 || S <= 0 || S > 16384 || ny <= 0 || nx <= 0 ||
      y0 < 0 || x0 < 0 || (long long)y0 + (long long)ny * S > H || (long long)x0 + (long long)nx * S > W ||
      (long long)ny * nx > (1 << 24))
    return MSEG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int ncrops = ny * nx;
  if (hipMemsetAsync(ws, 0, mseg_crop_census_workspace_bytes(), st) != hipSuccess) return MSEG_ELAUNCH;
  if (hipMemsetAsync(area + ncrops, 0, sizeof(int64_t), st) != hipSuccess) return MSEG_ELAUNCH;
  hipLaunchKernelGGL(crop_census_kernel, dim3((unsigned)ncrops), dim3(256), 0, st, mask, dtype, W, y0, x0, nx, S, ncrops,
                     cells, reinterpret_cast<unsigned long long*>(area), reinterpret_cast<uint32_t*>(ws));
  MSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(crop_census_region_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(ws),
                     cells + ncrops);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

// ---- mseg_crops_overlay: grey crop x 3 with yellow outlines (data_cropping.py:214-215,238-240) --------------------------
__global__ __launch_bounds__(256) void crops_overlay_kernel(const uint8_t* __restrict__ show,
                                                            const uint8_t* __restrict__ outlines, uint8_t* __restrict__ rgb,
                                                            size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t g = show[i];
  const bool o = outlines[i] != 0;
  rgb[3 * i] = o ? 255 : g;
  rgb[3 * i + 1] = o ? 255 : g;
  rgb[3 * i + 2] = o ? 0 : g;
}

extern "C" int mseg_crops_overlay(const uint8_t* show, const uint8_t* outlines, uint8_t* rgb, int K, int S, void* stream) {
  if (!show || !outlines || !rgb || K <= 0 || S <= 0 || S > 16384) return MSEG_EINVAL;
  const size_t n = (size_t)K * S * S;
  if ((n + 255) / 256 > 0x7fffffffull) return MSEG_EINVAL;
  hipLaunchKernelGGL(crops_overlay_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, show,
                     outlines, rgb, n);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
