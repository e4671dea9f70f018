// clahe.hip — contrast-limited adaptive histogram equalisation exactly as scikit-image 0.18.3 computes
//   (65535 * skimage.exposure.equalize_adapthist(img, clip_limit=0.01)).astype(np.uint16)
// for a batch of N single-channel images of one shape.  Reference call sites: the CLAHE branch of Contrast
// (src/training/mytransforms.py:92-95) and ContrastEnhancement (src/inference/inference_dataset.py:63-77).
//
// The library routine is integer arithmetic plus a few IEEE fp64 / fp32 operations in a fixed order, so the result is
// reproduced bit for bit (tests/golden/clahe_library.npz).  The steps, with the library's own quirks kept:
//   1  img_as_uint: uint16 as is, uint8 * 257
//   2  stretch to 2^14 levels: g = rint(((v - lo) / (hi - lo)) * 16383) in fp64 (lo != hi), else min(v, 16383)
//   3  reflect padding (edge not repeated) by k/2 in front and up to the next tile multiple + ceil(k/2) behind,
//      k = (H / 8, W / 8); indexed, never materialised
//   4  bin = g / 65 (65 = 1 + 16384 / 256 levels per bin: bins 0..252 of 256 are used)
//   5  one histogram per tile of the grid ceil(H / ky) x ceil(W / kx); tile (i, j) = rows i ky .. (i + 1) ky - 1, reflected
//   6  clipping at clim = int(max(0.01 ky kx, 1)) with the library's two-pass redistribution and its leftover loop
//   7  map = int(min(cumsum(h) * (16383 / (ky kx)), 16383)) in fp64
//   8  blend of the four surrounding tile maps (map grid edge-replicated by one tile; blocks of k from the padded origin):
//      sum over (e0, e1) in fp32 of float(double(map) * (wx * wy)), truncated to uint16
//   9  f = u * (1 / 65535); f = (f - min) / (max - min) (or clip(f, 0, 1) for a constant image); out = uint16(65535 f)
// Launches for the whole batch: input min / max, tile maps, blend (+ min / max of u), output rescale.  The two whole-image
// reductions are two-level without atomics: every block of the producing pass leaves its {min, max}, the next pass folds
// an image's partials (same-address atomics from thousands of short blocks serialise in L2: measured 50-90 us per pass).
#include "common.h"

// every fp operation below is the separately rounded IEEE operation the library performs: no fused multiply-add
#pragma clang fp contract(off)

#define CL_BLOCK 256
#define CL_BINS 256
#define CL_GRAY 16384
#define CL_BINSIZE 65
#define CL_MAX_BLOCKS_X 1024      // blocks of a streaming pass per image = {min, max} partials per image

struct ClaheGeom {
  int H, W, ky, kx, ny, nx;   // image, tile, tile grid
};

__device__ __forceinline__ unsigned cl_load(const void* __restrict__ in, int dtype, size_t i) {
  if (dtype == MSEG_PIX_U16) return reinterpret_cast<const uint16_t*>(in)[i];
  if (dtype == MSEG_PIX_U8) return 257u * reinterpret_cast<const uint8_t*>(in)[i];
  const float f = reinterpret_cast<const float*>(in)[i];
  return (unsigned)fminf(fmaxf(f, 0.f), 65535.f);      // integer-valued by contract; NaN -> 0
}

// step 2 for one pixel; mm = {lo, hi} of the image
__device__ __forceinline__ int cl_stretch(unsigned v, unsigned lo, unsigned hi) {
  if (lo == hi) return (int)(v < CL_GRAY - 1 ? v : CL_GRAY - 1);
  const double t = ((double)v - (double)lo) / ((double)hi - (double)lo);
  const int g = (int)rint(t * (double)(CL_GRAY - 1));    // rint: round half to even, like np.round
  return g < 0 ? 0 : (g > CL_GRAY - 1 ? CL_GRAY - 1 : g);
}

__device__ __forceinline__ int cl_reflect(int i, int n) { return i >= n ? 2 * (n - 1) - i : i; }

__device__ __forceinline__ unsigned cl_wave_min(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
  return v;
}
__device__ __forceinline__ unsigned cl_wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  return v;
}

// block-wide min / max, returned to every thread
__device__ __forceinline__ void cl_block_minmax(unsigned& lo, unsigned& hi) {
  __shared__ unsigned s_lo[CL_BLOCK / 64], s_hi[CL_BLOCK / 64];
  lo = cl_wave_min(lo);
  hi = cl_wave_max(hi);
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < CL_BLOCK / 64; ++w) { lo = s_lo[w] < lo ? s_lo[w] : lo; hi = s_hi[w] > hi ? s_hi[w] : hi; }
  __syncthreads();
}

// fold the nb per-block partials {min, max} of one image
__device__ __forceinline__ void cl_fold_partials(const unsigned* __restrict__ part, int nb, unsigned& lo, unsigned& hi) {
  lo = 0xffffffffu; hi = 0u;
  for (int i = threadIdx.x; i < nb; i += CL_BLOCK) {
    const unsigned a = part[2 * i], b = part[2 * i + 1];
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  cl_block_minmax(lo, hi);
}

// pin[s][block] = {min, max} of the block's share of image s
__global__ __launch_bounds__(CL_BLOCK) void clahe_minmax_kernel(const void* __restrict__ in, int dtype, int hw,
                                                                const int32_t* __restrict__ apply,
                                                                unsigned* __restrict__ pin) {
  const int s = blockIdx.y;
  if (apply && !apply[s]) return;
  const size_t base = (size_t)s * hw;
  unsigned lo = 0xffffffffu, hi = 0u;
  for (int i = blockIdx.x * CL_BLOCK + threadIdx.x; i < hw; i += gridDim.x * CL_BLOCK) {
    const unsigned v = cl_load(in, dtype, base + i);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  cl_block_minmax(lo, hi);
  if (threadIdx.x == 0) {
    unsigned* p = pin + 2 * ((size_t)s * gridDim.x + blockIdx.x);
    p[0] = lo; p[1] = hi;
  }
}

__device__ __forceinline__ int cl_block_sum(int v, int* sm /*[CL_BLOCK / 64]*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int w = 0; w < CL_BLOCK / 64; ++w) r += sm[w];
  __syncthreads();
  return r;
}

// steps 3-7: one workgroup per tile and image, thread b owns bin b.  The histogram is counted in one LDS copy per wave
// (a flat background sends a whole wave to one bin); the leftover loop is sequential over `index` as in the library, each
// of its steps cooperative: two block-wide counts.
__global__ __launch_bounds__(CL_BLOCK) void clahe_maps_kernel(const void* __restrict__ in, int dtype, ClaheGeom q, int clim,
                                                              const int32_t* __restrict__ apply,
                                                              const unsigned* __restrict__ pin, int nb,
                                                              unsigned* __restrict__ mm /*[N][2]: the image's {min, max}*/,
                                                              uint16_t* __restrict__ maps /*[N][ny*nx][256]*/) {
  __shared__ unsigned hist[CL_BLOCK / 64][CL_BINS];
  __shared__ int scan[CL_BINS];
  __shared__ int part[CL_BLOCK / 64];
  const int s = blockIdx.y, tile = blockIdx.x, b = threadIdx.x;
  if (apply && !apply[s]) return;
  const int ti = tile / q.nx, tj = tile - ti * q.nx;
  unsigned lo, hi;
  cl_fold_partials(pin + 2 * (size_t)s * nb, nb, lo, hi);
  if (tile == 0 && b == 0) { mm[2 * s] = lo; mm[2 * s + 1] = hi; }      // for the blend pass
#pragma unroll
  for (int w = 0; w < CL_BLOCK / 64; ++w) hist[w][b] = 0u;
  __syncthreads();
  const size_t base = (size_t)s * q.H * q.W;
  const int npx = q.ky * q.kx;
  unsigned* myhist = hist[b >> 6];
  for (int i = b; i < npx; i += CL_BLOCK) {
    const int r = i / q.kx, c = i - r * q.kx;
    const int y = cl_reflect(ti * q.ky + r, q.H), x = cl_reflect(tj * q.kx + c, q.W);
    const int g = cl_stretch(cl_load(in, dtype, base + (size_t)y * q.W + x), lo, hi);
    atomicAdd(&myhist[g / CL_BINSIZE], 1u);
  }
  __syncthreads();
  int h = 0;
#pragma unroll
  for (int w = 0; w < CL_BLOCK / 64; ++w) h += (int)hist[w][b];

  // clip_histogram: first pass
  int excess = cl_block_sum(h > clim ? h - clim : 0, part);
  h = h > clim ? clim : h;
  const int incr = excess / CL_BINS, upper = clim - incr;
  const bool low = h < upper;
  excess -= incr * __syncthreads_count(low);
  if (low) h += incr;
  const bool mid = h >= upper && h < clim;          // a raised bin that reached `upper` is filled up as well
  excess += cl_block_sum(mid ? h - clim : 0, part);
  if (mid) h = clim;
  // leftover loop; `excess` may end negative, as in the library
  while (excess > 0) {
    const int prev = excess;
    for (int index = 0; index < CL_BINS; ++index) {
      const bool under = h < clim;
      const int nunder = __syncthreads_count(under);
      int step = nunder / excess;
      step = step < 1 ? 1 : step;
      const bool inc = under && b >= index && (b - index) % step == 0;
      if (inc) h += 1;
      excess -= __syncthreads_count(inc);
      if (excess <= 0) break;
    }
    if (prev == excess) break;
  }
  // map_histogram: inclusive scan, scale in fp64, clamp, truncate
  scan[b] = h;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < CL_BINS; o <<= 1) {
    const int add = b >= o ? scan[b - o] : 0;
    __syncthreads();
    scan[b] += add;
    __syncthreads();
  }
  const double scale = (double)(CL_GRAY - 1) / (double)npx;
  double m = (double)scan[b] * scale;
  m = m > (double)(CL_GRAY - 1) ? (double)(CL_GRAY - 1) : m;
  maps[((size_t)s * q.ny * q.nx + tile) * CL_BINS + b] = (uint16_t)(int)m;
}

// step 8 -> u (uint16 plane in the workspace) and pu[s][block] = {min, max} of the block's share of u
__global__ __launch_bounds__(CL_BLOCK) void clahe_blend_kernel(const void* __restrict__ in, int dtype, ClaheGeom q,
                                                               const int32_t* __restrict__ apply,
                                                               const unsigned* __restrict__ mm,
                                                               const uint16_t* __restrict__ maps,
                                                               uint16_t* __restrict__ u, unsigned* __restrict__ pu) {
  const int s = blockIdx.y;
  if (apply && !apply[s]) return;
  const int hw = q.H * q.W;
  const size_t base = (size_t)s * hw;
  const unsigned lo = mm[2 * s], hi = mm[2 * s + 1];
  const uint16_t* mp = maps + (size_t)s * q.ny * q.nx * CL_BINS;
  unsigned ulo = 0xffffffffu, uhi = 0u;
  for (int i = blockIdx.x * CL_BLOCK + threadIdx.x; i < hw; i += gridDim.x * CL_BLOCK) {
    const int y = i / q.W, x = i - y * q.W;
    const int bin = cl_stretch(cl_load(in, dtype, base + i), lo, hi) / CL_BINSIZE;
    const int py = y + q.ky / 2, px = x + q.kx / 2;                     // position in the padded image
    const int bi = py / q.ky, bj = px / q.kx;
    const double cy = (double)(py - bi * q.ky) / (double)q.ky, cx = (double)(px - bj * q.kx) / (double)q.kx;
    float acc = 0.f;
#pragma unroll
    for (int e0 = 0; e0 < 2; ++e0) {
      int ti = bi + e0 - 1;
      ti = ti < 0 ? 0 : (ti > q.ny - 1 ? q.ny - 1 : ti);
      const double wy = e0 ? cy : 1.0 - cy;
#pragma unroll
      for (int e1 = 0; e1 < 2; ++e1) {
        int tj = bj + e1 - 1;
        tj = tj < 0 ? 0 : (tj > q.nx - 1 ? q.nx - 1 : tj);
        const double wx = e1 ? cx : 1.0 - cx;
        const double m = (double)mp[(size_t)(ti * q.nx + tj) * CL_BINS + bin];
        acc += (float)(m * (wx * wy));
      }
    }
    const unsigned v = (unsigned)acc;
    u[base + i] = (uint16_t)v;
    ulo = v < ulo ? v : ulo;
    uhi = v > uhi ? v : uhi;
  }
  cl_block_minmax(ulo, uhi);
  if (threadIdx.x == 0) {
    unsigned* p = pu + 2 * ((size_t)s * gridDim.x + blockIdx.x);
    p[0] = ulo; p[1] = uhi;
  }
}

// step 9; images with apply == 0 are copied through (fp32 -> fp32: the value itself)
__global__ __launch_bounds__(CL_BLOCK) void clahe_rescale_kernel(const void* __restrict__ in, int dtype, int hw,
                                                                 const int32_t* __restrict__ apply,
                                                                 const unsigned* __restrict__ pu,
                                                                 const uint16_t* __restrict__ u, void* __restrict__ out,
                                                                 int out_dtype) {
  const int s = blockIdx.y;
  const size_t base = (size_t)s * hw;
  const bool on = !apply || apply[s];
  const double inv = 1.0 / 65535;
  unsigned ulo = 0u, uhi = 0u;
  if (on) cl_fold_partials(pu + 2 * (size_t)s * gridDim.x, (int)gridDim.x, ulo, uhi);
  const double a = (double)ulo * inv, bmax = (double)uhi * inv;
  for (int i = blockIdx.x * CL_BLOCK + threadIdx.x; i < hw; i += gridDim.x * CL_BLOCK) {
    if (!on) {
      if (dtype == MSEG_PIX_F32 && out_dtype == MSEG_PIX_F32) {
        reinterpret_cast<float*>(out)[base + i] = reinterpret_cast<const float*>(in)[base + i];
      } else {
        const unsigned v = dtype == MSEG_PIX_U8 ? reinterpret_cast<const uint8_t*>(in)[base + i] : cl_load(in, dtype, base + i);
        if (out_dtype == MSEG_PIX_F32) reinterpret_cast<float*>(out)[base + i] = (float)v;
        else reinterpret_cast<uint16_t*>(out)[base + i] = (uint16_t)v;
      }
      continue;
    }
    double f = (double)u[base + i] * inv;
    if (a != bmax) f = (f - a) / (bmax - a);
    else f = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
    const unsigned r = (unsigned)(65535.0 * f);
    if (out_dtype == MSEG_PIX_F32) reinterpret_cast<float*>(out)[base + i] = (float)r;
    else reinterpret_cast<uint16_t*>(out)[base + i] = (uint16_t)r;
  }
}

static bool clahe_geom(int N, int H, int W, ClaheGeom* q) {
  if (N <= 0 || H < 8 || W < 8 || (long long)H * W > 0x7fffffffLL || N > 65535) return false;
  q->H = H; q->W = W;
  q->ky = H / 8; q->kx = W / 8;
  q->ny = (H + q->ky - 1) / q->ky; q->nx = (W + q->kx - 1) / q->kx;
  return true;
}

static size_t clahe_align(size_t b) { return (b + 255) & ~(size_t)255; }

// blocks per image of the streaming passes: about 2048 in all, at least 16 and at most CL_MAX_BLOCKS_X per image
static int clahe_blocks_x(int N, int hw) {
  int want = (2048 + N - 1) / N;
  want = want < 16 ? 16 : (want > CL_MAX_BLOCKS_X ? CL_MAX_BLOCKS_X : want);
  const int cap = (hw + CL_BLOCK - 1) / CL_BLOCK;
  return want < cap ? want : cap;
}

// workspace: {min, max} per image | per-block partials of the input and of u | tile maps uint16 [N][ny nx][256] | u uint16 [N][H][W]
extern "C" size_t mseg_clahe_workspace_bytes(int N, int H, int W) {
  ClaheGeom q;
  if (!clahe_geom(N, H, W, &q)) return 0;
  const size_t part = clahe_align((size_t)N * clahe_blocks_x(N, H * W) * 2 * sizeof(unsigned));
  return clahe_align((size_t)N * 2 * sizeof(unsigned)) + 2 * part +
         clahe_align((size_t)N * q.ny * q.nx * CL_BINS * sizeof(uint16_t)) +
         clahe_align((size_t)N * H * W * sizeof(uint16_t));
}

extern "C" int mseg_clahe_u16(const void* in, int in_dtype, int N, int H, int W, const int32_t* apply_dev, void* out,
                              int out_dtype, void* ws, size_t ws_bytes, void* stream) {
  ClaheGeom q;
  if (!in || !out || !ws || in == out || !clahe_geom(N, H, W, &q)) return MSEG_EINVAL;
  if (in_dtype != MSEG_PIX_U8 && in_dtype != MSEG_PIX_U16 && in_dtype != MSEG_PIX_F32) return MSEG_EINVAL;
  if (out_dtype != MSEG_PIX_U16 && out_dtype != MSEG_PIX_F32) return MSEG_EINVAL;
  if (ws_bytes < mseg_clahe_workspace_bytes(N, H, W)) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int hw = H * W, bx = clahe_blocks_x(N, hw);
  const size_t part = clahe_align((size_t)N * bx * 2 * sizeof(unsigned));
  char* p = (char*)ws;
  unsigned* mm = (unsigned*)p;   p += clahe_align((size_t)N * 2 * sizeof(unsigned));
  unsigned* pin = (unsigned*)p;  p += part;
  unsigned* pu = (unsigned*)p;   p += part;
  uint16_t* maps = (uint16_t*)p; p += clahe_align((size_t)N * q.ny * q.nx * CL_BINS * sizeof(uint16_t));
  uint16_t* u = (uint16_t*)p;
  const double lim = 0.01 * (double)(q.ky * q.kx);
  const int clim = (int)(lim > 1.0 ? lim : 1.0);
  hipLaunchKernelGGL(clahe_minmax_kernel, dim3(bx, N), dim3(CL_BLOCK), 0, st, in, in_dtype, hw, apply_dev, pin);
  hipLaunchKernelGGL(clahe_maps_kernel, dim3(q.ny * q.nx, N), dim3(CL_BLOCK), 0, st, in, in_dtype, q, clim, apply_dev,
                     (const unsigned*)pin, bx, mm, maps);
  hipLaunchKernelGGL(clahe_blend_kernel, dim3(bx, N), dim3(CL_BLOCK), 0, st, in, in_dtype, q, apply_dev,
                     (const unsigned*)mm, (const uint16_t*)maps, u, pu);
  hipLaunchKernelGGL(clahe_rescale_kernel, dim3(bx, N), dim3(CL_BLOCK), 0, st, in, in_dtype, hw, apply_dev,
                     (const unsigned*)pu, (const uint16_t*)u, out, out_dtype);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
