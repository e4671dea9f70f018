// analysis.hip — polygon ROIs -> filled / outlined stacks, region statistics and the RGB overlay.
//
// Replaces the per-polygon CPU loops of the reference's Analysis and Export workers:
//   mask[t, rr, cc] = cell_id  (skimage.draw.polygon)          src/inference/analysis.py:126-128, result_export.py:120-122
//   polygon_perimeter(r, c, shape, clip=True)                 analysis.py:130-132, result_export.py:124-126
//   regionprops(mask[frame]): area / axis lengths per cell     analysis.py:158-164
//   np.clip(255 * img / max(img)) + yellow outlines            result_export.py:183-190
// The relabel between fill and statistics (analysis.py:139-140) is mseg_stack_relabel in postproc.hip.
#include "common.h"
#include <math.h>

// skimage evaluates its point-in-polygon test in fp64 without fused multiply-adds; so does this file
#pragma clang fp contract(off)

#define AN_BLOCK 256
#define FILL_WAVE 64
#define FILL_CAP 512          // relevant edges of one polygon row kept in LDS; more -> the row tests every edge from HBM

namespace {

inline unsigned an_blocks(size_t n) {
  const size_t b = (n + AN_BLOCK - 1) / AN_BLOCK;
  return (unsigned)(b < 1 ? 1 : b);
}

inline size_t an_align(size_t v) { return (v + 255) / 256 * 256; }

// polygon k of the CSR arrays: the largest k with off[k] <= u
__device__ int upper_index(const int64_t* __restrict__ off, int n, int64_t u) {
  int lo = 0, hi = n;                       // off[lo] <= u < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- a. fill ---------------------------------------------------------------------------------------------------------
// Bounding box of skimage.draw.polygon (_draw.pyx _polygon): rows int(max(0, min r)) .. ceil(max r), columns likewise;
// rows[k] = number of rows (0 for an empty polygon or one of a frame outside the stack).
__global__ void roi_bbox_kernel(const int32_t* __restrict__ rc, const int64_t* __restrict__ voff,
                                const int32_t* __restrict__ frame, int n_poly, int T, int4* __restrict__ bbox,
                                int64_t* __restrict__ rows) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_poly) return;
  const int64_t a = voff[k], b = voff[k + 1];
  int r0 = INT32_MAX, r1 = INT32_MIN, c0 = INT32_MAX, c1 = INT32_MIN;
  for (int64_t v = a; v < b; ++v) {
    const int r = rc[2 * v], c = rc[2 * v + 1];
    r0 = min(r0, r); r1 = max(r1, r); c0 = min(c0, c); c1 = max(c1, c);
  }
  r0 = max(r0, 0); c0 = max(c0, 0);
  bbox[k] = make_int4(r0, r1, c0, c1);
  rows[k] = (b > a && r1 >= r0 && c1 >= c0 && frame[k] >= 0 && frame[k] < T) ? (int64_t)(r1 - r0 + 1) : 0;
}

// exclusive scan of rows[0..n) into off[0..n] (off[n] = total) by one workgroup: n is a polygon count (tens of thousands)
__global__ void roi_scan_kernel(const int64_t* __restrict__ rows, int n, int64_t* __restrict__ off) {
  __shared__ int64_t part[AN_BLOCK];
  const int per = (n + AN_BLOCK - 1) / AN_BLOCK;
  const int s = threadIdx.x * per, e = min(n, s + per);
  int64_t acc = 0;
  for (int i = s; i < e; ++i) acc += rows[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int i = 0; i < AN_BLOCK; ++i) { const int64_t v = part[i]; part[i] = run; run += v; }
    off[n] = run;
  }
  __syncthreads();
  int64_t run = part[threadIdx.x];
  for (int i = s; i < e; ++i) { off[i] = run; run += rows[i]; }
}

// The point test of skimage/_shared/geometry.pxd (point_in_polygon, O'Rourke), one edge (j -> i) at a time, in its fp64
// operation order.  Returns the vertex / right-crossing / left-crossing contributions as bits 0 / 1 / 2.
__device__ __forceinline__ unsigned pip_edge(double xi, double yi, double xj, double yj, double x, double y) {
  const double x0 = xi - x, y0 = yi - y, x1 = xj - x, y1 = yj - y;
  unsigned f = 0;
  if (x0 == 0.0 && y0 == 0.0) f |= 1u;                          // |x0|, |y0| < 1e-12 for integer vertices
  if ((y0 > 0.0) != (y1 > 0.0) && (x0 * y1 - x1 * y0) / (y1 - y0) > 0.0) f |= 2u;
  if ((y0 < 0.0) != (y1 < 0.0) && (x0 * y1 - x1 * y0) / (y1 - y0) < 0.0) f |= 4u;
  return f;
}

// One 64-lane workgroup per (polygon, row) unit, units handed out grid-stride: work follows bounding-box rows, so one large
// cell is spread over as many workgroups as it has rows instead of serialising one behind thousands of small ones.  The
// lanes first collect the row's relevant edges (a vertex on the row, or straddling it) into LDS, then test their pixels
// against that list only; the pixel keeps the LARGEST polygon number covering it (= the last writer of the reference loop).
__global__ void __launch_bounds__(FILL_WAVE) roi_fill_kernel(const int32_t* __restrict__ rc,
                                                             const int64_t* __restrict__ voff,
                                                             const int32_t* __restrict__ frame, int n_poly, int H, int W,
                                                             const int4* __restrict__ bbox,
                                                             const int64_t* __restrict__ roff, int32_t* __restrict__ owner) {
  __shared__ int4 edges[FILL_CAP];
  const int lane = threadIdx.x;
  const int64_t total = roff[n_poly];
  for (int64_t u = blockIdx.x; u < total; u += gridDim.x) {
    const int k = upper_index(roff, n_poly, u);
    const int4 bb = bbox[k];
    const int y = bb.x + (int)(u - roff[k]);
    const int64_t v0 = voff[k];
    const int nv = (int)(voff[k + 1] - v0);
    const int2* __restrict__ pv = (const int2*)rc + v0;           // (r, c)
    int cnt = 0;
    for (int e0 = 0; e0 < nv; e0 += FILL_WAVE) {
      const int e = e0 + lane;
      bool rel = false;
      int2 pi = make_int2(0, 0), pj = make_int2(0, 0);
      if (e < nv) {
        pi = pv[e];
        pj = pv[e == 0 ? nv - 1 : e - 1];
        rel = pi.x == y || ((pi.x > y) != (pj.x > y)) || ((pi.x < y) != (pj.x < y));
      }
      const unsigned long long m = __ballot(rel);
      const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
      if (rel && pos < FILL_CAP) edges[pos] = make_int4(pi.y, pi.x, pj.y, pj.x);   // (xi, yi, xj, yj)
      cnt += __popcll(m);
    }
    __syncthreads();
    if (y >= 0 && y < H) {
      const double yd = (double)y;
      int32_t* __restrict__ row = owner + ((size_t)frame[k] * H + y) * W;
      for (int x = bb.z + lane; x <= bb.w; x += FILL_WAVE) {
        const double xd = (double)x;
        unsigned acc = 0;
        if (cnt <= FILL_CAP) {
          for (int q = 0; q < cnt; ++q) {
            const int4 ed = edges[q];
            const unsigned f = pip_edge(ed.x, ed.y, ed.z, ed.w, xd, yd);
            acc = (acc ^ (f & 6u)) | (f & 1u);
          }
        } else {
          for (int i = 0; i < nv; ++i) {
            const int2 pi = pv[i], pj = pv[i == 0 ? nv - 1 : i - 1];
            const unsigned f = pip_edge(pi.y, pi.x, pj.y, pj.x, xd, yd);
            acc = (acc ^ (f & 6u)) | (f & 1u);
          }
        }
        if (acc && x < W) atomicMax(&row[x], k + 1);   // vertex, or an odd right or left crossing count
      }
    }
    __syncthreads();
  }
}

// owner k -> the value the reference's stack holds: uint16 until cell_id == 66535 (analysis.py:136-137), so cells
// 65536 .. 66534 wrap to k & 0xFFFF (0 erases); from 66535 on the stack is int32
__global__ void roi_value_kernel(int32_t* __restrict__ mask, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t k = mask[i];
  if (k >= 65536 && k < 66535) mask[i] = k & 0xFFFF;
}

// ---- b. outlines: skimage.draw.line (_draw.pyx _line, Bresenham) along edge (i -> i + 1) of the closed polygon ---------
__global__ void roi_outline_kernel(const int32_t* __restrict__ rc, const int64_t* __restrict__ voff,
                                   const int32_t* __restrict__ frame, int n_poly, int64_t n_vert, int T, int H, int W,
                                   uint8_t* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_vert) return;
  const int k = upper_index(voff, n_poly, g);
  const int t = frame[k];
  if (t < 0 || t >= T) return;
  const int64_t a = voff[k], b = voff[k + 1];
  const int64_t h = g + 1 < b ? g + 1 : a;
  const int r0 = rc[2 * g], c0 = rc[2 * g + 1], r1 = rc[2 * h], c1 = rc[2 * h + 1];
  uint8_t* __restrict__ img = out + (size_t)t * H * W;
  bool steep = false;
  int r = r0, c = c0, dr = abs(r1 - r0), dc = abs(c1 - c0);
  int sc = (c1 - c) > 0 ? 1 : -1, sr = (r1 - r) > 0 ? 1 : -1;
  if (dr > dc) {
    steep = true;
    int s = c; c = r; r = s;
    s = dc; dc = dr; dr = s;
    s = sc; sc = sr; sr = s;
  }
  int d = 2 * dr - dc;
  for (int i = 0; i < dc; ++i) {
    const int pr = steep ? c : r, pc = steep ? r : c;
    if ((unsigned)pr < (unsigned)H && (unsigned)pc < (unsigned)W) img[(size_t)pr * W + pc] = 1;
    while (d >= 0) { r += sr; d -= 2 * dc; }
    c += sc;
    d += 2 * dr;
  }
  if ((unsigned)r1 < (unsigned)H && (unsigned)c1 < (unsigned)W) img[(size_t)r1 * W + c1] = 1;
}

// ---- d. region statistics ----------------------------------------------------------------------------------------------
struct RsMom { unsigned long long sy, sx, syy, sxx, sxy; };

// One thread per pixel; the first pixel of each horizontal run of a label adds the run's closed-form sums (6 atomics per
// run instead of per pixel).  Integer sums are exact and order-free, so the result is deterministic.
__global__ void rs_runs_kernel(const int32_t* __restrict__ lab, int T, int H, int W, const int64_t* __restrict__ loff,
                               unsigned long long* __restrict__ area, RsMom* __restrict__ mom,
                               unsigned long long* __restrict__ total_area) {
  const size_t hw = (size_t)H * W, n = (size_t)T * hw;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t l = lab[i];
  if (l <= 0) return;
  const int t = (int)(i / hw);
  const size_t p = i - (size_t)t * hw;
  const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
  if (x > 0 && lab[i - 1] == l) return;
  const int64_t K = loff[t + 1] - loff[t];
  if (l > K) return;                                              // ids beyond the frame's table are ignored
  int e = x;
  while (e + 1 < W && lab[i + (e + 1 - x)] == l) ++e;
  const unsigned long long len = (unsigned long long)(e - x + 1);
  const unsigned long long yy = (unsigned long long)y, a = (unsigned long long)x, b = (unsigned long long)e;
  const unsigned long long sx = (a + b) * len / 2;
  const size_t s = (size_t)(loff[t] + l - 1);
  atomicAdd(&area[s], len);
  atomicAdd(&mom[s].sy, yy * len);
  atomicAdd(&mom[s].sx, sx);
  atomicAdd(&mom[s].syy, yy * yy * len);
  atomicAdd(&mom[s].sxx, run_sum_sq(a, b));
  atomicAdd(&mom[s].sxy, yy * sx);
  atomicAdd(&total_area[t], (unsigned long long)l * len);
}

__device__ __forceinline__ double i128_to_f64(__int128 v) {
  const bool neg = v < 0;
  const unsigned __int128 u = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
  const double d = (double)(unsigned long long)(u >> 64) * 18446744073709551616.0 + (double)(unsigned long long)u;
  return neg ? -d : d;
}

// regionprops: inertia tensor of the central moments / mu00, eigenvalues l1 >= l2 (clipped at 0), axis = 4 sqrt(l).
// n * sum(y^2) - sum(y)^2 etc. are formed exactly in 128 bits (n * sum(y^2) overflows 64 bits for ~1e6-px cells at
// coordinates near 8191), then divided by n^2 in fp64.
__global__ void rs_axes_kernel(const unsigned long long* __restrict__ area, const RsMom* __restrict__ mom, int64_t n_lab,
                               double* __restrict__ major, double* __restrict__ minor) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_lab) return;
  const unsigned long long cnt = area[s];
  if (!cnt) { major[s] = 0.0; minor[s] = 0.0; return; }
  const RsMom m = mom[s];
  const __int128 N = (__int128)cnt;
  const double nn = (double)cnt * (double)cnt;
  const double a = i128_to_f64(N * (__int128)m.syy - (__int128)m.sy * (__int128)m.sy) / nn;
  const double c = i128_to_f64(N * (__int128)m.sxx - (__int128)m.sx * (__int128)m.sx) / nn;
  const double b = i128_to_f64(N * (__int128)m.sxy - (__int128)m.sx * (__int128)m.sy) / nn;
  const double h = 0.5 * (a + c), q = sqrt(0.25 * (a - c) * (a - c) + b * b);
  const double l1 = h + q, l2 = h - q;
  major[s] = 4.0 * sqrt(fmax(l1, 0.0));
  minor[s] = 4.0 * sqrt(fmax(l2, 0.0));
}

// ---- e. overlay ---------------------------------------------------------------------------------------------------------
template <typename P>
__global__ void ov_max_kernel(const P* __restrict__ img, size_t n, uint32_t* __restrict__ mx) {
  uint32_t m = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    m = max(m, (uint32_t)img[i]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(mx, m);
}

// out[t][y][x][ch] = uint8(clip(255 * f32(img) / f32(max), 0, 255)) (truncation; NaN of an all-zero image -> 0), outline
// pixels (255, 255, 0) in channels 0..2.  Cin == 1: the grey value in three channels.
template <typename P>
__global__ void ov_kernel(const P* __restrict__ img, size_t npx, int Cin, int Cout, const uint8_t* __restrict__ outl,
                          const uint32_t* __restrict__ mx, uint8_t* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= npx * (size_t)Cout) return;
  const size_t px = e / Cout;
  const int ch = (int)(e - px * Cout);
  uint8_t v;
  if (ch < 3 && outl[px]) {
    v = ch == 2 ? 0 : 255;
  } else {
    const float f = 255.0f * (float)img[Cin == 1 ? px : e] / (float)*mx;
    const float cl = f > 255.0f ? 255.0f : (f < 0.0f ? 0.0f : f);
    v = cl == cl ? (uint8_t)cl : (uint8_t)0;
  }
  out[e] = v;
}

}  // namespace

// ---- entry points ---------------------------------------------------------------------------------------------------------
extern "C" size_t mseg_roi_fill_workspace_bytes(int n_poly) {
  if (n_poly < 0) return 0;
  const size_t n = (size_t)n_poly;
  return an_align(sizeof(int4) * (n + 1)) + an_align(sizeof(int64_t) * (n + 1)) + an_align(sizeof(int64_t) * (n + 1));
}

extern "C" int mseg_roi_fill(const int32_t* rc, const int64_t* voff, const int32_t* frame, int n_poly, int T, int H, int W,
                             int32_t* mask, void* ws, size_t ws_bytes, void* stream) {
  if (!mask || !ws || n_poly < 0 || T <= 0 || H <= 0 || W <= 0) return MSEG_EINVAL;
  if (n_poly > 0 && (!rc || !voff || !frame)) return MSEG_EINVAL;
  if (ws_bytes < mseg_roi_fill_workspace_bytes(n_poly)) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)T * H * W;
  if (hipMemsetAsync(mask, 0, n * sizeof(int32_t), st) != hipSuccess) return MSEG_ELAUNCH;
  if (n_poly == 0) return MSEG_OK;
  char* b = (char*)ws;
  int4* bbox = (int4*)b;
  int64_t* rows = (int64_t*)(b + an_align(sizeof(int4) * (n_poly + 1)));
  int64_t* roff = (int64_t*)((char*)rows + an_align(sizeof(int64_t) * (n_poly + 1)));
  hipLaunchKernelGGL(roi_bbox_kernel, dim3(an_blocks(n_poly)), dim3(AN_BLOCK), 0, st, rc, voff, frame, n_poly, T, bbox, rows);
  hipLaunchKernelGGL(roi_scan_kernel, dim3(1), dim3(AN_BLOCK), 0, st, (const int64_t*)rows, n_poly, roff);
  hipLaunchKernelGGL(roi_fill_kernel, dim3(8192), dim3(FILL_WAVE), 0, st, rc, voff, frame, n_poly, H, W,
                     (const int4*)bbox, (const int64_t*)roff, mask);
  hipLaunchKernelGGL(roi_value_kernel, dim3(an_blocks(n)), dim3(AN_BLOCK), 0, st, mask, n);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

extern "C" int mseg_roi_outline(const int32_t* rc, const int64_t* voff, const int32_t* frame, int n_poly, int64_t n_vert,
                                int T, int H, int W, uint8_t* outlines, void* stream) {
  if (!outlines || n_poly < 0 || n_vert < 0 || T <= 0 || H <= 0 || W <= 0) return MSEG_EINVAL;
  if (n_poly > 0 && (!rc || !voff || !frame)) return MSEG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(outlines, 0, (size_t)T * H * W, st) != hipSuccess) return MSEG_ELAUNCH;
  if (n_poly == 0 || n_vert == 0) return MSEG_OK;
  hipLaunchKernelGGL(roi_outline_kernel, dim3(an_blocks((size_t)n_vert)), dim3(AN_BLOCK), 0, st, rc, voff, frame, n_poly,
                     n_vert, T, H, W, outlines);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

extern "C" size_t mseg_region_stats_workspace_bytes(int64_t n_labels) {
  return n_labels < 0 ? 0 : an_align(sizeof(RsMom) * (size_t)(n_labels + 1));
}

extern "C" int mseg_region_stats(const int32_t* labels, int T, int H, int W, const int64_t* label_off, int64_t n_labels,
                                 int64_t* area, double* major, double* minor, uint64_t* total_area, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!labels || !label_off || !total_area || !ws || T <= 0 || H <= 0 || W <= 0 || n_labels < 0) return MSEG_EINVAL;
  if (n_labels > 0 && (!area || !major || !minor)) return MSEG_EINVAL;
  if (ws_bytes < mseg_region_stats_workspace_bytes(n_labels)) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(total_area, 0, sizeof(uint64_t) * (size_t)T, st) != hipSuccess) return MSEG_ELAUNCH;
  if (n_labels == 0) return MSEG_OK;
  if (hipMemsetAsync(area, 0, sizeof(int64_t) * (size_t)n_labels, st) != hipSuccess) return MSEG_ELAUNCH;
  if (hipMemsetAsync(ws, 0, sizeof(RsMom) * (size_t)n_labels, st) != hipSuccess) return MSEG_ELAUNCH;
  const size_t n = (size_t)T * H * W;
  hipLaunchKernelGGL(rs_runs_kernel, dim3(an_blocks(n)), dim3(AN_BLOCK), 0, st, labels, T, H, W, label_off,
                     (unsigned long long*)area, (RsMom*)ws, (unsigned long long*)total_area);
  hipLaunchKernelGGL(rs_axes_kernel, dim3(an_blocks((size_t)n_labels)), dim3(AN_BLOCK), 0, st,
                     (const unsigned long long*)area, (const RsMom*)ws, n_labels, major, minor);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

extern "C" size_t mseg_overlay_workspace_bytes(void) { return 256; }

extern "C" int mseg_overlay_rgb(const void* img, int dtype, int T, int H, int W, int C, const uint8_t* outlines,
                                uint8_t* out, void* ws, size_t ws_bytes, void* stream) {
  if (!img || !outlines || !out || !ws || T <= 0 || H <= 0 || W <= 0 || (C != 1 && C < 3)) return MSEG_EINVAL;
  if (dtype != MSEG_PIX_U8 && dtype != MSEG_PIX_U16) return MSEG_EINVAL;
  if (ws_bytes < mseg_overlay_workspace_bytes()) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* mx = (uint32_t*)ws;
  if (hipMemsetAsync(mx, 0, sizeof(uint32_t), st) != hipSuccess) return MSEG_ELAUNCH;
  const size_t npx = (size_t)T * H * W, nin = npx * (size_t)C;
  const int Cout = C == 1 ? 3 : C;
  const unsigned gmax = an_blocks(nin) < 2048 ? an_blocks(nin) : 2048;
  if (dtype == MSEG_PIX_U8) {
    hipLaunchKernelGGL(ov_max_kernel<uint8_t>, dim3(gmax), dim3(AN_BLOCK), 0, st, (const uint8_t*)img, nin, mx);
    hipLaunchKernelGGL(ov_kernel<uint8_t>, dim3(an_blocks(npx * Cout)), dim3(AN_BLOCK), 0, st, (const uint8_t*)img, npx, C,
                       Cout, outlines, (const uint32_t*)mx, out);
  } else {
    hipLaunchKernelGGL(ov_max_kernel<uint16_t>, dim3(gmax), dim3(AN_BLOCK), 0, st, (const uint16_t*)img, nin, mx);
    hipLaunchKernelGGL(ov_kernel<uint16_t>, dim3(an_blocks(npx * Cout)), dim3(AN_BLOCK), 0, st, (const uint16_t*)img, npx,
                       C, Cout, outlines, (const uint32_t*)mx, out);
  }
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
