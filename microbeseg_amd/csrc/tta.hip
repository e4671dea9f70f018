// tta.hip — test-time augmentation for inference: the members of a frame under the flips / rotations of
// the square (mseg_tta_expand) and the merge of their predictions (mseg_tta_merge).  Both are pure data movement plus, in
// the merge, one ordered fp32 sum per output element; both are HBM-bound.
//
// Codes are those of aug_flip_src (augment.hip), extended to rectangles.  With a of H x W and T_c(a) the member:
//   code   0        1        2        3        4        5        6        7
//   T_c    a        fliplr   flipud   rot90    rot180   rot270   a.T      rot90(flipud)
//   (t, fy, fx)  000  001     010      101      011      110      100      111
// T_c(a)[i][j] = a[fy ? H-1-s : s][fx ? W-1-r : r] with (s, r) = (i, j) for t = 0 and (j, i) for t = 1 (the member is
// W x H then).  Read the other way: frame pixel (y, x) sits at member position (y', x') (t = 0) or (x', y') (t = 1) with
// y' = fy ? H-1-y : y, x' = fx ? W-1-x : x — the same expression serves the expansion and the mapping back.
//
// Memory access: a destination tile is 32 x 32, a block 32 x 8 threads, lanes run along the destination row.  A member that
// does not transpose is read directly: its row runs with the destination row, forwards or backwards, so a wave reads whole
// 128-byte lines.  A member that transposes is staged through LDS (TtaTile, row pitch 33 words: odd, so the column read
// touches 32 different banks): the global read runs along the SOURCE row, the LDS read along the column.
#include "common.h"

#define TTA_TILE 32
#define TTA_ROWS 8                         // threadIdx.y; a thread owns TTA_TILE / TTA_ROWS rows of the tile
#define TTA_PER (TTA_TILE / TTA_ROWS)
#define TTA_PITCH (TTA_TILE + 1)
#define TTA_MAX 8

typedef float TtaTile[TTA_TILE][TTA_PITCH];

__device__ __forceinline__ bool tta_transposes(int code) { return code == 3 || code == 5 || code == 6 || code == 7; }
__device__ __forceinline__ bool tta_flips_y(int code) { return code == 2 || code == 4 || code == 5 || code == 7; }
__device__ __forceinline__ bool tta_flips_x(int code) { return code == 1 || code == 3 || code == 4 || code == 7; }

// The one tiling of both kernels.  Destination tile origin (a0, b0), extent A x B; the source is addressed (b, a): `load(b,
// a)` returns the element whose SOURCE row belongs to destination column b and whose source column belongs to destination
// row a.  Stage: lanes run along a, i.e. along the source row.  Read: the thread of destination (a0 + la, b0 + lb) takes
// tile[lb][la].  The caller puts a __syncthreads() between the two.
template <typename Load>
__device__ __forceinline__ void tta_stage_transposed(TtaTile& tile, int a0, int b0, int A, int B, Load load) {
#pragma unroll
  for (int r = 0; r < TTA_PER; ++r) {
    const int lb = threadIdx.y + TTA_ROWS * r, la = threadIdx.x;
    if (a0 + la < A && b0 + lb < B) tile[lb][la] = load(b0 + lb, a0 + la);
  }
}
__device__ __forceinline__ float tta_read_transposed(const TtaTile& tile, int la, int lb) { return tile[lb][la]; }

// ---- expand ----------------------------------------------------------------------------------------------------------------
struct TtaExpand {
  const void* src;            // [n][H0][W0]
  const uint32_t* minmax;     // [n][2] {~min, max} (frames_minmax_kernel); unused for MSEG_PIX_F32
  float* out;                 // [k][n][Hp][Wp]
  int dtype, n, H0, W0, pad_top, pad_left, Hp, Wp, k;
  int code[TTA_MAX];
};

__device__ __forceinline__ float tta_src_px(const TtaExpand& p, size_t frame, int sy, int sx, float fmin, float frange) {
  const size_t i = (frame * p.H0 + sy) * (size_t)p.W0 + sx;
  if (p.dtype == MSEG_PIX_F32) return reinterpret_cast<const float*>(p.src)[i];
  const unsigned v = p.dtype == MSEG_PIX_U8 ? reinterpret_cast<const uint8_t*>(p.src)[i]
                                            : reinterpret_cast<const uint16_t*>(p.src)[i];
  return raw_frame_norm(v, fmin, frange);        // common.h: the fp32 operations of first.hip, in its order
}

// grid: x = tiles of the padded member, y = frame, z = member.  Every pixel of the member is written once: -1 in the top /
// left padding (the value the host formula gives for the pad value `min`), the transformed frame elsewhere.
__global__ __launch_bounds__(TTA_TILE * TTA_ROWS) void tta_expand_kernel(const TtaExpand p) {
  __shared__ TtaTile tile;
  const int tiles_x = (p.Wp + TTA_TILE - 1) / TTA_TILE;
  const int Y0 = (int)(blockIdx.x / tiles_x) * TTA_TILE, X0 = (int)(blockIdx.x % tiles_x) * TTA_TILE;
  const size_t frame = blockIdx.y;
  const int code = p.code[blockIdx.z];
  const bool t = tta_transposes(code), fy = tta_flips_y(code), fx = tta_flips_x(code);
  float fmin = 0.f, frange = 1.f;
  if (p.dtype != MSEG_PIX_F32) {
    const unsigned lo = ~p.minmax[2 * frame], hi = p.minmax[2 * frame + 1];
    fmin = (float)lo; frange = (float)(hi - lo);
  }
  float* o = p.out + ((size_t)blockIdx.z * p.n + frame) * ((size_t)p.Hp * p.Wp);
  if (t) {      // member pixel (Y, X) = frame pixel (fy ? H0-1-j : j, fx ? W0-1-i : i), i = Y - pad_top, j = X - pad_left
    tta_stage_transposed(tile, Y0, X0, p.Hp, p.Wp, [&](int X, int Y) -> float {
      const int i = Y - p.pad_top, j = X - p.pad_left;
      if (i < 0 || j < 0) return -1.f;
      return tta_src_px(p, frame, fy ? p.H0 - 1 - j : j, fx ? p.W0 - 1 - i : i, fmin, frange);
    });
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < TTA_PER; ++r) {
    const int ly = threadIdx.y + TTA_ROWS * r, Y = Y0 + ly, X = X0 + (int)threadIdx.x;
    if (Y >= p.Hp || X >= p.Wp) continue;
    float v;
    if (t) {
      v = tta_read_transposed(tile, ly, threadIdx.x);
    } else {
      const int i = Y - p.pad_top, j = X - p.pad_left;
      v = (i < 0 || j < 0) ? -1.f : tta_src_px(p, frame, fy ? p.H0 - 1 - i : i, fx ? p.W0 - 1 - j : j, fmin, frange);
    }
    o[(size_t)Y * p.Wp + X] = v;
  }
}

extern "C" int mseg_tta_expand(const void* src, int dtype, int n, int H0, int W0, const uint32_t* minmax,
                               const int32_t* codes, int k, int pad_top, int pad_left, float* out, void* stream) {
  if (!src || !out || !codes || n <= 0 || n > 65535 || H0 <= 0 || W0 <= 0 || pad_top < 0 || pad_left < 0 || k < 1 ||
      k > TTA_MAX)
    return MSEG_EINVAL;
  if (dtype != MSEG_PIX_U8 && dtype != MSEG_PIX_U16 && dtype != MSEG_PIX_F32) return MSEG_EINVAL;
  if (dtype != MSEG_PIX_F32 && !minmax) return MSEG_EINVAL;
  TtaExpand p;
  for (int m = 0; m < TTA_MAX; ++m) p.code[m] = 0;
  int transposing = 0;
  for (int m = 0; m < k; ++m) {
    if (codes[m] < 0 || codes[m] > 7) return MSEG_EINVAL;
    p.code[m] = codes[m];
    transposing += (codes[m] == 3 || codes[m] == 5 || codes[m] == 6 || codes[m] == 7) ? 1 : 0;
  }
  if (transposing != 0 && transposing != k) return MSEG_EINVAL;      // one shape class per call
  const int Hm = transposing ? W0 : H0, Wm = transposing ? H0 : W0;
  if ((long long)Hm + pad_top > 0x7fffffffLL || (long long)Wm + pad_left > 0x7fffffffLL) return MSEG_EINVAL;
  p.src = src; p.minmax = minmax; p.out = out;
  p.dtype = dtype; p.n = n; p.H0 = H0; p.W0 = W0; p.pad_top = pad_top; p.pad_left = pad_left;
  p.Hp = Hm + pad_top; p.Wp = Wm + pad_left; p.k = k;
  const long long tiles = (long long)((p.Hp + TTA_TILE - 1) / TTA_TILE) * ((p.Wp + TTA_TILE - 1) / TTA_TILE);
  if (tiles > 0x7fffffffLL) return MSEG_EINVAL;
  hipLaunchKernelGGL(tta_expand_kernel, dim3((unsigned)tiles, (unsigned)n, (unsigned)k), dim3(TTA_TILE, TTA_ROWS), 0,
                     (hipStream_t)stream, p);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

// ---- merge -----------------------------------------------------------------------------------------------------------------
struct TtaMerge {
  MsegTtaMember m[TTA_MAX];      // by value in the kernel arguments: no device-side table
  float* dst;
  long long dfs, dcs, drs, dps;
  int k, n, C, H, W;
  float scale;                   // 1 / k, exact: k is a power of two
};

// grid: x = 32 x 32 tiles of the frame, y = frame; the channels are a loop (an HWC source keeps its lines in this CU's
// cache from one channel to the next).  P = (((p_0 + p_1) + p_2) + ...) * (1 / k): registers only, one store per element.
__global__ __launch_bounds__(TTA_TILE * TTA_ROWS) void tta_merge_kernel(const TtaMerge p) {
  __shared__ TtaTile tile[TTA_MAX];
  const int tiles_x = (p.W + TTA_TILE - 1) / TTA_TILE;
  const int y0 = (int)(blockIdx.x / tiles_x) * TTA_TILE, x0 = (int)(blockIdx.x % tiles_x) * TTA_TILE;
  const long long frame = blockIdx.y;
  for (int ch = 0; ch < p.C; ++ch) {
    int staged = 0;
    for (int m = 0; m < p.k; ++m) {
      const MsegTtaMember& M = p.m[m];
      if (!tta_transposes(M.code)) continue;
      const bool fy = tta_flips_y(M.code), fx = tta_flips_x(M.code);
      const float* s = M.ptr + frame * M.frame_stride + ch * M.chan_stride;
      // frame pixel (y, x) is member element [x'][y']: the member's row runs along y
      tta_stage_transposed(tile[staged], y0, x0, p.H, p.W, [&](int x, int y) -> float {
        const long long i = fx ? p.W - 1 - x : x, j = fy ? p.H - 1 - y : y;
        return s[i * M.row_stride + j * M.pix_stride];
      });
      ++staged;
    }
    if (staged) __syncthreads();
#pragma unroll
    for (int r = 0; r < TTA_PER; ++r) {
      const int ly = threadIdx.y + TTA_ROWS * r, y = y0 + ly, x = x0 + (int)threadIdx.x;
      if (y >= p.H || x >= p.W) continue;
      float acc = 0.f;
      int t = 0;
      for (int m = 0; m < p.k; ++m) {
        const MsegTtaMember& M = p.m[m];
        float v;
        if (tta_transposes(M.code)) {
          v = tta_read_transposed(tile[t++], ly, threadIdx.x);
        } else {
          const long long i = tta_flips_y(M.code) ? p.H - 1 - y : y, j = tta_flips_x(M.code) ? p.W - 1 - x : x;
          v = M.ptr[frame * M.frame_stride + ch * M.chan_stride + i * M.row_stride + j * M.pix_stride];
        }
        acc = m == 0 ? v : __fadd_rn(acc, v);
      }
      p.dst[frame * p.dfs + ch * p.dcs + (long long)y * p.drs + (long long)x * p.dps] = __fmul_rn(acc, p.scale);
    }
    if (staged && ch + 1 < p.C) __syncthreads();      // the tiles are refilled for the next channel
  }
}

extern "C" int mseg_tta_merge(const MsegTtaMember* members, int k, int n, int C, int H, int W, float* dst,
                              long long dst_frame_stride, long long dst_chan_stride, long long dst_row_stride,
                              long long dst_pix_stride, void* stream) {
  if (!members || !dst || (k != 1 && k != 2 && k != 4 && k != 8) || n <= 0 || n > 65535 || C <= 0 || H <= 0 || W <= 0)
    return MSEG_EINVAL;
  TtaMerge p;
  for (int m = 0; m < TTA_MAX; ++m) p.m[m] = members[0];
  for (int m = 0; m < k; ++m) {
    if (!members[m].ptr || members[m].code < 0 || members[m].code > 7) return MSEG_EINVAL;
    p.m[m] = members[m];
  }
  p.dst = dst; p.dfs = dst_frame_stride; p.dcs = dst_chan_stride; p.drs = dst_row_stride; p.dps = dst_pix_stride;
  p.k = k; p.n = n; p.C = C; p.H = H; p.W = W; p.scale = 1.f / (float)k;
  const long long tiles = (long long)((H + TTA_TILE - 1) / TTA_TILE) * ((W + TTA_TILE - 1) / TTA_TILE);
  if (tiles > 0x7fffffffLL) return MSEG_EINVAL;
  hipLaunchKernelGGL(tta_merge_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(TTA_TILE, TTA_ROWS), 0, (hipStream_t)stream,
                     p);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
