// spots.hip — fluorescent foci of a segmented stack: an exact integer band-pass (difference of two binomial smoothings) over
// every pixel of every measured channel, a peak search, and the spots counted per cell.  An extension of the
// per-cell table (cells.hip, §6l).
//
//   B_k(v)  = the separable smoothing with the taps C(2k, j), j = 0 .. 2k, along rows, then along columns, over the plane
//             extended by its edge values (coordinates clamped); not normalised: the taps sum to 4^k per axis
//   D       = 16^s B_s(v) - B_2s(v), exact in int64 (every term < 65535 * 16^10 < 2^56)
//   a spot  = a pixel p with D(p) >= thr * 16^(2s) that beats its up to eight neighbours q inside the frame: D(p) > D(q), or
//             D(p) == D(q) and p before q in raster order
//
//   sp_init_kernel  the two tap rows into the workspace; the counters, the cursor and the status word cleared
//   sp_tile_kernel  one workgroup per 32 x 64 tile of one frame and channel: the tile and a ring of 2s + 1 pixels staged in
//                   LDS (clamped reads: the edge extension), both horizontal passes into LDS, the vertical passes and D on
//                   the tile and a ring of 1 in registers, D into LDS over the horizontal sums, the peak test on the tile;
//                   per spot one atomic add on its cell's (or its frame's background) counter and one on the list cursor
// Integers only, order-free integer adds; the list arrives in any order and is sorted by the caller.
#include "cell_common.h"

#define SP_TH 32
#define SP_TW 64
#define SP_BLOCK 256
#define SP_MAXS 5
#define SP_DH (SP_TH + 2)                                   // D: the tile and a ring of 1
#define SP_DW (SP_TW + 2)
#define SP_DN ((SP_DH * SP_DW + SP_BLOCK - 1) / SP_BLOCK)   // D values a thread holds
#define SP_TAPS_A 0                                         // workspace: C(2s, j), j = 0 .. 2s
#define SP_TAPS_B (2 * SP_MAXS + 1)                         //            C(4s, j), j = 0 .. 4s
#define SP_NTAPS (SP_TAPS_B + 4 * SP_MAXS + 1)
#define SP_WS_BYTES 256

namespace {

inline size_t sp_align16(size_t v) { return (v + 15) / 16 * 16; }

// LDS of one workgroup: the input tile, then the horizontal sums (uint32 B_s, H2 B_2s), D over the latter two
inline size_t sp_lds_bytes(int s, size_t pix_bytes, size_t h2_bytes) {
  const size_t ih = SP_DH + 4 * s, iw = SP_DW + 4 * s;
  const size_t sums = ih * SP_DW * (4 + h2_bytes), dd = (size_t)SP_DH * SP_DW * 8;
  return sp_align16(ih * iw * pix_bytes) + (sums > dd ? sums : dd);
}

__global__ void __launch_bounds__(SP_BLOCK) sp_init_kernel(uint32_t* __restrict__ taps, int s, int32_t* __restrict__ cell_count,
                                                           int64_t n_cell, int32_t* __restrict__ bg_count, int64_t n_bg,
                                                           u64* __restrict__ n_found, int32_t* __restrict__ status) {
  const int64_t i0 = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * SP_BLOCK;
  if (i0 < SP_NTAPS) {
    const int k = i0 < SP_TAPS_B ? 2 * s : 4 * s, j = (int)(i0 < SP_TAPS_B ? i0 : i0 - SP_TAPS_B);
    u64 c = 0;
    if (j <= k) {
      c = 1;
      for (int i = 0; i < j; ++i) c = c * (u64)(k - i) / (u64)(i + 1);      // exact: a binomial coefficient at every step
    }
    taps[i0] = (uint32_t)c;                                                    // C(20, 10) = 184756
  }
  if (i0 == 0) { *n_found = 0; *status = 0; }
  for (int64_t i = i0; i < n_cell; i += step) cell_count[i] = 0;
  for (int64_t i = i0; i < n_bg; i += step) bg_count[i] = 0;
}

// H2: the type of the horizontal sums of B_2s: uint32 wherever 4^(2s) * the largest pixel value fits (uint8: always,
// uint16: s <= 4), else 64 bits.  S = s at compile time: the tap loops have fixed trip counts, so the compiler unrolls them
// and reads the taps once, into scalar registers, instead of once per position
template <typename L, typename P, typename H2, int S>
__global__ void __launch_bounds__(SP_BLOCK) sp_tile_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                           const int64_t* __restrict__ loff, int64_t n,
                                                           const P* __restrict__ img, int C, int64_t fs, int64_t cs, int64_t rs,
                                                           int64_t ps, int64_t thr, const uint32_t* __restrict__ taps,
                                                           int tiles_x, int tiles_y, int32_t* __restrict__ cell_count,
                                                           int32_t* __restrict__ bg_count, MsegSpot* __restrict__ spots,
                                                           int64_t cap, u64* __restrict__ n_found, int32_t* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char sp_lds[];
  const int tid = threadIdx.x;
  unsigned b = blockIdx.x;
  const int tx = (int)(b % (unsigned)tiles_x);
  b /= (unsigned)tiles_x;
  const int ty = (int)(b % (unsigned)tiles_y);
  b /= (unsigned)tiles_y;
  const int c = (int)(b % (unsigned)C), t = (int)(b / (unsigned)C);
  if (t >= T) return;
  constexpr int s = S, s2 = 2 * s, ih = SP_DH + 2 * s2, iw = SP_DW + 2 * s2;      // the input tile: D's area and a ring of 2s
  constexpr size_t in_bytes = ((size_t)ih * iw * sizeof(P) + 15) / 16 * 16;
  P* in = (P*)sp_lds;                                                  // [ih][iw]
  uint32_t* h1 = (uint32_t*)(sp_lds + in_bytes);                       // [ih][SP_DW]: rows of B_s
  H2* h2 = (H2*)(sp_lds + in_bytes + (size_t)ih * SP_DW * 4);          // [ih][SP_DW]: rows of B_2s (264 bytes per h1 row: aligned)
  int64_t* dd = (int64_t*)(sp_lds + in_bytes);                         // [SP_DH][SP_DW], once h1 and h2 are read
  const uint32_t* ta = taps + SP_TAPS_A;
  const uint32_t* tb = taps + SP_TAPS_B;

  // the tile and its ring, coordinates clamped to the frame: no read leaves the plane, and this is the edge extension
  const int y0 = ty * SP_TH - 1 - s2, x0 = tx * SP_TW - 1 - s2;
  const P* plane = img + (int64_t)t * fs + (int64_t)c * cs;
  // All loads of a lane are issued before the first is stored: one trip to memory per workgroup, not one per element
  constexpr int n_in = (ih * iw + SP_BLOCK - 1) / SP_BLOCK;             // 11 at s = 1, 19 at s = 5
  P staged[n_in];
#pragma unroll
  for (int k = 0; k < n_in; ++k) {
    const int e = min(tid + k * SP_BLOCK, ih * iw - 1);                 // no branch: a lane past the end reads the last element
    const int r = e / iw, q = e - r * iw;
    const int y = min(max(y0 + r, 0), H - 1), x = min(max(x0 + q, 0), W - 1);
    staged[k] = plane[(int64_t)y * rs + (int64_t)x * ps];
  }
#pragma unroll
  for (int k = 0; k < n_in; ++k) {
    const int e = tid + k * SP_BLOCK;
    if (e < ih * iw) in[e] = staged[k];
  }
  __syncthreads();

  // along rows: column q of the sums is centred on input column q + 2s
  for (int e = tid; e < ih * SP_DW; e += SP_BLOCK) {
    const int r = e / SP_DW, q = e - r * SP_DW;
    const P* row = in + r * iw + q;
    H2 wide = 0;
#pragma unroll
    for (int j = 0; j <= 2 * s2; ++j) wide += (H2)tb[j] * (H2)row[j];
    uint32_t narrow = 0;
#pragma unroll
    for (int j = 0; j <= s2; ++j) narrow += ta[j] * (uint32_t)row[s + j];    // <= 65535 * 4^5 < 2^26
    h1[e] = narrow;
    h2[e] = wide;
  }
  __syncthreads();

  // along columns: row r of D is centred on row r + 2s of the sums
  int64_t d[SP_DN];
#pragma unroll
  for (int k = 0; k < SP_DN; ++k) {
    const int e = tid + k * SP_BLOCK;
    d[k] = 0;
    if (e < SP_DH * SP_DW) {
      const int r = e / SP_DW, q = e - r * SP_DW;
      u64 a1 = 0, a2 = 0;
#pragma unroll
      for (int j = 0; j <= s2; ++j) a1 += (u64)ta[j] * (u64)h1[(r + s + j) * SP_DW + q];
#pragma unroll
      for (int j = 0; j <= 2 * s2; ++j) a2 += (u64)tb[j] * (u64)h2[(r + j) * SP_DW + q];
      d[k] = (int64_t)(a1 << (4 * s)) - (int64_t)a2;                    // both < 2^56
    }
  }
  __syncthreads();                                                       // every thread has read the sums
#pragma unroll
  for (int k = 0; k < SP_DN; ++k) {
    const int e = tid + k * SP_BLOCK;
    if (e < SP_DH * SP_DW) dd[e] = d[k];
  }
  __syncthreads();

  const int64_t k_t = (t + 1 < T ? loff[t + 1] : n) - loff[t];           // the frame's table
  for (int e = tid; e < SP_TH * SP_TW; e += SP_BLOCK) {
    const int r = e / SP_TW, q = e - r * SP_TW;
    const int y = ty * SP_TH + r, x = tx * SP_TW + q;
    if (y >= H || x >= W) continue;
    const int64_t v = dd[(r + 1) * SP_DW + q + 1];
    if (v < thr) continue;
    bool peak = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (dy == 0 && dx == 0) continue;
        if (y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W) continue;      // outside the frame: takes no part
        const int64_t w = dd[(r + 1 + dy) * SP_DW + q + 1 + dx];
        peak = peak && ((dy < 0 || (dy == 0 && dx < 0)) ? v > w : v >= w);
      }
    if (!peak) continue;
    const int l = (int)lab[((int64_t)t * H + y) * W + x];
    if (l == 0) {
      atomicAdd(&bg_count[(int64_t)t * C + c], 1);
    } else if (cell_id(l, k_t)) {
      const int64_t slot = loff[t] + l - 1;
      if (slot >= 0 && slot < n) atomicAdd(&cell_count[(int64_t)c * n + slot], 1);
    }
    const u64 at = atomicAdd(n_found, 1ull);
    if (at < (u64)cap) {
      MsegSpot rec;
      rec.frame = t; rec.channel = c; rec.y = y; rec.x = x;
      rec.label = (int32_t)l;
      rec.value = (int32_t)in[(r + 1 + s2) * iw + q + 1 + s2];
      rec.d = v;
      spots[at] = rec;
    } else {
      atomicOr(status, 1);
    }
  }
}

template <typename L, typename P, typename H2, int S>
void sp_launch_s(hipStream_t st, unsigned tiles, const void* labels, int T, int H, int W, const int64_t* loff, int64_t n,
               const void* img, int C, int64_t fs, int64_t cs, int64_t rs, int64_t ps, int64_t thr, const uint32_t* taps, int tiles_x,
                 int tiles_y, int32_t* cell_count, int32_t* bg_count, MsegSpot* spots, int64_t cap, u64* n_found,
                 int32_t* status) {
  hipLaunchKernelGGL((sp_tile_kernel<L, P, H2, S>), dim3(tiles), dim3(SP_BLOCK), sp_lds_bytes(S, sizeof(P), sizeof(H2)), st,
                     (const L*)labels, T, H, W, loff, n, (const P*)img, C, fs, cs, rs, ps, thr, taps, tiles_x, tiles_y,
                     cell_count, bg_count, spots, cap, n_found, status);
}

// W5: the type of the B_2s row sums at s = 5 (uint16 images: 64 bits, 65535 * 4^10 >= 2^32); below that 32 bits always do
template <typename L, typename P, typename... A>
void sp_launch(int s, A... a) {
  typedef typename std::conditional<sizeof(P) == 1, uint32_t, u64>::type W5;
  switch (s) {
    case 1: sp_launch_s<L, P, uint32_t, 1>(a...); break;
    case 2: sp_launch_s<L, P, uint32_t, 2>(a...); break;
    case 3: sp_launch_s<L, P, uint32_t, 3>(a...); break;
    case 4: sp_launch_s<L, P, uint32_t, 4>(a...); break;
    default: sp_launch_s<L, P, W5, 5>(a...); break;
  }
}

}  // namespace

// ---- entry points -------------------------------------------------------------------------------------------------------
extern "C" size_t mseg_cell_spots_workspace_bytes(int T, int64_t n_labels, int C) {
  if (T <= 0 || n_labels < 0 || C < 1 || (int64_t)T * C > (1 << 20)) return 0;
  return SP_WS_BYTES;                                               // the two tap rows; nothing per frame, channel or cell
}

extern "C" int mseg_cell_spots(const void* labels, int label_dtype, int T, int H, int W, const int64_t* label_off,
                               int64_t n_labels, const void* img, int img_dtype, int C, int64_t frame_stride,
                               int64_t chan_stride, int64_t row_stride, int64_t pix_stride, int scale, int threshold,
                               int32_t* cell_count, int32_t* bg_count, MsegSpot* spots, int64_t spot_cap, int64_t* n_spots,
                               int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!img || !bg_count || !n_spots || !status || !ws) return MSEG_EINVAL;
  if (!cell_stack_ok(labels, label_off, label_dtype, T, H, W, 512) || !cell_image_ok(img_dtype)) return MSEG_EINVAL;
  if (n_labels < 0 || C < 1) return MSEG_EINVAL;
  if (scale < 1 || scale > SP_MAXS || threshold < 1 || threshold > 65535) return MSEG_EINVAL;
  if (spot_cap < 0 || spot_cap > (1ll << 32) || (spot_cap > 0 && !spots)) return MSEG_EINVAL;
  if (n_labels > 0 && !cell_count) return MSEG_EINVAL;
  const size_t need = mseg_cell_spots_workspace_bytes(T, n_labels, C);
  if (need == 0) return MSEG_EINVAL;
  const int tiles_x = (W + SP_TW - 1) / SP_TW, tiles_y = (H + SP_TH - 1) / SP_TH;
  const int64_t tiles = (int64_t)T * C * tiles_x * tiles_y;
  if (tiles > 0x7FFFFFFFll || n_labels > (1ll << 40) / C) return MSEG_EINVAL;
  if (ws_bytes < need) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* taps = (uint32_t*)ws;
  if (spot_cap > 0 && hipMemsetAsync(spots, 0, (size_t)spot_cap * sizeof(MsegSpot), st) != hipSuccess) return MSEG_ELAUNCH;
  const int64_t n_cell = (int64_t)C * n_labels, n_bg = (int64_t)T * C;
  int64_t items = n_cell > n_bg ? n_cell : n_bg;
  if (items < SP_NTAPS) items = SP_NTAPS;
  int64_t blocks = (items + SP_BLOCK - 1) / SP_BLOCK;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(sp_init_kernel, dim3((unsigned)blocks), dim3(SP_BLOCK), 0, st, taps, scale, cell_count, n_cell, bg_count,
                     n_bg, (u64*)n_spots, status);
  const int64_t thr = (int64_t)threshold << (8 * scale);              // thr * 16^(2s)
  cell_dispatch(label_dtype, img_dtype, [&](auto l, auto p) {
    sp_launch<decltype(l), decltype(p)>(scale, st, (unsigned)tiles, labels, T, H, W, label_off, n_labels, img, C, frame_stride,
                                        chan_stride, row_stride, pix_stride, thr, (const uint32_t*)taps, tiles_x, tiles_y,
                                        cell_count, bg_count, spots, spot_cap, (u64*)n_spots, status);
  });
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
