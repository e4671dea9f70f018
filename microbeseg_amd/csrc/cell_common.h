// cell_common.h — what the per-cell files share (cells, hull, midline, order_stats, profile, neighbors, spots, drift;
// DESIGN.md §6l): the eight-pixel loader, the rule that makes an id a cell of its frame, the walk of one wave over a cell's
// box, the pair table's hash and slot claim, and the opening checks and type dispatch of the entry points.  A new per-cell
// file takes these from here.
#pragma once
#include "common.h"

typedef unsigned long long u64;

inline size_t mseg_align256(size_t v) { return (v + 255) / 256 * 256; }
inline unsigned mseg_blocks(int64_t n, int block) { return (unsigned)((n + block - 1) / block < 1 ? 1 : (n + block - 1) / block); }

// ---- device ---------------------------------------------------------------------------------------------------------------
// Elements q0 .. q0 + 7 of an array of n; positions outside 0 .. n - 1 read as 0 ("not a cell").  One or two vector loads
// when all eight are inside and the address is aligned (16 bytes; 8 for uint8), scalar loads under a bounds test otherwise.
template <typename E>
__device__ __forceinline__ void cell_load8(const E* __restrict__ base, int64_t q0, int64_t n, int (&v)[8]) {
  const E* p = base + q0;
  if (q0 >= 0 && q0 + 8 <= n && ((uintptr_t)p & (sizeof(E) == 1 ? 7 : 15)) == 0) {
    if (sizeof(E) == 4) {
      const int4 a = *reinterpret_cast<const int4*>(p), b = *reinterpret_cast<const int4*>(p + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else if (sizeof(E) == 2) {
      const uint4 a = *reinterpret_cast<const uint4*>(p);
      v[0] = a.x & 0xFFFF; v[1] = a.x >> 16; v[2] = a.y & 0xFFFF; v[3] = a.y >> 16;
      v[4] = a.z & 0xFFFF; v[5] = a.z >> 16; v[6] = a.w & 0xFFFF; v[7] = a.w >> 16;
    } else {
      const uint2 a = *reinterpret_cast<const uint2*>(p);
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[k] = (a.x >> (8 * k)) & 0xFF; v[4 + k] = (a.y >> (8 * k)) & 0xFF; }
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t q = q0 + k;
    v[k] = (q >= 0 && q < n) ? (int)base[q] : 0;
  }
}

// an id is a cell of its frame only if the frame's table of K entries holds it; everything else is 0
__device__ __forceinline__ int cell_id(int v, int64_t K) { return (v > 0 && (int64_t)v <= K) ? v : 0; }

// ---- one wave per cell slot (order_stats, profile) ------------------------------------------------------------------------
#define CELL_WAVE 64

// the frame of slot s: the last t with loff[t] <= s
__device__ __forceinline__ int cell_slot_frame(const int64_t* __restrict__ loff, int T, int64_t s) {
  int lo_t = 0, hi_t = T;
  while (hi_t - lo_t > 1) {
    const int mid = (lo_t + hi_t) >> 1;
    if (loff[mid] <= s) lo_t = mid; else hi_t = mid;
  }
  return lo_t;
}

// A cell's box (r0, c0, r1, c1, half-open), clipped to the frame: no read leaves the arrays, whatever the box says.  An
// all-zero box (an absent cell) and a label that is no id have no elements.
struct CellWalk {
  int r0, c0, bw, cells;          // the first row and column, the width, the elements of the clipped box
  int lbl;                        // the cell's id in its frame
  int qy, qx;                     // 64 elements on in flat order: qy rows and qx columns
};

__device__ __forceinline__ CellWalk cell_walk_box(int4 bb, int H, int W, int64_t l64) {
  CellWalk k;
  k.r0 = max(bb.x, 0); k.c0 = max(bb.y, 0);
  const int r1 = min(bb.z, H), c1 = min(bb.w, W);
  k.bw = c1 > k.c0 ? c1 - k.c0 : 0;
  const int bh = r1 > k.r0 ? r1 - k.r0 : 0;
  k.cells = (l64 >= 1 && l64 <= 0x7FFFFFFFll) ? k.bw * bh : 0;              // bw * bh <= H * W < 2^31 - 512
  k.lbl = (int)l64;
  k.qy = k.bw ? CELL_WAVE / k.bw : 0; k.qx = k.bw ? CELL_WAVE % k.bw : 0;
  return k;
}

// The wave walks the box in flat order (lane i takes element i, i + 64, ... of the box, so consecutive lanes take
// consecutive columns and run on into the next row: a box narrower than the wave leaves no lane idle) and calls f(y, x)
// for every pixel of the cell, in frame coordinates.
template <typename L, typename F>
__device__ __forceinline__ void cell_walk(const L* __restrict__ frame, int W, const CellWalk& k, int lane, F&& f) {
  int y = k.bw ? lane / k.bw : 0, x = k.bw ? lane % k.bw : 0;
  for (int i = lane; i < k.cells; i += CELL_WAVE) {
    if ((int)frame[(int64_t)(k.r0 + y) * W + k.c0 + x] == k.lbl && (sizeof(L) == 4 || k.lbl <= 0xFFFF)) f(k.r0 + y, k.c0 + x);
    y += k.qy; x += k.qx;
    if (x >= k.bw) { x -= k.bw; ++y; }
  }
}

__device__ __forceinline__ uint32_t cell_pair_hash(uint32_t a, uint32_t b) {
  uint32_t h = a * 0x9E3779B1u ^ b * 0x85EBCA77u;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 13;
  return h;
}

// The slot of the pair (a, b) in an open-addressing table of mask + 1 keys (a << 32 | b, 0 = empty), claimed if new;
// mask + 1: the table is full, and status says so.  BAIL: a long probe looks at the status word every 32 steps and gives up
// once another lane found the table full: the caller redoes the frame anyway, and walking a full table to its end for every
// further pair would take longer than the redo.
template <bool BAIL>
__device__ __forceinline__ uint32_t cell_pair_slot(u64* __restrict__ keys, uint32_t mask, uint32_t a, uint32_t b,
                                                   int32_t* __restrict__ status) {
  const u64 key = (u64)a << 32 | b;
  uint32_t h = cell_pair_hash(a, b) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    u64 k = keys[h];
    if (k == 0) k = atomicCAS(&keys[h], 0ull, key);
    if (k == 0 || k == key) return h;
    if (BAIL && (probe & 31) == 31 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
      return mask + 1;
    h = (h + 1) & mask;
  }
  atomicOr(status, 1);
  return mask + 1;
}

// ---- host: the opening checks and the type dispatch of an entry point --------------------------------------------------------
// the label stack; margin: what a kernel's index arithmetic adds to H * W at most (512, or the file's chunk)
inline bool cell_stack_ok(const void* labels, const int64_t* label_off, int label_dtype, int T, int H, int W, int margin) {
  return labels && label_off && T > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) - margin &&
         (label_dtype == MSEG_PIX_U16 || label_dtype == MSEG_PIX_I32);
}

inline bool cell_image_ok(int img_dtype) { return img_dtype == MSEG_PIX_U8 || img_dtype == MSEG_PIX_U16; }

// f(L()) with L = the label type of a checked dtype; f(L(), P()) with P = the pixel type of a checked image dtype as well
template <typename F>
inline void cell_dispatch(int label_dtype, F&& f) {
  if (label_dtype == MSEG_PIX_U16) f(uint16_t()); else f(int32_t());
}
template <typename F>
inline void cell_dispatch(int label_dtype, int img_dtype, F&& f) {
  cell_dispatch(label_dtype, [&](auto l) {
    if (img_dtype == MSEG_PIX_U8) f(l, uint8_t()); else f(l, uint16_t());
  });
}
