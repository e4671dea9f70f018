// neighbors.hip — the per-cell neighbourhood of a segmented stack: contact edges, touching cells, nearest neighbour within a
// radius, and the contact graph.  An extension of the per-cell table (cells.hip, §6l).
//
// Within one frame, for two cells a < b: edges(a, b) = unit pixel edges between them, d2(a, b) = the smallest squared
// distance between the centres of a pixel of a and a pixel of b; the pair exists when d2 <= R^2.
//   nb_tile_kernel    one workgroup per 32 x 64 tile, the sanitised labels of the tile and its halo (one row above, R rows
//                     below, R columns on either side) in LDS: per cell pixel the contact / border / free edges, shared
//                     right and lower edges into the frame's pair table, and the boundary pixels of the tile into a list;
//                     then the listed pixels scan their half window (dy > 0, or dy == 0 and dx > 0) for the pairs' d2
//   nb_table_kernel   one thread per table entry: the per-cell counts, nearest neighbour and main contact, the pair rows
//   nb_finish_kernel  one thread per cell: unpacks the two packed planes
// Integers only, order-free integer atomics: bit-identical from run to run (the order of the pair rows aside).
#include "cell_common.h"

#define NB_BLOCK 256
#define NB_TH 32                  // tile rows
#define NB_TW 64                  // tile columns
#define NB_PPL 8                  // consecutive pixels of one tile row per lane: NB_TW / NB_PPL lanes per row
#define NB_MAX_R 32
#define NB_MIN_CAP 64
#define NB_CACHE 4                // neighbour ids a scanning lane keeps the best d2 of in registers

namespace {

struct NbWs {
  u64* keys;          // [T][cap]  a << 32 | b with a < b, 0 = empty
  uint32_t* edges;    // [T][cap]
  uint32_t* d2;       // [T][cap]  all ones = none yet
  u64* nn;            // [n]       min of d2 << 32 | label, all ones = none
  u64* best;          // [n]       max of edges << 32 | ~label, 0 = none
};

inline NbWs nb_carve(void* ws, int T, int64_t n, int64_t cap) {
  const size_t entries = (size_t)T * (size_t)cap;
  char* b = (char*)ws;
  NbWs w;
  w.keys = (u64*)b;
  b += mseg_align256(entries * sizeof(u64));
  w.edges = (uint32_t*)b;
  b += mseg_align256(entries * sizeof(uint32_t));
  w.d2 = (uint32_t*)b;
  b += mseg_align256(entries * sizeof(uint32_t));
  w.nn = (u64*)b;
  b += mseg_align256((size_t)(n + 1) * sizeof(u64));
  w.best = (u64*)b;
  return w;
}

__global__ void nb_init_kernel(NbWs w, int64_t entries, int64_t n, int64_t* __restrict__ out, int32_t* __restrict__ status,
                               int T, int64_t* __restrict__ n_pairs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < entries) { w.keys[i] = 0; w.edges[i] = 0; w.d2[i] = 0xFFFFFFFFu; }
  if (i < n) {
    w.nn[i] = ~0ull;
    w.best[i] = 0;
#pragma unroll
    for (int p = 0; p < 9; ++p) out[(int64_t)p * n + i] = 0;
  }
  if (i < T) status[i] = 0;
  if (i == 0) n_pairs[0] = 0;
}

struct NbTable {
  u64* keys;
  uint32_t* edges;
  uint32_t* d2;
  uint32_t mask;
  int32_t* status;
};

// a pair's entry in the frame's table: the slot of (the smaller, the larger id); a lane gives up early on a full table
__device__ __forceinline__ void nb_add_edges(const NbTable& tb, int a, int b, uint32_t len) {
  const uint32_t lo = (uint32_t)min(a, b), hi = (uint32_t)max(a, b);
  const uint32_t h = cell_pair_slot<true>(tb.keys, tb.mask, lo, hi, tb.status);
  if (h <= tb.mask) atomicAdd(&tb.edges[h], len);
}

// d2 only ever falls, so a value read earlier is an upper bound of the entry: a candidate that does not beat it is dropped
__device__ __forceinline__ void nb_min_d2(const NbTable& tb, int a, int b, uint32_t d2) {
  const uint32_t lo = (uint32_t)min(a, b), hi = (uint32_t)max(a, b);
  const uint32_t h = cell_pair_slot<true>(tb.keys, tb.mask, lo, hi, tb.status);
  if (h <= tb.mask && tb.d2[h] > d2) atomicMin(&tb.d2[h], d2);
}

// LDS: the tile of labels (dynamic, E = uint16_t for uint16 stacks, int32_t for int32 ones; ids that are not a cell and
// positions outside the frame hold 0), the list of the tile's boundary pixels, the half widths of the disc per row.
template <typename L, typename E>
__global__ void __launch_bounds__(NB_BLOCK) nb_tile_kernel(const L* __restrict__ lab, int H, int W, int tiles_x, int tiles_y,
                                                           const int64_t* __restrict__ loff, int R, NbWs w, uint32_t cap,
                                                           u64* __restrict__ out, int64_t n, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nb_smem[];
  __shared__ uint16_t list[NB_TH * NB_TW];
  __shared__ int xlim[NB_MAX_R + 1];
  __shared__ unsigned n_list;
  E* tile = reinterpret_cast<E*>(nb_smem);
  const int LR = NB_TH + R + 1, LC = NB_TW + 2 * R;
  const int tid = threadIdx.x;
  const int per_frame = tiles_x * tiles_y;
  const int t = (int)(blockIdx.x / (unsigned)per_frame);
  const int in_frame = (int)(blockIdx.x - (unsigned)t * (unsigned)per_frame);
  const int y0 = (in_frame / tiles_x) * NB_TH, x0 = (in_frame % tiles_x) * NB_TW;
  const int64_t base = loff[t], K = loff[t + 1] - base;
  const L* frame = lab + (int64_t)t * H * W;

  if (tid == 0) n_list = 0;
  if (tid <= R) {                                   // largest dx with dy^2 + dx^2 <= R^2
    int x = 0;
    while ((x + 1) * (x + 1) + tid * tid <= R * R) ++x;
    xlim[tid] = x;
  }
  for (int ly = tid >> 6; ly < LR; ly += NB_BLOCK / 64) {
    const int gy = y0 - 1 + ly;
    const bool row_in = gy >= 0 && gy < H;
    const L* row = frame + (int64_t)(row_in ? gy : 0) * W;
    for (int lx = tid & 63; lx < LC; lx += 64) {
      const int gx = x0 - R + lx;
      int v = 0;
      if (row_in && gx >= 0 && gx < W) v = (int)row[gx];
      tile[ly * LC + lx] = (E)cell_id(v, K);
    }
  }
  __syncthreads();

  NbTable tb;
  tb.keys = w.keys + (size_t)t * cap;
  tb.edges = w.edges + (size_t)t * cap;
  tb.d2 = w.d2 + (size_t)t * cap;
  tb.mask = cap - 1;
  tb.status = status + t;

  // ---- a. pixel pass: the edges of the lane's 8 pixels ------------------------------------------------------------------
  {
    const int ry = tid / (NB_TW / NB_PPL), cx = (tid % (NB_TW / NB_PPL)) * NB_PPL;
    const int y = y0 + ry;
    const int c0 = (ry + 1) * LC + R + cx;
    int cur = 0, pa = 0, pb = 0;
    uint32_t cc = 0, cb = 0, cf = 0, plen = 0, bmask = 0;
#pragma unroll
    for (int k = 0; k < NB_PPL; ++k) {
      const int c = c0 + k, x = x0 + cx + k;
      const int a = (int)tile[c];                  // 0 beyond the frame's last row / column
      if (a != cur) {
        if (cur > 0) {
          const int64_t s = base + cur - 1;
          if (cc) atomicAdd(&out[s], (u64)cc);
          if (cb) atomicAdd(&out[n + s], (u64)cb);
          if (cf) atomicAdd(&out[2 * n + s], (u64)cf);
        }
        cur = a; cc = cb = cf = 0;
      }
      bool ok = false;
      int na = 0, nb = 0;
      if (a > 0) {
        const int l = (int)tile[c - 1], r = (int)tile[c + 1], u = (int)tile[c - LC], d = (int)tile[c + LC];
        const uint32_t border = (uint32_t)(x == 0) + (uint32_t)(x == W - 1) + (uint32_t)(y == 0) + (uint32_t)(y == H - 1);
        const uint32_t zero = (uint32_t)(l == 0) + (uint32_t)(r == 0) + (uint32_t)(u == 0) + (uint32_t)(d == 0);
        const uint32_t other = (uint32_t)(l != 0 && l != a) + (uint32_t)(r != 0 && r != a) + (uint32_t)(u != 0 && u != a) +
                               (uint32_t)(d != 0 && d != a);
        cb += border;
        cf += zero - border;                       // the outside of the frame reads as 0
        cc += other;
        if (zero + other) bmask |= 1u << k;
        if (r != 0 && r != a) nb_add_edges(tb, a, r, 1);
        ok = d != 0 && d != a;
        na = min(a, d); nb = max(a, d);
      }
      if (plen && (!ok || na != pa || nb != pb)) { nb_add_edges(tb, pa, pb, plen); plen = 0; }
      if (ok) { pa = na; pb = nb; ++plen; }
    }
    if (plen) nb_add_edges(tb, pa, pb, plen);
    if (cur > 0) {
      const int64_t s = base + cur - 1;
      if (cc) atomicAdd(&out[s], (u64)cc);
      if (cb) atomicAdd(&out[n + s], (u64)cb);
      if (cf) atomicAdd(&out[2 * n + s], (u64)cf);
    }
    if (bmask) {
      unsigned at = atomicAdd(&n_list, (unsigned)__popc(bmask));
#pragma unroll
      for (int k = 0; k < NB_PPL; ++k)
        if (bmask >> k & 1) list[at++] = (uint16_t)(c0 + k);
    }
  }
  __syncthreads();

  // ---- b. window scan: every boundary pixel of the tile against the half window below and to the right of it --------------
  const unsigned count = n_list;
  for (unsigned i = tid; i < count; i += NB_BLOCK) {
    const int c = list[i];
    const int ly = c / LC;
    const int a = (int)tile[c];
    const int rows = min(R, H - 1 - (y0 - 1 + ly));          // rows of the window inside the frame
    int last = 0, slot = 0;
    uint32_t last_d2 = 0;
    int cid[NB_CACHE];
    uint32_t cd2[NB_CACHE];
#pragma unroll
    for (int j = 0; j < NB_CACHE; ++j) { cid[j] = 0; cd2[j] = 0; }
    for (int dy = 0; dy <= rows; ++dy) {
      const int xr = xlim[dy];
      const E* row = tile + c + dy * LC;
      for (int dx = dy ? -xr : 1; dx <= xr; ++dx) {
        const int b = (int)row[dx];
        if (b == 0 || b == a) continue;
        const uint32_t d2 = (uint32_t)(dy * dy + dx * dx);
        if (b == last) { last_d2 = min(last_d2, d2); continue; }
        if (last) {                                // the run of `last` ends: into the lane's cache, evicting round robin
          bool hit = false;
#pragma unroll
          for (int j = 0; j < NB_CACHE; ++j)
            if (cid[j] == last) { cd2[j] = min(cd2[j], last_d2); hit = true; }
          if (!hit) {
#pragma unroll
            for (int j = 0; j < NB_CACHE; ++j)
              if (j == slot) {
                if (cid[j]) nb_min_d2(tb, a, cid[j], cd2[j]);
                cid[j] = last; cd2[j] = last_d2;
              }
            slot = (slot + 1) % NB_CACHE;
          }
        }
        last = b; last_d2 = d2;
      }
    }
    if (last) {
      bool hit = false;
#pragma unroll
      for (int j = 0; j < NB_CACHE; ++j)
        if (cid[j] == last) { cd2[j] = min(cd2[j], last_d2); hit = true; }
      if (!hit) nb_min_d2(tb, a, last, last_d2);
    }
#pragma unroll
    for (int j = 0; j < NB_CACHE; ++j)
      if (cid[j]) nb_min_d2(tb, a, cid[j], cd2[j]);
  }
}

// every table entry: the counts of its two cells, their nearest neighbour (min of d2 << 32 | label: ties to the smallest
// label) and main contact (max of edges << 32 | ~label: ties to the smallest label), and one pair row
__global__ void nb_table_kernel(NbWs w, int64_t entries, int cap_shift, const int64_t* __restrict__ loff,
                                u64* __restrict__ out, int64_t n, int32_t* __restrict__ pairs, int64_t pair_cap,
                                u64* __restrict__ n_pairs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= entries) return;
  const u64 k = w.keys[i];
  if (k == 0) return;
  const int t = (int)(i >> cap_shift);
  const uint32_t a = (uint32_t)(k >> 32), b = (uint32_t)k, e = w.edges[i], d = w.d2[i];
  const int64_t sa = loff[t] + a - 1, sb = loff[t] + b - 1;
  atomicAdd(&out[4 * n + sa], 1ull);
  atomicAdd(&out[4 * n + sb], 1ull);
  atomicMin(&w.nn[sa], (u64)d << 32 | b);
  atomicMin(&w.nn[sb], (u64)d << 32 | a);
  if (e) {
    atomicAdd(&out[3 * n + sa], 1ull);
    atomicAdd(&out[3 * n + sb], 1ull);
    atomicMax(&w.best[sa], (u64)e << 32 | (uint32_t)~b);
    atomicMax(&w.best[sb], (u64)e << 32 | (uint32_t)~a);
  }
  const u64 row = atomicAdd(n_pairs, 1ull);
  if (row < (u64)pair_cap) {
    int32_t* p = pairs + 5 * row;
    p[0] = t; p[1] = (int32_t)a; p[2] = (int32_t)b; p[3] = (int32_t)e; p[4] = (int32_t)d;
  }
}

__global__ void nb_finish_kernel(NbWs w, int64_t n, int64_t* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const u64 nn = w.nn[s], best = w.best[s];
  const bool near = nn != ~0ull;
  out[5 * n + s] = near ? (int64_t)(uint32_t)nn : 0;
  out[6 * n + s] = near ? (int64_t)(nn >> 32) : 0;
  out[7 * n + s] = best ? (int64_t)(uint32_t)~(uint32_t)best : 0;
  out[8 * n + s] = (int64_t)(best >> 32);
}

}  // namespace

// ---- entry points -------------------------------------------------------------------------------------------------------
extern "C" size_t mseg_cell_neighbors_workspace_bytes(int T, int64_t n_labels, int64_t table_cap) {
  if (T <= 0 || n_labels < 0 || table_cap < NB_MIN_CAP || table_cap > (1ll << 31) || (table_cap & (table_cap - 1))) return 0;
  if ((int64_t)T * table_cap > (1ll << 40)) return 0;
  const size_t entries = (size_t)T * (size_t)table_cap;
  return mseg_align256(entries * sizeof(u64)) + 2 * mseg_align256(entries * sizeof(uint32_t)) +
         2 * mseg_align256((size_t)(n_labels + 1) * sizeof(u64));
}

extern "C" int mseg_cell_neighbors(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off,
                                   int64_t n_labels, int radius, int64_t table_cap, int64_t* out, int32_t* pairs,
                                   int64_t pair_cap, int64_t* n_pairs, int32_t* status, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (!cell_stack_ok(labels, label_off, dtype, T, H, W, 512) || !status || !n_pairs || !ws || n_labels < 0) return MSEG_EINVAL;
  if (radius < 1 || radius > NB_MAX_R) return MSEG_EINVAL;
  if (pair_cap < 0 || (pair_cap > 0 && !pairs) || pair_cap > (1ll << 40)) return MSEG_EINVAL;
  if (n_labels > 0 && !out) return MSEG_EINVAL;
  const size_t need = mseg_cell_neighbors_workspace_bytes(T, n_labels, table_cap);
  if (need == 0) return MSEG_EINVAL;
  const int tiles_x = (W + NB_TW - 1) / NB_TW, tiles_y = (H + NB_TH - 1) / NB_TH;
  const int64_t tiles = (int64_t)T * tiles_x * tiles_y, entries = (int64_t)T * table_cap;
  if (tiles > 0x7FFFFFFFll || (entries + NB_BLOCK - 1) / NB_BLOCK > 0x7FFFFFFFll ||
      (n_labels + NB_BLOCK - 1) / NB_BLOCK > 0x7FFFFFFFll)
    return MSEG_EINVAL;
  if (ws_bytes < need) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (n_labels == 0) {                                              // no cell, no kernel: status and the count alone
    if (hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)T, st) != hipSuccess) return MSEG_ELAUNCH;
    if (hipMemsetAsync(n_pairs, 0, sizeof(int64_t), st) != hipSuccess) return MSEG_ELAUNCH;
    return MSEG_OK;
  }
  const NbWs w = nb_carve(ws, T, n_labels, table_cap);
  int64_t items = entries > n_labels ? entries : n_labels;
  if (T > items) items = T;
  hipLaunchKernelGGL(nb_init_kernel, dim3(mseg_blocks(items, NB_BLOCK)), dim3(NB_BLOCK), 0, st, w, entries, n_labels, out,
                     status, T, n_pairs);
  const size_t cells = (size_t)(NB_TH + radius + 1) * (size_t)(NB_TW + 2 * radius);
  const uint32_t cap = (uint32_t)table_cap;                         // 2^31 at most
  cell_dispatch(dtype, [&](auto l) {
    typedef decltype(l) L;                                          // the tile in LDS holds the labels' own type
    hipLaunchKernelGGL((nb_tile_kernel<L, L>), dim3((unsigned)tiles), dim3(NB_BLOCK), (cells * sizeof(L) + 15) / 16 * 16, st,
                       (const L*)labels, H, W, tiles_x, tiles_y, label_off, radius, w, cap, (u64*)out, n_labels, status);
  });
  int cap_shift = 0;
  while ((1ll << cap_shift) < table_cap) ++cap_shift;
  hipLaunchKernelGGL(nb_table_kernel, dim3(mseg_blocks(entries, NB_BLOCK)), dim3(NB_BLOCK), 0, st, w, entries, cap_shift, label_off,
                     (u64*)out, n_labels, pairs, pair_cap, (u64*)n_pairs);
  hipLaunchKernelGGL(nb_finish_kernel, dim3(mseg_blocks(n_labels, NB_BLOCK)), dim3(NB_BLOCK), 0, st, w, n_labels, out);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
