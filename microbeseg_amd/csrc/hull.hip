// hull.hip — per-cell outline measures of a segmented stack: crack perimeter, convex hull, largest and smallest caliper
// (DESIGN.md §6p).  An extension of the per-cell table (cells.hip, §6l).
//
// A cell is the union of the closed unit squares of its pixels; its corners are integer points in 0..H x 0..W.
//   ch_label_kernel  labels [T][H][W], read once: per cell the number of exposed unit edges, and per corner row of the cell
//                    the smallest and the largest corner column (the row extents), by int32 atomicMin / atomicMax
//   ch_hull_kernel   one wave per cell: the two monotone chains over the row extents, then shoelace, the farthest vertex
//                    pair and the smallest width over the hull edges, spread over the lanes
// Integers only, order-free atomics: bit-identical from run to run.
#include "cell_common.h"

#define CH_BLOCK 256
#define CH_WAVES (CH_BLOCK / 64)
#define CH_PPL 8                  // consecutive pixels per lane: 16 bytes of uint16 labels, two loads of int32

namespace {

typedef unsigned __int128 u128;

struct ChWs {
  int32_t* xmin;      // [n_rows]  smallest corner column of a corner row, INT32_MAX: the cell has no pixel beside the row
  int32_t* xmax;      // [n_rows]  largest corner column, INT32_MIN likewise
  int2* hv;           // [2 * n_rows]  per cell the left chain (rows of the cell entries), then the right chain
};

inline ChWs ch_carve(void* ws, int64_t n_rows) {
  const size_t r = (size_t)(n_rows > 0 ? n_rows : 1);
  char* b = (char*)ws;
  ChWs w;
  w.xmin = (int32_t*)b;
  w.xmax = (int32_t*)(b + mseg_align256(r * sizeof(int32_t)));
  w.hv = (int2*)(b + 2 * mseg_align256(r * sizeof(int32_t)));
  return w;
}

// ---- a. label pass ------------------------------------------------------------------------------------------------------
// A lane owns 8 consecutive pixels of a frame (flat order, so the loads are aligned whenever the frame is).  Its left and
// right neighbours are the pixels before and after the 8, the upper and lower ones the same 8 positions one row up / down:
// the neighbouring lanes' and rows' loads, served from cache.  A pixel whose left (right) neighbour is not of its cell is a
// run end: it lowers xmin (raises xmax) of the two corner rows it touches.  Exposed edges are counted in a register and
// added once per stretch of one label.
template <typename L>
__global__ void __launch_bounds__(CH_BLOCK) ch_label_kernel(const L* __restrict__ lab, int T, int H, int W,
                                                            const int64_t* __restrict__ loff,
                                                            const int32_t* __restrict__ bbox,
                                                            const int64_t* __restrict__ row_off, int64_t n_rows,
                                                            int32_t* __restrict__ xmin, int32_t* __restrict__ xmax,
                                                            u64* __restrict__ perim, int32_t* __restrict__ status) {
  const int HW = H * W;
  const int64_t groups = ((int64_t)HW + CH_PPL - 1) / CH_PPL;
  const int64_t g = (int64_t)blockIdx.x * CH_BLOCK + threadIdx.x;
  if (g >= (int64_t)T * groups) return;
  const int t = (int)(g / groups);
  const int p0 = (int)(g - (int64_t)t * groups) * CH_PPL;
  const int64_t base = loff[t], K = loff[t + 1] - base;
  const L* frame = lab + (int64_t)t * HW;
  int e[CH_PPL], up[CH_PPL], dn[CH_PPL];
  cell_load8<L>(frame, p0, HW, e);
  bool any = false;
#pragma unroll
  for (int k = 0; k < CH_PPL; ++k) {
    e[k] = cell_id(e[k], K);
    any |= e[k] > 0;
  }
  if (!any) return;
  cell_load8<L>(frame, (int64_t)p0 - W, HW, up);     // outside the frame: 0, not a cell
  cell_load8<L>(frame, (int64_t)p0 + W, HW, dn);
  const int el = cell_id(p0 > 0 ? (int)frame[p0 - 1] : 0, K), er = cell_id(p0 + CH_PPL < HW ? (int)frame[p0 + CH_PPL] : 0, K);
  int y = p0 / W, x = p0 - y * W;
  int cur = 0;
  unsigned cnt = 0;
#pragma unroll
  for (int k = 0; k < CH_PPL; ++k) {
    const int l = e[k];
    if (l != cur) {
      if (cur > 0 && cnt) atomicAdd(&perim[base + cur - 1], (u64)cnt);
      cur = l;
      cnt = 0;
    }
    if (l > 0) {
      const int u = cell_id(up[k], K), d = cell_id(dn[k], K);
      const int lf = x > 0 ? (k > 0 ? e[k > 0 ? k - 1 : 0] : el) : 0;
      const int rt = x < W - 1 ? (k < CH_PPL - 1 ? e[k < CH_PPL - 1 ? k + 1 : k] : er) : 0;
      const bool open_l = lf != l, open_r = rt != l;
      cnt += (unsigned)open_l + (unsigned)open_r + (unsigned)(u != l) + (unsigned)(d != l);
      if (open_l || open_r) {
        const int64_t s = base + l - 1;
        const int32_t* bp = bbox + 4 * s;
        const int4 bb = make_int4(bp[0], bp[1], bp[2], bp[3]);             // r0, c0, r1, c1
        const int64_t ro = row_off[s], nr = row_off[s + 1] - ro;
        const int64_t rel = (int64_t)y - bb.x;
        // inside the box given for the cell, and both corner rows inside the cell's own rows of the workspace
        if (y >= bb.x && y < bb.z && x >= bb.y && x < bb.w && ro >= 0 && rel + 1 < nr && ro + nr <= n_rows) {
          if (open_l) { atomicMin(&xmin[ro + rel], x); atomicMin(&xmin[ro + rel + 1], x); }
          if (open_r) { atomicMax(&xmax[ro + rel], x + 1); atomicMax(&xmax[ro + rel + 1], x + 1); }
        } else {
          atomicOr(status, 1);
        }
      }
    }
    if (++x == W) { x = 0; ++y; }
  }
  if (cur > 0 && cnt) atomicAdd(&perim[base + cur - 1], (u64)cnt);
}

__global__ void ch_init_kernel(int32_t* __restrict__ xmin, int32_t* __restrict__ xmax, int64_t n_rows,
                               int64_t* __restrict__ out, int64_t n, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_rows) { xmin[i] = INT32_MAX; xmax[i] = INT32_MIN; }
  if (i < n) out[i] = 0;                       // plane 0, the perimeter, is accumulated; the hull pass writes planes 1 .. 9
  if (i == 0) status[0] = 0;
}

// ---- b. hull pass -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t ch_cross(int2 o, int2 a, int2 b) {
  return (int64_t)(a.x - o.x) * (int64_t)(b.y - o.y) - (int64_t)(a.y - o.y) * (int64_t)(b.x - o.x);
}

__device__ __forceinline__ uint32_t ch_gcd(uint32_t a, uint32_t b) {
  while (b) { const uint32_t r = a % b; a = b; b = r; }
  return a;
}

// (y, x) order of two points
__device__ __forceinline__ bool ch_less(int2 a, int2 b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

struct ChPair {                   // farthest pair: a < b in (y, x) order; d2 < 0: none yet
  long long d2;
  int2 a, b;                      // .x = y, .y = x (see ch_hull_kernel)
};
__device__ __forceinline__ bool ch_pair_better(const ChPair& p, const ChPair& q) {      // p before q
  if (p.d2 != q.d2) return p.d2 > q.d2;
  if (p.a.x != q.a.x || p.a.y != q.a.y) return ch_less(p.a, q.a);
  return ch_less(p.b, q.b);
}
// width num / sqrt(den2); den2 == 0: none yet.  num < 2^32, den2 < 2^63, so num^2 * den2' < 2^127
__device__ __forceinline__ bool ch_width_better(u64 pn, u64 pd, u64 qn, u64 qd) {
  if (qd == 0) return pd != 0;
  if (pd == 0) return false;
  const u128 lhs = (u128)(pn * pn) * qd, rhs = (u128)(qn * qn) * pd;
  return lhs != rhs ? lhs < rhs : pd < qd;
}

// One wave per cell slot.  Points are int2 with .x = row (y) and .y = column (x).  Lane 0 scans the left chain (the
// (row, xmin) points, top to bottom, kept while the boundary turns left), lane 1 the right chain; each keeps its stack in
// the cell's piece of the workspace (a chain has at most one vertex per row), the top two entries in registers.  The hull
// is the left chain downwards followed by the right chain upwards: xmin < xmax on every row, so no vertex repeats, and
// the top and bottom sides are horizontal, so their ends are strict vertices.  Then lane i takes hull edge i, i + 64, ...
// against every vertex: shoelace term, largest squared distance from the edge's first vertex, largest |cross| against the
// edge's line; butterflies fold the lanes.
__global__ void __launch_bounds__(CH_BLOCK) ch_hull_kernel(const int32_t* __restrict__ bbox,
                                                           const int64_t* __restrict__ row_off, int64_t n, int64_t n_rows,
                                                           const int32_t* __restrict__ xmin,
                                                           const int32_t* __restrict__ xmax, int2* __restrict__ hv,
                                                           int64_t* __restrict__ out, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t s = ((int64_t)blockIdx.x * CH_BLOCK + threadIdx.x) >> 6;
  if (s >= n) return;                                               // wave-uniform
  int64_t ro = row_off[s], nr = row_off[s + 1] - ro;
  const int r0 = bbox[4 * s];
  if (ro < 0 || nr < 0 || ro + nr > n_rows) {                       // rows that are not inside the workspace: touch none
    if (lane == 0) atomicOr(status, 1);
    ro = 0; nr = 0;
  }
  int2* chain = hv + 2 * ro + (lane == 1 ? nr : 0);
  int64_t sp = 0;
  if (lane < 2 && nr >= 2) {
    const int32_t* ext = lane ? xmax : xmin;
    const int32_t none = lane ? INT32_MIN : INT32_MAX;
    const int64_t sgn = lane ? -1 : 1;
    int2 top = make_int2(0, 0), sec = make_int2(0, 0);
    for (int64_t i = 0; i < nr; ++i) {
      const int32_t xv = ext[ro + i];
      if (xv == none) continue;                                     // no pixel of the cell beside this corner row
      const int2 p = make_int2((int)(r0 + i), xv);
      while (sp >= 2) {
        // left chain: the middle point stays while it lies strictly left of the chord (smaller column); right: mirrored
        if (sgn * ch_cross(sec, top, p) > 0) break;
        --sp;
        top = sec;
        if (sp >= 2) sec = chain[sp - 2];
      }
      chain[sp] = p;
      sec = top;
      top = p;
      ++sp;
    }
  }
  __threadfence();                                                  // the chains are read by all lanes below
  const int64_t nl = __shfl(sp, 0, 64), nrt = __shfl(sp, 1, 64), k = nl + nrt;
  if (nl < 2 || nrt < 2) {                                          // an absent cell (or one whose pixels were all refused)
    if (lane >= 1 && lane < 10) out[(int64_t)lane * n + s] = 0;
    return;
  }
  const int2* lc = hv + 2 * ro;
  const int2* rc = lc + nr;
#define CH_V(i) ((i) < nl ? lc[(i)] : rc[k - 1 - (i)])
  const int2 v0 = lc[0];
  long long area = 0;
  ChPair best;
  best.d2 = -1; best.a = v0; best.b = v0;
  u64 wn = 0, wd = 0;
  for (int64_t i = lane; i < k; i += 64) {
    const int2 a = CH_V(i), b = CH_V(i + 1 == k ? 0 : i + 1);
    area += ch_cross(v0, a, b);
    const int64_t ey = b.x - a.x, ex = b.y - a.y;
    u64 mc = 0;
    for (int64_t j = 0; j < k; ++j) {
      const int2 v = CH_V(j);
      const int64_t dy = v.x - a.x, dx = v.y - a.y;
      const int64_t c = ey * dx - ex * dy;
      const u64 ac = (u64)(c < 0 ? -c : c);
      mc = ac > mc ? ac : mc;
      ChPair q;
      q.d2 = dy * dy + dx * dx;
      if (j != i && q.d2 >= best.d2) {
        const bool a_first = ch_less(a, v);
        q.a = a_first ? a : v;
        q.b = a_first ? v : a;
        if (ch_pair_better(q, best)) best = q;
      }
    }
    // the direction alone decides the pair: the edge over its gcd.  |cross| < 2 H W < 2^32 and |ey|, |ex| < 2^31
    const uint32_t g = ch_gcd((uint32_t)(ey < 0 ? -ey : ey), (uint32_t)(ex < 0 ? -ex : ex));
    if (g == 0) continue;
    const int64_t ny = (int32_t)ey / (int32_t)g, nx = (int32_t)ex / (int32_t)g;
    const u64 num = (uint32_t)mc / g, den2 = (u64)(ny * ny + nx * nx);
    if (ch_width_better(num, den2, wn, wd)) { wn = num; wd = den2; }
  }
#undef CH_V
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    area += __shfl_xor(area, d, 64);
    ChPair q;
    q.d2 = __shfl_xor(best.d2, d, 64);
    q.a.x = __shfl_xor(best.a.x, d, 64); q.a.y = __shfl_xor(best.a.y, d, 64);
    q.b.x = __shfl_xor(best.b.x, d, 64); q.b.y = __shfl_xor(best.b.y, d, 64);
    if (ch_pair_better(q, best)) best = q;
    const u64 qn = __shfl_xor(wn, d, 64), qd = __shfl_xor(wd, d, 64);
    if (ch_width_better(qn, qd, wn, wd)) { wn = qn; wd = qd; }
  }
  if (lane == 0) {
    out[1 * n + s] = k;
    out[2 * n + s] = area < 0 ? -area : area;
    out[3 * n + s] = best.d2;
    out[4 * n + s] = best.a.x;
    out[5 * n + s] = best.a.y;
    out[6 * n + s] = best.b.x;
    out[7 * n + s] = best.b.y;
    out[8 * n + s] = (int64_t)wn;
    out[9 * n + s] = (int64_t)wd;
  }
}

}  // namespace

// ---- entry points -------------------------------------------------------------------------------------------------------
extern "C" size_t mseg_cell_hull_workspace_bytes(int64_t n_labels, int64_t n_rows) {
  if (n_labels < 0 || n_rows < 0 || n_rows > (1ll << 40)) return 0;
  const size_t r = (size_t)(n_rows > 0 ? n_rows : 1);
  return 2 * mseg_align256(r * sizeof(int32_t)) + mseg_align256(2 * r * sizeof(int2));
}

extern "C" int mseg_cell_hull(const void* labels, int dtype, int T, int H, int W, const int64_t* label_off,
                              int64_t n_labels, const int32_t* bbox, const int64_t* row_off, int64_t n_rows, int64_t* out,
                              int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!cell_stack_ok(labels, label_off, dtype, T, H, W, 512) || !status || !ws || n_labels < 0 || n_rows < 0) return MSEG_EINVAL;
  if (n_labels > 0 && (!bbox || !row_off || !out)) return MSEG_EINVAL;
  const size_t need = mseg_cell_hull_workspace_bytes(n_labels, n_rows);
  if (need == 0) return MSEG_EINVAL;
  const int64_t lanes = (int64_t)T * (((int64_t)H * W + CH_PPL - 1) / CH_PPL);
  if ((lanes + CH_BLOCK - 1) / CH_BLOCK > 0x7FFFFFFFll || (n_labels + CH_WAVES - 1) / CH_WAVES > 0x7FFFFFFFll) return MSEG_EINVAL;
  if (ws_bytes < need) return MSEG_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (n_labels == 0) {                                              // no cell, no kernel: the status word alone is written
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return MSEG_ELAUNCH;
    return MSEG_OK;
  }
  const ChWs w = ch_carve(ws, n_rows);
  const int64_t items = n_rows > n_labels ? n_rows : n_labels;
  const dim3 block(CH_BLOCK);
  hipLaunchKernelGGL(ch_init_kernel, dim3(mseg_blocks(items, CH_BLOCK)), block, 0, st, w.xmin, w.xmax, n_rows, out, n_labels,
                     status);
  cell_dispatch(dtype, [&](auto l) {
    typedef decltype(l) L;
    hipLaunchKernelGGL(ch_label_kernel<L>, dim3(mseg_blocks(lanes, CH_BLOCK)), block, 0, st, (const L*)labels, T, H, W,
                       label_off, bbox, row_off, n_rows, w.xmin, w.xmax, (u64*)out, status);
  });
  hipLaunchKernelGGL(ch_hull_kernel, dim3(mseg_blocks(n_labels * 64, CH_BLOCK)), block, 0, st, bbox, row_off, n_labels, n_rows,
                     (const int32_t*)w.xmin, (const int32_t*)w.xmax, w.hv, out, status);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}
