// resample.hip — inference at a chosen resolution: separable, anti-aliased linear resampling with
// pixel-centre alignment.  mseg_resample_frames turns raw frames into the scaled, normalised, padded network input;
// mseg_resample_planes maps predictions back to the frame's own grid.  The rule lives on the host
// (inference/resample.py axis_table): per output index a first source index, a tap count and `taps` fp32 weights.  The
// kernels compute no weights.
//
// One kernel body serves both entry points.  A workgroup of 256 threads owns a TW x TH tile of the (padded) output:
//   1. it reads first / count of the tile's first and last valid row and column: the source window [wy0, wy0 + wyn) x
//      [wx0, wx0 + wxn) (first and first + count do not decrease along an axis: validated on the host);
//   2. stages the tile's slice of both tables and the window in LDS (raw pixels are normalised on load), waves over rows,
//      lanes along the source row: whole lines of global memory;
//   3. filters along x into a second LDS buffer mid[wyn][TW]: lanes run along the window's ROWS, so a wave reads
//      win[r][k] with an odd row pitch (32 different banks) and the weights of its column as a broadcast;
//   4. filters along y into a register and stores: lanes run along the output row — mid is read along its rows, the
//      store is one line per wave.
// Accumulation: acc = fmaf(w_t, v_t, acc) from acc = 0, t ascending, x before y — a value depends on nothing but its
// own window and weights: not on the tile, the launch or the other frames of the launch.
//
// LDS: wyn * (wxn | 1) + wyn * (TW + 1) words of dynamic memory plus 4.4 KB of tables, at most 64 KB together.  The tile
// starts at 64 x 16 and is halved (x, then y, in turn) until the largest window of the call fits; the host has the
// tables, so the window sizes are exact, not estimated.
#include "common.h"

#define RS_THREADS 256
#define RS_MAX_TAPS 12
#define RS_TW_MAX 64
#define RS_TH_MAX 16
#define RS_LDS_BYTES 65536

struct RsAxis {
  const int32_t* first;
  const int32_t* count;
  const float* weight;
  int n_in, n_out, taps;
};

struct RsParams {
  const void* src;
  const uint32_t* minmax;      // [n][2] {~min, max}; raw dtypes only
  float* dst;
  long long sfs, scs, srs, sps;      // source strides in elements: frame, channel, row, pixel
  long long dfs, dcs, drs, dps;
  RsAxis y, x;
  int n, C, pad_top, pad_left;      // the output is (y.n_out + pad_top) x (x.n_out + pad_left); padding = -1
  int tw_log2, th_log2;             // tile
  int win_h, win_w, wpitch;         // capacity of the window buffer (rows, columns) and its row pitch (odd)
};

struct RsTables {                   // the tile's slice of both tables
  int xf[RS_TW_MAX], xc[RS_TW_MAX], yf[RS_TH_MAX], yc[RS_TH_MAX];
  float xw[RS_TW_MAX * RS_MAX_TAPS], yw[RS_TH_MAX * RS_MAX_TAPS];
};

template <int DT>
__device__ __forceinline__ float rs_load(const RsParams& p, long long off, float fmin, float frange) {
  if (DT == MSEG_PIX_F32) return reinterpret_cast<const float*>(p.src)[off];
  const unsigned v = DT == MSEG_PIX_U8 ? reinterpret_cast<const uint8_t*>(p.src)[off]
                                       : reinterpret_cast<const uint16_t*>(p.src)[off];
  return raw_frame_norm(v, fmin, frange);        // common.h: the value mseg_frames_normalize gives the pixel
}

// first / count of one output index relative to a window of `wn` elements starting at `w0`, kept inside the window
// whatever the device table holds (the host copy was validated; this keeps a mismatching device copy in bounds)
__device__ __forceinline__ void rs_tap_range(int first, int count, int taps, int w0, int wn, int& f, int& c) {
  c = min(max(count, 0), min(taps, wn));
  f = min(max(first - w0, 0), wn - c);
}

// grid: x = tiles of the padded output, y = frame; the channels are a loop
template <int DT>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const RsParams p) {
  extern __shared__ float rs_lds[];
  __shared__ RsTables tb;
  float* win = rs_lds;
  float* mid = rs_lds + (size_t)p.win_h * p.wpitch;
  const int TW = 1 << p.tw_log2, TH = 1 << p.th_log2, mpitch = TW + 1;
  const int Hp = p.y.n_out + p.pad_top, Wp = p.x.n_out + p.pad_left;
  const int tiles_x = (Wp + TW - 1) >> p.tw_log2;
  const int Y0 = (int)(blockIdx.x / tiles_x) << p.th_log2, X0 = (int)(blockIdx.x % tiles_x) << p.tw_log2;
  const long long frame = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // valid (un-padded) output indices of the tile: [iy0, iy1) x [ix0, ix1)
  const int iy0 = max(Y0 - p.pad_top, 0), iy1 = min(Y0 + TH - p.pad_top, p.y.n_out);
  const int ix0 = max(X0 - p.pad_left, 0), ix1 = min(X0 + TW - p.pad_left, p.x.n_out);
  const bool any = iy0 < iy1 && ix0 < ix1;
  int wy0 = 0, wyn = 0, wx0 = 0, wxn = 0;
  if (any) {
    wy0 = min(max(p.y.first[iy0], 0), p.y.n_in);
    wyn = min(min(max(p.y.first[iy1 - 1] + p.y.count[iy1 - 1], wy0), p.y.n_in) - wy0, p.win_h);
    wx0 = min(max(p.x.first[ix0], 0), p.x.n_in);
    wxn = min(min(max(p.x.first[ix1 - 1] + p.x.count[ix1 - 1], wx0), p.x.n_in) - wx0, p.win_w);
    for (int i = tid; i < ix1 - ix0; i += RS_THREADS) {
      rs_tap_range(p.x.first[ix0 + i], p.x.count[ix0 + i], p.x.taps, wx0, wxn, tb.xf[i], tb.xc[i]);
    }
    for (int i = tid; i < iy1 - iy0; i += RS_THREADS) {
      rs_tap_range(p.y.first[iy0 + i], p.y.count[iy0 + i], p.y.taps, wy0, wyn, tb.yf[i], tb.yc[i]);
    }
    for (int i = tid; i < (ix1 - ix0) * p.x.taps; i += RS_THREADS) tb.xw[i] = p.x.weight[(size_t)ix0 * p.x.taps + i];
    for (int i = tid; i < (iy1 - iy0) * p.y.taps; i += RS_THREADS) tb.yw[i] = p.y.weight[(size_t)iy0 * p.y.taps + i];
  }
  float fmin = 0.f, frange = 1.f;
  if (DT != MSEG_PIX_F32) {
    const unsigned lo = ~p.minmax[2 * frame], hi = p.minmax[2 * frame + 1];
    fmin = (float)lo; frange = (float)(hi - lo);
  }
  const int ncols = ix1 - ix0;
  for (int ch = 0; ch < p.C; ++ch) {
    if (any) {
      const long long sbase = frame * p.sfs + ch * p.scs + (long long)wy0 * p.srs + (long long)wx0 * p.sps;
      for (int r = wave; r < wyn; r += RS_THREADS / 64)
        for (int c = lane; c < wxn; c += 64)
          win[r * p.wpitch + c] = rs_load<DT>(p, sbase + r * p.srs + c * p.sps, fmin, frange);
      __syncthreads();       // (also: the tables are staged)
      for (unsigned idx = tid; idx < (unsigned)(wyn * ncols); idx += RS_THREADS) {
        const int oc = (int)(idx / (unsigned)wyn), r = (int)(idx - (unsigned)oc * (unsigned)wyn);
        const float* v = win + r * p.wpitch + tb.xf[oc];
        const float* w = tb.xw + oc * p.x.taps;
        const int cnt = tb.xc[oc];
        float acc = 0.f;
        for (int t = 0; t < cnt; ++t) acc = fmaf(w[t], v[t], acc);
        mid[r * mpitch + oc] = acc;
      }
      __syncthreads();
    }
    for (int idx = tid; idx < TW * TH; idx += RS_THREADS) {
      const int lx = idx & (TW - 1), ly = idx >> p.tw_log2;
      const int Y = Y0 + ly, X = X0 + lx;
      if (Y >= Hp || X >= Wp) continue;
      const int i = Y - p.pad_top, j = X - p.pad_left;
      float acc = -1.f;                                  // top / left padding: the normalised frame minimum
      if (i >= 0 && j >= 0) {
        const int li = i - iy0;
        const float* v = mid + tb.yf[li] * mpitch + (j - ix0);
        const float* w = tb.yw + li * p.y.taps;
        const int cnt = tb.yc[li];
        acc = 0.f;
        for (int t = 0; t < cnt; ++t) acc = fmaf(w[t], v[t * mpitch], acc);
      }
      p.dst[frame * p.dfs + ch * p.dcs + (long long)Y * p.drs + (long long)X * p.dps] = acc;
    }
    if (any && ch + 1 < p.C) __syncthreads();            // win / mid are refilled for the next channel
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// the table as the host sees it: every window inside [0, n_in), 1 <= count <= taps, first and first + count not decreasing
static bool rs_axis_valid(const MsegResampleAxis* a) {
  if (!a || !a->first || !a->count || !a->weight || !a->host_first || !a->host_count) return false;
  if (a->n_in <= 0 || a->n_out <= 0 || a->taps < 1 || a->taps > RS_MAX_TAPS) return false;
  int pf = 0, pe = 0;
  for (int i = 0; i < a->n_out; ++i) {
    const int f = a->host_first[i], c = a->host_count[i];
    if (f < 0 || c < 1 || c > a->taps || (long long)f + c > a->n_in) return false;
    if (f < pf || f + c < pe) return false;
    pf = f; pe = f + c;
  }
  return true;
}

// the largest source window of a tile of T outputs, tiles starting at multiples of T in the padded output
static int rs_max_window(const MsegResampleAxis* a, int T, int pad) {
  int widest = 0;
  for (long long P0 = 0; P0 < (long long)a->n_out + pad; P0 += T) {
    const long long i0 = P0 - pad > 0 ? P0 - pad : 0;
    const long long i1 = (P0 + T - pad < a->n_out ? P0 + T - pad : a->n_out) - 1;
    if (i1 < i0) continue;
    const int w = a->host_first[i1] + a->host_count[i1] - a->host_first[i0];
    widest = w > widest ? w : widest;
  }
  return widest;
}

static int rs_launch(RsParams& p, const MsegResampleAxis* ya, const MsegResampleAxis* xa, int dtype, hipStream_t stream) {
  p.y = RsAxis{ya->first, ya->count, ya->weight, ya->n_in, ya->n_out, ya->taps};
  p.x = RsAxis{xa->first, xa->count, xa->weight, xa->n_in, xa->n_out, xa->taps};
  const long long Hp = (long long)ya->n_out + p.pad_top, Wp = (long long)xa->n_out + p.pad_left;
  if (Hp > 0x7fffffffLL || Wp > 0x7fffffffLL) return MSEG_EINVAL;
  int twl = 6, thl = 4;
  size_t bytes = 0;
  for (bool halve_x = true;; halve_x = !halve_x) {
    const int TW = 1 << twl, TH = 1 << thl;
    p.win_w = rs_max_window(xa, TW, p.pad_left);
    p.win_h = rs_max_window(ya, TH, p.pad_top);
    p.wpitch = p.win_w | 1;
    bytes = ((size_t)p.win_h * p.wpitch + (size_t)p.win_h * (TW + 1)) * sizeof(float);
    if (bytes + sizeof(RsTables) <= RS_LDS_BYTES) break;
    if (twl == 0 && thl == 0) return MSEG_EINVAL;        // (12 x 12 taps fit a 1 x 1 tile: not reached)
    if ((halve_x && twl > 0) || thl == 0) --twl; else --thl;
  }
  p.tw_log2 = twl; p.th_log2 = thl;
  const long long tiles = ((Hp + (1 << thl) - 1) >> thl) * ((Wp + (1 << twl) - 1) >> twl);
  if (tiles > 0x7fffffffLL) return MSEG_EINVAL;
  const dim3 grid((unsigned)tiles, (unsigned)p.n), block(RS_THREADS);
  if (dtype == MSEG_PIX_U8) hipLaunchKernelGGL(resample_kernel<MSEG_PIX_U8>, grid, block, bytes, stream, p);
  else if (dtype == MSEG_PIX_U16) hipLaunchKernelGGL(resample_kernel<MSEG_PIX_U16>, grid, block, bytes, stream, p);
  else hipLaunchKernelGGL(resample_kernel<MSEG_PIX_F32>, grid, block, bytes, stream, p);
  MSEG_LAUNCH_CHECK();
  return MSEG_OK;
}

extern "C" int mseg_resample_frames(const void* src, int dtype, int n, const uint32_t* minmax,
                                    const MsegResampleAxis* yaxis, const MsegResampleAxis* xaxis, int pad_top, int pad_left,
                                    float* out, void* stream) {
  if (!src || !out || n <= 0 || n > 65535 || pad_top < 0 || pad_left < 0) return MSEG_EINVAL;
  if (dtype != MSEG_PIX_U8 && dtype != MSEG_PIX_U16 && dtype != MSEG_PIX_F32) return MSEG_EINVAL;
  if (dtype != MSEG_PIX_F32 && !minmax) return MSEG_EINVAL;
  if (!rs_axis_valid(yaxis) || !rs_axis_valid(xaxis)) return MSEG_EINVAL;
  RsParams p;
  p.src = src; p.minmax = minmax; p.dst = out;
  p.sfs = (long long)yaxis->n_in * xaxis->n_in; p.scs = 0; p.srs = xaxis->n_in; p.sps = 1;
  const long long Wp = (long long)xaxis->n_out + pad_left;
  p.dfs = ((long long)yaxis->n_out + pad_top) * Wp; p.dcs = 0; p.drs = Wp; p.dps = 1;
  p.n = n; p.C = 1; p.pad_top = pad_top; p.pad_left = pad_left;
  return rs_launch(p, yaxis, xaxis, dtype, (hipStream_t)stream);
}

extern "C" int mseg_resample_planes(const float* src, long long src_frame_stride, long long src_chan_stride,
                                    long long src_row_stride, long long src_pix_stride, int n, int C,
                                    const MsegResampleAxis* yaxis, const MsegResampleAxis* xaxis, float* dst,
                                    long long dst_frame_stride, long long dst_chan_stride, long long dst_row_stride,
                                    long long dst_pix_stride, void* stream) {
  if (!src || !dst || n <= 0 || n > 65535 || C <= 0) return MSEG_EINVAL;
  if (!rs_axis_valid(yaxis) || !rs_axis_valid(xaxis)) return MSEG_EINVAL;
  RsParams p;
  p.src = src; p.minmax = nullptr; p.dst = dst;
  p.sfs = src_frame_stride; p.scs = src_chan_stride; p.srs = src_row_stride; p.sps = src_pix_stride;
  p.dfs = dst_frame_stride; p.dcs = dst_chan_stride; p.drs = dst_row_stride; p.dps = dst_pix_stride;
  p.n = n; p.C = C; p.pad_top = 0; p.pad_left = 0;
  return rs_launch(p, yaxis, xaxis, MSEG_PIX_F32, (hipStream_t)stream);
}
