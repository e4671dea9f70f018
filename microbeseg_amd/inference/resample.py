"""[extension] Inference at a chosen resolution (``InferWorker.scale``): the resampling rule and the
wrappers of its two kernels (csrc/resample.hip).

The rule is separable, anti-aliased linear resampling with pixel-centre alignment — what
``torch.nn.functional.interpolate(mode='bilinear', align_corners=False, antialias=True)`` computes for an explicit
``size``: plain bilinear when enlarging, a triangle filter widened by the ratio when shrinking.  It lives HERE, as one
table per axis computed on the host in float64 (``axis_table``); the kernels receive the tables and compute no weights.
There is no CPU path for the resampling itself.
"""
import ctypes as C
import functools
import math
import numbers

import numpy as np

SCALE_MIN, SCALE_MAX = 0.25, 4.0
MAX_TAPS = 12                                   # RS_MAX_TAPS of csrc/resample.hip


def check_scale(scale):
    """``scale`` as a float; ValueError for a bool, a non-number, a NaN and anything outside [0.25, 4]"""
    if isinstance(scale, bool) or not isinstance(scale, numbers.Real):
        raise ValueError(f"scale must be a real number in [{SCALE_MIN}, {SCALE_MAX}] (got {scale!r})")
    s = float(scale)
    if math.isnan(s) or not SCALE_MIN <= s <= SCALE_MAX:
        raise ValueError(f"scale must be a real number in [{SCALE_MIN}, {SCALE_MAX}] (got {scale!r})")
    return s


def out_size(n, s):
    """edge length of an ``n``-pixel axis at scale ``s``: max(1, floor(n * s + 0.5))"""
    return max(1, int(math.floor(int(n) * float(s) + 0.5)))


def axis_table(n_in, n_out, dtype=np.float32):
    """-> (first int32[n_out], count int32[n_out], weight float32[n_out, taps]): output element i is
    ``sum_t weight[i, t] * v[first[i] + t]`` over ``t < count[i]``; the weights of a row are zero beyond its count.
    float64 on the host: r = n_in / n_out, sup = max(r, 1), c = r (i + 0.5); the window is [int(c - sup + 0.5) clipped at 0,
    int(c + sup + 0.5) clipped at n_in), the weight of source j is max(0, 1 - |j - c + 0.5| / sup), divided by the
    row's sum and then rounded to fp32 (``dtype=np.float64`` keeps the weights as computed: for checking the rule)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"axis_table: positive sizes expected (got {n_in}, {n_out})")
    r = n_in / n_out
    sup = max(r, 1.0)
    first = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    rows = []
    for i in range(n_out):
        c = r * (i + 0.5)
        lo = max(int(c - sup + 0.5), 0)
        hi = min(int(c + sup + 0.5), n_in)
        w = np.maximum(0.0, 1.0 - np.abs(np.arange(lo, hi, dtype=np.float64) - c + 0.5) / sup)
        first[i], count[i] = lo, hi - lo
        rows.append(w / w.sum())
    taps = int(count.max())
    weight = np.zeros((n_out, taps), dtype)
    for i, w in enumerate(rows):
        weight[i, :len(w)] = w
    return first, count, weight


class Axis:
    """an axis table on the host and on one device, and its descriptor for the kernels"""

    def __init__(self, n_in, n_out, device):
        import torch
        from .. import _lib
        self.first, self.count, self.weight = axis_table(n_in, n_out)
        self.n_in, self.n_out, self.taps = int(n_in), int(n_out), int(self.weight.shape[1])
        if self.taps > MAX_TAPS:
            raise RuntimeError(f"resample: {self.taps} taps per output ({n_in} -> {n_out}); the kernels take up to "
                               f"{MAX_TAPS}")
        self.dev = tuple(torch.from_numpy(a).to(device) for a in (self.first, self.count, self.weight))
        self.desc = _lib.MsegResampleAxis(self.dev[0].data_ptr(), self.dev[1].data_ptr(), self.dev[2].data_ptr(),
                                          self.first.ctypes.data, self.count.ctypes.data, self.n_in, self.n_out,
                                          self.taps, 0)


@functools.lru_cache(maxsize=32)
def _axis(n_in, n_out, device):
    return Axis(n_in, n_out, device)


def axis(n_in, n_out, device):
    """the (cached) ``Axis`` of ``n_in -> n_out`` on ``device``"""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("resample: the tables live on a GPU; there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _axis(int(n_in), int(n_out), device)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def frames(src, yaxis, xaxis, pads=(0, 0), minmax=None):
    """src: contiguous (n, H0, W0) CUDA tensor, uint8 / uint16 (int16 storage) raw frames with ``minmax`` (n, 2) int32 as
    mseg_frames_minmax writes it, or float32 frames that are normalised already.  -> (n, Hs + top, Ws + left) float32:
    every frame normalised, resampled to ``yaxis.n_out x xaxis.n_out`` and padded top / left with -1."""
    import torch
    from .. import _lib
    pix = {torch.uint8: _lib.PIX_U8, torch.int16: _lib.PIX_U16, torch.uint16: _lib.PIX_U16, torch.float32: _lib.PIX_F32}
    if src.dim() != 3 or src.dtype not in pix or not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("resample.frames: a contiguous (n, H, W) uint8 / uint16 / float32 CUDA tensor expected")
    if src.dtype != torch.float32 and minmax is None:
        raise RuntimeError("resample.frames: raw frames need their minmax")
    n, h0, w0 = src.shape
    if (h0, w0) != (yaxis.n_in, xaxis.n_in):
        raise RuntimeError(f"resample.frames: tables for {yaxis.n_in} x {xaxis.n_in}, frames of {h0} x {w0}")
    out = torch.empty((n, yaxis.n_out + int(pads[0]), xaxis.n_out + int(pads[1])), dtype=torch.float32, device=src.device)
    _lib.check(_lib.load().mseg_resample_frames(src.data_ptr(), pix[src.dtype], n,
                                                None if minmax is None else minmax.data_ptr(), C.byref(yaxis.desc),
                                                C.byref(xaxis.desc), int(pads[0]), int(pads[1]), out.data_ptr(),
                                                _stream()), "resample_frames")
    return out


def planes(t, yaxis, xaxis, pads=(0, 0), hwc=False):
    """t: float32 CUDA tensor (frames, C, rows, pixels) in any strides (permute an HWC tensor) whose top / left ``pads``
    are skipped; what follows them is ``yaxis.n_in x xaxis.n_in``.  -> (n, C, H, W) float32, or (n, H, W, C) with ``hwc``,
    H x W = ``yaxis.n_out x xaxis.n_out``."""
    import torch
    from .. import _lib
    if t.dim() != 4 or t.dtype != torch.float32 or not t.is_cuda:
        raise RuntimeError("resample.planes: a 4-D float32 CUDA tensor expected")
    n, ch, rows, cols = t.shape
    if (rows - int(pads[0]), cols - int(pads[1])) != (yaxis.n_in, xaxis.n_in):
        raise RuntimeError(f"resample.planes: tables for {yaxis.n_in} x {xaxis.n_in}, planes of {rows} x {cols} with "
                           f"pads {tuple(pads)}")
    fs, cs, rs, ps = t.stride()
    off = int(pads[0]) * rs + int(pads[1]) * ps
    if hwc:
        dst = torch.empty((n, yaxis.n_out, xaxis.n_out, ch), dtype=torch.float32, device=t.device)
        dfs, drs, dps, dcs = dst.stride()
    else:
        dst = torch.empty((n, ch, yaxis.n_out, xaxis.n_out), dtype=torch.float32, device=t.device)
        dfs, dcs, drs, dps = dst.stride()
    _lib.check(_lib.load().mseg_resample_planes(t.data_ptr() + 4 * off, fs, cs, rs, ps, n, ch, C.byref(yaxis.desc),
                                                C.byref(xaxis.desc), dst.data_ptr(), dfs, dcs, drs, dps, _stream()),
               "resample_planes")
    return dst
