"""[extension] Test-time augmentation for inference: a frame is predicted under flips / rotations of the
square, every prediction is mapped back, the predictions are averaged and the average is segmented.

Transform codes are those of ``mseg_aug_flip`` (training/device_augment.py), extended to rectangles; for a plane ``a``:
0 ``a``, 1 ``fliplr``, 2 ``flipud``, 3 ``rot90``, 4 ``rot90(a, 2)``, 5 ``rot90(a, 3)``, 6 ``rot90(fliplr(a))`` = ``a.T``,
7 ``rot90(flipud(a))``.  3, 5, 6 and 7 transpose.  The members of a frame are expanded (``expand``) and their predictions
merged (``merge``) by csrc/tta.hip; there is no CPU path.
"""
import ctypes as C

import torch

from .. import _lib

MEMBER_CODES = {1: (0,), 2: (0, 1), 4: (0, 1, 2, 4), 8: (0, 1, 2, 3, 4, 5, 6, 7)}
TRANSPOSING = (3, 5, 6, 7)
_PIX = {torch.uint8: _lib.PIX_U8, torch.int16: _lib.PIX_U16, torch.uint16: _lib.PIX_U16, torch.float32: _lib.PIX_F32}


def member_codes(tta):
    """codes of the ``tta`` members of a frame, ascending (the order of the merge's sum); 1 = the frame itself = off"""
    if isinstance(tta, bool) or tta not in MEMBER_CODES:
        raise ValueError(f"tta must be one of 1, 2, 4, 8 (got {tta!r})")
    return MEMBER_CODES[tta]


def inverse_code(c):
    """code of the transform that undoes code ``c``: rot90 <-> rot270, every other code is its own inverse"""
    if c not in range(8):
        raise ValueError(f"transform code 0..7 expected (got {c!r})")
    return {3: 5, 5: 3}.get(c, c)


def shape_classes(codes, H, W):
    """members of an H x W frame by class: [(codes, (Hm, Wm), pads)] — the members that keep the orientation first, then
    (if any) those that transpose, W x H with its own padding.  The two classes stay apart for square frames as well: a
    class is one ``expand`` call and one batched forward."""
    from ..utils.utils import pad_amounts
    out = []
    for transposing in (False, True):
        cs = tuple(c for c in codes if (c in TRANSPOSING) == transposing)
        if cs:
            shape = (int(W), int(H)) if transposing else (int(H), int(W))
            out.append((cs, shape, [int(p) for p in pad_amounts(shape)]))
    return out


def chunk_members(Hp, Wp, frame_batch, K):
    """-> (m, frames): at most ``m = frame_batch_for(Hp, Wp, K * frame_batch)`` members go through one forward
    (``frame_batch`` 0 = auto as for infer_stack) and a group holds ``max(1, m // K)`` frames."""
    from .infer import frame_batch_for
    fb = int(frame_batch)
    m = frame_batch_for(Hp, Wp, int(K) * fb if fb > 0 else 0)
    return m, max(1, m // int(K))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def expand(src, codes, pads, minmax=None):
    """src: contiguous (n, H0, W0) CUDA tensor, uint8 / uint16 (int16 storage) raw frames with ``minmax`` (n, 2) int32 as
    mseg_frames_minmax writes it, or float32 frames that are normalised already.  ``codes``: the codes of ONE class,
    ``pads`` its (top, left) padding.  -> (k, n, Hm + top, Wm + left) float32: member-major, padded, normalised."""
    if src.dim() != 3 or src.dtype not in _PIX or not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("tta.expand: a contiguous (n, H, W) uint8 / uint16 / float32 CUDA tensor expected")
    if src.dtype != torch.float32 and minmax is None:
        raise RuntimeError("tta.expand: raw frames need their minmax")
    n, h0, w0 = src.shape
    k = len(codes)
    transposing = k > 0 and codes[0] in TRANSPOSING
    hm, wm = (w0, h0) if transposing else (h0, w0)
    out = torch.empty((k, n, hm + int(pads[0]), wm + int(pads[1])), dtype=torch.float32, device=src.device)
    arr = (C.c_int32 * max(k, 1))(*[int(c) for c in codes])
    _lib.check(_lib.load().mseg_tta_expand(src.data_ptr(), _PIX[src.dtype], n, h0, w0,
                                           None if minmax is None else minmax.data_ptr(), arr, k, int(pads[0]),
                                           int(pads[1]), out.data_ptr(), _stream()), "tta_expand")
    return out


def member(t, code, first=0, pads=(0, 0)):
    """descriptor of one member for ``merge``: ``t`` a float32 CUDA tensor (frames, C, rows, pixels) in any strides (permute
    an HWC tensor), the member's frames starting at index ``first``, its top / left padding skipped through the offset"""
    if t.dim() != 4 or t.dtype != torch.float32 or not t.is_cuda:
        raise RuntimeError("tta.member: a 4-D float32 CUDA tensor expected")
    fs, cs, rs, ps = t.stride()
    off = int(first) * fs + int(pads[0]) * rs + int(pads[1]) * ps
    return _lib.MsegTtaMember(t.data_ptr() + 4 * off, fs, cs, rs, ps, int(code), 0)


def merge(members, n, C_, H, W, hwc=False):
    """members: ``member`` descriptors in member order.  -> (n, C, H, W) float32, or (n, H, W, C) with ``hwc``: the ordered
    fp32 sum of the predictions, each mapped back by the inverse of its code, times 1 / K."""
    k = len(members)
    dev = torch.device("cuda", torch.cuda.current_device())
    if hwc:
        dst = torch.empty((n, H, W, C_), dtype=torch.float32, device=dev)
        fs, rs, ps, cs = dst.stride()
    else:
        dst = torch.empty((n, C_, H, W), dtype=torch.float32, device=dev)
        fs, cs, rs, ps = dst.stride()
    arr = (_lib.MsegTtaMember * max(k, 1))(*members)
    _lib.check(_lib.load().mseg_tta_merge(arr, k, int(n), int(C_), int(H), int(W), dst.data_ptr(), fs, cs, rs, ps,
                                          _stream()), "tta_merge")
    return dst
