"""CLAHE on the MI355X, exactly as the reference gets it from scikit-image (csrc/clahe.hip):

    (65535 * skimage.exposure.equalize_adapthist(np.squeeze(img), clip_limit=0.01)).astype(np.uint16)

(``src/training/mytransforms.py:92-95``, ``src/inference/inference_dataset.py:63-77``; scikit-image 0.18.3), bit for bit.
``clahe_device`` is the batched call on device tensors that the inference worker and the training augmentation use,
``equalize_adapthist_device`` the convenience front for one image or a stack of images of one shape.
"""
import numpy as np
import torch

from .. import _lib

_PIX = {torch.uint8: _lib.PIX_U8, torch.uint16: _lib.PIX_U16, torch.int16: _lib.PIX_U16, torch.float32: _lib.PIX_F32}


def clahe_device(src, apply=None, out_dtype=torch.uint16, out=None):
    """src: contiguous (N, H, W) device tensor, uint8 | uint16 (or its bits in int16 storage) | float32 holding the integers
    0..65535.  apply: None (all images) or an int32 device tensor (N,), 0 = the image is copied through unchanged.
    Returns a new (N, H, W) tensor of ``out_dtype`` (torch.uint16 | torch.int16 = the same bits | torch.float32), or fills
    ``out``.  Runs on the current stream; H, W >= 8."""
    if src.dim() != 3 or src.dtype not in _PIX or not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("clahe_device: a contiguous (N, H, W) uint8 / uint16 / float32 CUDA tensor expected")
    if out is None:
        out = torch.empty(src.shape, dtype=out_dtype, device=src.device)
    elif out.shape != src.shape or not out.is_contiguous() or out.device != src.device:
        raise RuntimeError("clahe_device: `out` must be a contiguous tensor of the input's shape on its device")
    if out.dtype not in (torch.uint16, torch.int16, torch.float32):
        raise RuntimeError("clahe_device: the result is uint16 (or int16 storage) or float32")
    if apply is not None and (apply.dtype != torch.int32 or apply.numel() != src.shape[0] or not apply.is_cuda):
        raise RuntimeError("clahe_device: `apply` must be an int32 device tensor with one flag per image")
    lib = _lib.load()
    n, h, w = (int(v) for v in src.shape)
    nbytes = lib.mseg_clahe_workspace_bytes(n, h, w)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.mseg_clahe_u16(src.data_ptr(), _PIX[src.dtype], n, h, w,
                                      None if apply is None else apply.data_ptr(), out.data_ptr(), _PIX[out.dtype],
                                      ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "clahe_u16")
    return out


def equalize_adapthist_device(img, device=None):
    """uint8 / uint16 image (H, W) or images (N, H, W) — a device tensor or a numpy array — -> the uint16 tensor of the same
    shape on the device that ``(65535 * equalize_adapthist(img, clip_limit=0.01)).astype(np.uint16)`` gives per image."""
    if isinstance(img, np.ndarray):
        if img.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"equalize_adapthist_device: uint8 or uint16 images only, got {img.dtype} (float images "
                             "have no fixed grey-level range here; convert them first)")
        host = np.ascontiguousarray(img)
        t = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host)
        t = t.to(torch.device(device if device is not None else "cuda"))
    elif isinstance(img, torch.Tensor):
        if img.dtype not in (torch.uint8, torch.uint16, torch.int16):
            raise ValueError(f"equalize_adapthist_device: uint8 or uint16 images only, got {img.dtype} (float images "
                             "have no fixed grey-level range here; convert them first)")
        t = img if device is None else img.to(torch.device(device))
        if not t.is_cuda:
            t = t.to("cuda")
        t = t.contiguous()
    else:
        raise ValueError("equalize_adapthist_device: a numpy array or a torch tensor expected")
    if t.dim() not in (2, 3):
        raise ValueError("equalize_adapthist_device: (H, W) or (N, H, W) expected")
    out = clahe_device(t if t.dim() == 3 else t[None])
    return out if t.dim() == 3 else out[0]
