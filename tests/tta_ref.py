"""Plain numpy restatement of test-time augmentation, written from the definitions:

  transform(a, code)          the eight symmetries, extended to rectangles, as index arithmetic
  inverse(code)               the code that undoes ``code``
  member_input(frame, code)   what the network gets for that member: the host normalisation formula + zero_pad_model_input
  merge(members, codes, K)    fp32 left-to-right sum of the members mapped back, one multiply by 1 / K
"""
import numpy as np

TRANSPOSING = (3, 5, 6, 7)


def transform(a, code):
    """out[i][j] = a[si][sj] on the LAST TWO axes of ``a`` (H x W); codes 3, 5, 6, 7 give W x H"""
    a = np.asarray(a)
    H, W = a.shape[-2:]
    code = int(code)
    if code in TRANSPOSING:
        i, j = np.mgrid[0:W, 0:H]
    else:
        i, j = np.mgrid[0:H, 0:W]
    si, sj = {0: (i, j), 1: (i, W - 1 - j), 2: (H - 1 - i, j), 3: (j, W - 1 - i), 4: (H - 1 - i, W - 1 - j),
              5: (H - 1 - j, i), 6: (j, i), 7: (H - 1 - j, W - 1 - i)}[code]
    return np.ascontiguousarray(a[..., si, sj])


def inverse(code):
    return {3: 5, 5: 3}.get(int(code), int(code))


def member_input(frame, code):
    """-> (padded, normalised member of an integer frame, fp32; pads).  The extrema are the frame's own (the transforms do
    not change them); a float frame is taken as normalised already and padded with -1."""
    from microbeseg_amd.utils.utils import zero_pad_model_input
    frame = np.asarray(frame)
    t = transform(frame, code)
    if frame.dtype == np.float32:
        return zero_pad_model_input(t, pad_val=np.float32(-1.0))
    fmin, fmax = np.min(frame), np.max(frame)
    padded, pads = zero_pad_model_input(t, pad_val=fmin)
    return (2 * (padded.astype(np.float32) - fmin) / (fmax - fmin) - 1).astype(np.float32), pads


def merge(members, codes, K):
    """members[m]: un-padded prediction of member m in ITS orientation, (..., Hm, Wm) fp32; -> (..., H, W) fp32:
    (((p_0 + p_1) + p_2) + ...) * (1 / K) with p_m mapped back by the inverse of codes[m]"""
    assert len(members) == len(codes) == K
    acc = None
    for p, c in zip(members, codes):
        back = transform(np.asarray(p, dtype=np.float32), inverse(c))
        acc = back.copy() if acc is None else (acc + back).astype(np.float32)
    return (acc * np.float32(1.0 / K)).astype(np.float32)
