#!/usr/bin/env python3
"""Times the library-exact CLAHE (mseg_clahe_u16, csrc/clahe.hip) on the MI355X:

  * a batch of 32 x 256^2 fp32 planes, every image enhanced — the shape of the training augmentation — through the new
    call and through the earlier stand-in (mseg_aug_clahe) in the same process, alternating call by call;
  * one 2048^2 uint16 frame, the shape of inference with --clahe.

Each call is timed with device events on the current stream (workspace allocated beforehand); the median over the repeats
is reported, with the GB/s that the bytes each pass has to move amount to:
    new, fp32 -> fp32:    min/max reads 4, tile maps read 4, blend reads 4 + writes 2, rescale reads 2 + writes 4 = 20 B/px
    new, uint16 -> uint16: 2 + 2 + (2 + 2) + (2 + 2)                                                             = 12 B/px
    old, fp32 -> fp32:    tile maps read 4, apply reads 4 + writes 4                                             = 12 B/px
No gate: the two operations compute different things.  One JSON line.

    python tools/bench_clahe.py [--reps 30]
"""
import argparse
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def images(n, s, seed):
    """gradient + blobs + noise, uint16"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:s, 0:s].astype(np.float32)
    out = np.empty((n, s, s), np.uint16)
    for i in range(n):
        img = 400 + 9000 * (0.3 + 0.2 * np.sin(x / (0.2 * s)) * np.cos(y / (0.15 * s)))
        for _ in range(12):
            cy, cx, r = rng.uniform(0, s), rng.uniform(0, s), rng.uniform(0.01 * s, 0.06 * s)
            img += 6000 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
        img += rng.normal(0, 150, (s, s))
        out[i] = np.clip(img, 0, 65535).astype(np.uint16)
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    from microbeseg_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    med = lambda v: float(np.median(np.asarray(v)))      # noqa: E731

    # batch of 32 x 256^2, fp32 planes
    N, S = 32, 256
    src = torch.from_numpy(images(N, S, 1).astype(np.float32)).to(dev)
    dst_new, dst_old = torch.empty_like(src), torch.empty_like(src)
    nb = lib.mseg_clahe_workspace_bytes(N, S, S)
    ws_new = torch.empty(nb, dtype=torch.uint8, device=dev)
    ws_old = torch.empty(lib.mseg_aug_clahe_workspace_bytes(N), dtype=torch.uint8, device=dev)
    choice = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    choice[:, 0] = 3

    def new():
        _lib.check(lib.mseg_clahe_u16(src.data_ptr(), _lib.PIX_F32, N, S, S, None, dst_new.data_ptr(), _lib.PIX_F32,
                                      ws_new.data_ptr(), nb, st), "clahe_u16")

    def old():
        _lib.check(lib.mseg_aug_clahe(src.data_ptr(), dst_old.data_ptr(), N, S, S, choice.data_ptr(), ws_old.data_ptr(), st),
                   "aug_clahe")
    for _ in range(3):
        new()
        old()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(args.reps):
        t_new.append(timed(new))
        t_old.append(timed(old))
    px = N * S * S
    res = {"batch_32x256_new_ms": round(med(t_new), 4), "batch_32x256_old_ms": round(med(t_old), 4),
           "batch_32x256_new_over_old": round(med(t_new) / med(t_old), 2),
           "batch_32x256_new_GBps": round(20 * px / med(t_new) / 1e6, 1),
           "batch_32x256_old_GBps": round(12 * px / med(t_old) / 1e6, 1)}

    # one 2048^2 uint16 frame
    F = 2048
    frame = torch.from_numpy(images(1, F, 2).view(np.int16)).to(dev)
    out = torch.empty_like(frame)
    nbf = lib.mseg_clahe_workspace_bytes(1, F, F)
    wsf = torch.empty(nbf, dtype=torch.uint8, device=dev)

    def one():
        _lib.check(lib.mseg_clahe_u16(frame.data_ptr(), _lib.PIX_U16, 1, F, F, None, out.data_ptr(), _lib.PIX_U16,
                                      wsf.data_ptr(), nbf, st), "clahe_u16")
    for _ in range(3):
        one()
    torch.cuda.synchronize()
    t_one = [timed(one) for _ in range(args.reps)]
    res.update({"frame_2048_u16_ms": round(med(t_one), 4), "frame_2048_u16_GBps": round(12 * F * F / med(t_one) / 1e6, 1),
                "reps": args.reps, "device": torch.cuda.get_device_name(0)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
