#!/usr/bin/env python3
"""Per-cell fluorescent foci on the MI355X: device milliseconds per frame of mseg_cell_spots at scale 1, 2 and
5 (HIP events around the whole call: the list cleared, initialisation, tile pass) and, alternating in the same process, of
mseg_cell_measure with the same 2 channels, the yardstick; the rate against the bytes the call has to move (the labels once
plus each channel once); the all-in time of measure_cells with and without spots; the numpy restatement (tests/spots_ref.py)
on one frame for one host core.  Synthetic stack as in tools/bench_cells.py: 2048^2 frames with about 2400 cells each, uint16
labels, a 2-channel uint16 image of noise with about two planted foci per cell.  Prints one JSON line at the end.  GPU box only.
  python tools/bench_spots.py [--frames 16] [--reps 9] [--threshold 1500] [--no-host]"""
import argparse
import ctypes as C
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
from microbeseg_amd import _lib  # noqa: E402
from microbeseg_amd.inference import cells  # noqa: E402
from bench_analysis import stack  # noqa: E402
import cells_ref as ref  # noqa: E402
import spots_ref as sref  # noqa: E402

SCALES = (1, 2, 5)
THRESHOLD = 1500          # grey levels: about nine standard deviations of the noise's response at scale 1, fewer foci above


def planted(rng, labels, channels=2, per_cell=2, amplitude=20000):
    """uniform noise in 0 .. 4095 plus 7 x 7 Gaussian stamps (sigma 1) on random cell pixels, about ``per_cell`` per cell"""
    T, H, W = labels.shape
    img = rng.integers(0, 4096, (T, channels, H, W)).astype(np.int64)
    yy, xx = np.mgrid[-3:4, -3:4]
    stamp = np.rint(amplitude * np.exp(-(yy * yy + xx * xx) / 2.0)).astype(np.int64)
    for t in range(T):
        ys, xs = np.nonzero(labels[t])
        for c in range(channels):
            pick = rng.choice(len(ys), per_cell * int(labels[t].max()), replace=False)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    np.add.at(img[t, c], (np.clip(ys[pick] + dy, 0, H - 1), np.clip(xs[pick] + dx, 0, W - 1)),
                              stamp[dy + 3, dx + 3])
    return np.minimum(img, 65535).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threshold", type=int, default=THRESHOLD, help="grey levels; 65535 finds no spot: the filter alone")
    ap.add_argument("--no-host", action="store_true", help="device times only (for a profiler run)")
    a = ap.parse_args()
    thr = a.threshold
    rng = np.random.Generator(np.random.PCG64(7))
    labels = stack(rng, a.frames)
    T, H, W = labels.shape
    Cn = 2
    img = planted(rng, labels, Cn)
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lab_d = torch.from_numpy(labels.view(np.int16)).to(dev)
    img_d = torch.from_numpy(img.view(np.int16)).to(dev)
    off = ref.frame_tables(labels)
    n = int(off[-1])
    off_d = torch.from_numpy(off).to(dev)
    shape = torch.empty((6, n), dtype=torch.int64, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    chs, chm = torch.empty((2, Cn, n), dtype=torch.int64, device=dev), torch.empty((2, Cn, n), dtype=torch.int32, device=dev)
    bgs, bgm = torch.empty((3, T, Cn), dtype=torch.int64, device=dev), torch.empty((2, T, Cn), dtype=torch.int32, device=dev)
    strides = (Cn * H * W, H * W, W, 1)

    def measure():
        _lib.check(lib.mseg_cell_measure(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, img_d.data_ptr(),
                                         _lib.PIX_U16, Cn, *strides, shape.data_ptr(), bbox.data_ptr(), chs.data_ptr(),
                                         chm.data_ptr(), bgs.data_ptr(), bgm.data_ptr(), st))

    cap = 16 * n
    cell_count = torch.empty((Cn, n), dtype=torch.int32, device=dev)
    bg_count = torch.empty((T, Cn), dtype=torch.int32, device=dev)
    records = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    tail = torch.empty(2, dtype=torch.int64, device=dev)                     # n_spots, status
    ws = torch.empty(lib.mseg_cell_spots_workspace_bytes(T, n, Cn), dtype=torch.uint8, device=dev)

    def spots(s):
        _lib.check(lib.mseg_cell_spots(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, img_d.data_ptr(),
                                       _lib.PIX_U16, Cn, *strides, s, thr, cell_count.data_ptr(), bg_count.data_ptr(),
                                       records.data_ptr(), cap, tail.data_ptr(), tail.data_ptr() + 8, ws.data_ptr(), ws.numel(),
                                       st))

    frame_bytes = H * W * (2 + 2 * Cn)                       # the labels once plus each channel once
    print(f"stack {T} x {H} x {W}, {n} cells ({n / T:.0f} per frame), {Cn} uint16 channels, threshold {thr}, room for "
          f"{cap} spots, {frame_bytes / 1e6:.1f} MB to move per frame")
    fns = [("measure", measure)] + [(f"spots_s{s}", (lambda s=s: spots(s))) for s in SCALES]
    res = {"frames": T, "height": H, "width": W, "channels": Cn, "cells_per_frame": n / T, "threshold": thr,
           "bytes_per_frame": frame_bytes}
    for name, fn in fns:
        fn()
        torch.cuda.synchronize()
        if name != "measure":
            end = tail.cpu().numpy()
            assert end[1:].view(np.int32)[0] == 0 and end[0] <= cap, "the spot list was too short"
            res[f"{name}_spots_per_frame"] = int(end[0]) / T
            res[f"{name}_spots_on_cells_per_frame"] = int(cell_count.sum()) / T
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {name: [] for name, _ in fns}
    for _ in range(a.reps):                                  # alternating: all passes see the same machine state
        for name, fn in fns:
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    for name, v in ms.items():
        med = float(np.median(v))
        res[f"{name}_ms_per_frame"] = med / T
        res[f"{name}_ms_per_frame_min_max"] = [min(v) / T, max(v) / T]
        res[f"{name}_gb_per_s"] = frame_bytes * T / (med * 1e-3) / 1e9
        extra = f", {res[f'{name}_spots_per_frame']:.0f} spots per frame" if name != "measure" else ""
        print(f"  {name:10s} {med / T:8.4f} ms per frame ({min(v) / T:.4f} .. {max(v) / T:.4f}), "
              f"{res[f'{name}_gb_per_s']:.0f} GB/s of the bytes to move{extra}")
    if not a.no_host:
        for flag in (None, thr, None, thr):      # alternating; the second round is the one reported
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            df = cells.measure_cells(lab_d, img_d, spots=flag)
            key = "measure_cells_spots_all_in_ms_per_frame" if flag else "measure_cells_all_in_ms_per_frame"
            res[key] = 1e3 * (time.perf_counter() - t0) / T
            print(f"  measure_cells(spots={flag}) all-in {res[key]:8.1f} ms per frame ({len(df)} rows, {len(df.columns)} columns)")
        t0 = time.perf_counter()
        table = cells.cell_spots(lab_d, img_d, spots=thr)
        res["cell_spots_all_in_ms_per_frame"] = 1e3 * (time.perf_counter() - t0) / T
        print(f"  cell_spots all-in {res['cell_spots_all_in_ms_per_frame']:8.1f} ms per frame ({len(table)} rows)")
        t0 = time.perf_counter()
        want = sref.reference(labels[:1], off[:2], img[:1], list(range(Cn)), thr, 2)
        res["numpy_restatement_s2_s_per_frame_per_core"] = time.perf_counter() - t0
        print(f"  numpy restatement, scale 2 {res['numpy_restatement_s2_s_per_frame_per_core']:8.1f} s per frame on one host core")
        spots(2)
        got = records.cpu().numpy().reshape(-1).view(cells.SPOT_RECORD)[:int(tail.cpu()[0])]
        got = got[got["frame"] == 0]
        got = got[np.lexsort((got["x"], got["y"], got["channel"]))]
        assert got.tolist() == want[2], "device and restatement differ"
        assert np.array_equal(cell_count.cpu().numpy()[:, :int(off[1])], want[0])
        assert np.array_equal(bg_count.cpu().numpy()[:1], want[1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
