#!/usr/bin/env python3
"""Per-cell intensity profile on the MI355X: device milliseconds per frame of mseg_cell_profile at N = 8, 16 and
32 bins (HIP events around the call) and, alternating in the same process, of mseg_cell_order_stats for the percentiles (5, 50,
95), the yardstick: the existing one-wave-per-cell, two-walk kernel over the same boxes (its whole call, and the same call with
n_labels = 0, which leaves its background passes alone: the difference is its cell pass); the all-in time of measure_cells with
and without profile=16 (medians of alternating calls); the numpy restatement (tests/profile_ref.py) on one frame for one host
core.  Synthetic stack as in tools/bench_cells.py: 2048^2 frames with about 2400 cells each, uint16 labels, a 2-channel uint16
image.  Prints one JSON line at the end.  GPU box only.
  python tools/bench_profile.py [--frames 16] [--reps 9] [--host-reps 5] [--no-host]"""
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
import profile_ref as pref  # noqa: E402

PERCENTILES = (5, 50, 95)
BINS = (8, 16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=5, help="timed measure_cells calls per setting")
    ap.add_argument("--no-host", action="store_true", help="device times only (for a profiler run)")
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(7))
    labels = stack(rng, a.frames)
    T, H, W = labels.shape
    Cn, R = 2, 2 * len(PERCENTILES)
    img = (rng.integers(0, 4096, (T, Cn, H, W)) + 2000 * (labels[:, None] > 0)).astype(np.uint16)
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lab_d = torch.from_numpy(labels.view(np.int16)).to(dev)
    img_d = torch.from_numpy(img.view(np.int16)).to(dev)
    off = ref.frame_tables(labels)
    n = int(off[-1])
    off_d = torch.from_numpy(off).to(dev)
    off0_d = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    strides = (Cn * H * W, H * W, W, 1)
    raw = cells.measure_raw(lab_d, _lib.PIX_U16, off, cells._image_to_device(img_d, (T, H, W), dev), [0, 1])
    area, bg_n = raw["shape"][0].astype(np.int64), raw["bg_sums"][0, :, 0].astype(np.int64)
    bbox = torch.from_numpy(raw["bbox"]).to(dev)
    dirs = cells._cell_directions(raw)
    dirs_d = torch.from_numpy(dirs).to(dev)
    ranks, bg_ranks = cells.percentile_ranks(area, PERCENTILES)[0], cells.percentile_ranks(bg_n, PERCENTILES)[0]
    ranks_d, bg_ranks_d = torch.from_numpy(ranks).to(dev), torch.from_numpy(bg_ranks).to(dev)
    values = torch.empty((R, Cn, n), dtype=torch.int32, device=dev)
    bg_values = torch.empty((R, T, Cn), dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mseg_cell_order_stats_workspace_bytes(T, n, Cn, R), dtype=torch.uint8, device=dev)
    count = torch.empty((max(BINS), n), dtype=torch.int32, device=dev)
    sums = torch.empty((Cn, max(BINS), n), dtype=torch.int64, device=dev)
    extent = torch.empty((2, n), dtype=torch.int64, device=dev)

    def order(cells_too=True):
        _lib.check(lib.mseg_cell_order_stats(lab_d.data_ptr(), _lib.PIX_U16, T, H, W,
                                             (off_d if cells_too else off0_d).data_ptr(), n if cells_too else 0,
                                             img_d.data_ptr(), _lib.PIX_U16, Cn, *strides, bbox.data_ptr(), R, ranks_d.data_ptr(),
                                             bg_ranks_d.data_ptr(), values.data_ptr(), bg_values.data_ptr(), status.data_ptr(),
                                             ws.data_ptr(), ws.numel(), st))

    def profile(N):
        _lib.check(lib.mseg_cell_profile(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, img_d.data_ptr(),
                                         _lib.PIX_U16, Cn, *strides, bbox.data_ptr(), dirs_d.data_ptr(), N, count.data_ptr(),
                                         sums.data_ptr(), extent.data_ptr(), st))

    box = raw["bbox"].astype(np.int64)
    box_px = float(((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])).sum()) / T
    cell_px = float(area.sum()) / T
    print(f"stack {T} x {H} x {W}, {Cn} channels, {n} cells ({n / T:.0f} per frame), {box_px:.0f} box pixels and {cell_px:.0f} "
          f"cell pixels per frame")
    passes = [(f"profile_{N}", lambda N=N: profile(N)) for N in BINS] + \
        [("order_stats", order), ("order_stats_background_only", lambda: order(False))]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {name: [] for name, _ in passes}
    for _ in range(2):                                        # warm-up: code objects, caches, clocks
        for _, fn in passes:
            fn()
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0, "a rank beyond a cell's pixels"
    for _ in range(a.reps):                                  # alternating: all passes see the same machine state
        for name, fn in passes:
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    res = {"frames": T, "height": H, "width": W, "channels": Cn, "cells_per_frame": n / T, "box_pixels_per_frame": box_px,
           "cell_pixels_per_frame": cell_px, "reps": a.reps}
    for name, v in ms.items():
        med = float(np.median(v))
        res[f"{name}_ms_per_frame"] = med / T
        res[f"{name}_ms_per_frame_min_max"] = [min(v) / T, max(v) / T]
        print(f"  {name:28s} {med / T:8.4f} ms per frame ({min(v) / T:.4f} .. {max(v) / T:.4f})")
    res["order_stats_cell_pass_ms_per_frame"] = res["order_stats_ms_per_frame"] - res["order_stats_background_only_ms_per_frame"]
    # what a profile call has to move per frame: the labels of the boxes twice (two walks), the channel values of the cells'
    # pixels once, the boxes and directions in, the bins out
    for N in BINS:
        moved = 2 * 2 * box_px + 2 * Cn * cell_px + (n / T) * (16 + 8 + 4 * N + 8 * Cn * N + 16)
        res[f"profile_{N}_bytes_per_frame"] = moved
        res[f"profile_{N}_gb_per_s"] = moved / (res[f"profile_{N}_ms_per_frame"] * 1e-3) / 1e9
        res[f"profile_{N}_over_order_stats_cell_pass"] = res[f"profile_{N}_ms_per_frame"] / res["order_stats_cell_pass_ms_per_frame"]
        print(f"  profile_{N}: {moved / 1e6:.2f} MB per frame, {res[f'profile_{N}_gb_per_s']:.1f} GB/s, "
              f"{res[f'profile_{N}_over_order_stats_cell_pass']:.2f} x the order-statistics cell pass "
              f"({res['order_stats_cell_pass_ms_per_frame']:.4f} ms per frame)")
    if not a.no_host:
        keys = {None: "measure_cells_all_in_ms_per_frame", 16: "measure_cells_profile_all_in_ms_per_frame"}
        took = {bins: [] for bins in keys}
        for bins in keys:                                         # warm-up
            cells.measure_cells(lab_d, img_d, profile=bins)
        for _ in range(a.host_reps):                              # alternating, like the device passes
            for bins in keys:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                df = cells.measure_cells(lab_d, img_d, profile=bins)
                took[bins].append(1e3 * (time.perf_counter() - t0) / T)
        for bins, key in keys.items():
            res[key] = float(np.median(took[bins]))
            res[key + "_min_max"] = [min(took[bins]), max(took[bins])]
            print(f"  measure_cells(profile={bins}) all-in {res[key]:8.1f} ms per frame ({min(took[bins]):.1f} .. {max(took[bins]):.1f}, "
                  f"{a.host_reps} runs)")
        res["host_reps"] = a.host_reps
        k = int(off[1])
        profile(16)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = pref.profile(labels[:1], off[:2], img[:1], box[:k], dirs[:k], 16)
        res["numpy_restatement_s_per_frame_per_core"] = time.perf_counter() - t0
        print(f"  numpy restatement {res['numpy_restatement_s_per_frame_per_core']:8.2f} s per frame on one host core")
        assert np.array_equal(count.cpu().numpy().view(np.uint32).reshape(-1)[:16 * n].reshape(16, n)[:, :k], want[0]), \
            "device and restatement differ"
        assert np.array_equal(sums.cpu().numpy().view(np.uint64).reshape(-1)[:Cn * 16 * n].reshape(Cn, 16, n)[:, :, :k], want[1]), \
            "device and restatement differ"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
