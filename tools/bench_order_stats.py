#!/usr/bin/env python3
"""Per-cell percentiles on the MI355X: device milliseconds per frame of mseg_cell_order_stats (HIP events
around the whole call: workspace clearing, the cell pass, the four background passes) and, alternating in the same process, of
mseg_cell_measure with the same 2 channels, the yardstick; the same call with n_labels = 0, which leaves the background passes
alone; the all-in time of measure_cells with and without percentiles; the numpy restatement (tests/order_stats_ref.py, np.sort
per cell) on one frame for one host core.  Synthetic stack as in tools/bench_cells.py: 2048^2 frames with about 2400 cells
each, uint16 labels, a 2-channel uint16 image, percentiles (5, 50, 95).  Prints one JSON line at the end.  GPU box only.
  python tools/bench_order_stats.py [--frames 16] [--reps 9] [--no-host]"""
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
import order_stats_ref as oref  # noqa: E402

PERCENTILES = (5, 50, 95)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
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
    shape = torch.empty((6, n), dtype=torch.int64, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    chs, chm = torch.empty((2, Cn, n), dtype=torch.int64, device=dev), torch.empty((2, Cn, n), dtype=torch.int32, device=dev)
    bgs, bgm = torch.empty((3, T, Cn), dtype=torch.int64, device=dev), torch.empty((2, T, Cn), dtype=torch.int32, device=dev)
    strides = (Cn * H * W, H * W, W, 1)

    def measure():
        _lib.check(lib.mseg_cell_measure(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, img_d.data_ptr(),
                                         _lib.PIX_U16, Cn, *strides, shape.data_ptr(), bbox.data_ptr(), chs.data_ptr(),
                                         chm.data_ptr(), bgs.data_ptr(), bgm.data_ptr(), st))

    measure()
    area = shape.cpu().numpy()[0]
    bg_n = bgs.cpu().numpy()[0, :, 0]
    ranks, bg_ranks = cells.percentile_ranks(area, PERCENTILES)[0], cells.percentile_ranks(bg_n, PERCENTILES)[0]
    ranks_d, bg_ranks_d = torch.from_numpy(ranks).to(dev), torch.from_numpy(bg_ranks).to(dev)
    values = torch.empty((R, Cn, n), dtype=torch.int32, device=dev)
    bg_values = torch.empty((R, T, Cn), dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mseg_cell_order_stats_workspace_bytes(T, n, Cn, R), dtype=torch.uint8, device=dev)

    def order(cells_too=True):
        _lib.check(lib.mseg_cell_order_stats(lab_d.data_ptr(), _lib.PIX_U16, T, H, W,
                                             (off_d if cells_too else off0_d).data_ptr(), n if cells_too else 0,
                                             img_d.data_ptr(), _lib.PIX_U16, Cn, *strides, bbox.data_ptr(), R, ranks_d.data_ptr(),
                                             bg_ranks_d.data_ptr(), values.data_ptr(), bg_values.data_ptr(), status.data_ptr(),
                                             ws.data_ptr(), ws.numel(), st))

    box = bbox.cpu().numpy().astype(np.int64)
    box_px = float(((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])).sum()) / T
    print(f"stack {T} x {H} x {W}, {Cn} channels, {n} cells ({n / T:.0f} per frame), {box_px:.0f} box pixels per frame, "
          f"{R} ranks, workspace {ws.numel()} bytes")
    passes = (("order_stats", order), ("measure_2ch", measure), ("order_stats_background_only", lambda: order(False)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {name: [] for name, _ in passes}
    for _, fn in passes:
        fn()
    order()
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0, "a rank beyond a cell's pixels"
    for _ in range(a.reps):                                  # alternating: all passes see the same machine state
        for name, fn in passes:
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    order()
    torch.cuda.synchronize()
    res = {"frames": T, "height": H, "width": W, "channels": Cn, "ranks": R, "cells_per_frame": n / T,
           "box_pixels_per_frame": box_px}
    for name, v in ms.items():
        med = float(np.median(v))
        res[f"{name}_ms_per_frame"] = med / T
        res[f"{name}_ms_per_frame_min_max"] = [min(v) / T, max(v) / T]
        print(f"  {name:28s} {med / T:8.4f} ms per frame ({min(v) / T:.4f} .. {max(v) / T:.4f})")
    res["order_stats_over_measure"] = res["order_stats_ms_per_frame"] / res["measure_2ch_ms_per_frame"]
    res["cell_pass_ms_per_frame"] = res["order_stats_ms_per_frame"] - res["order_stats_background_only_ms_per_frame"]
    # what the background passes have to move per frame: labels and image once per channel in each of the two walks
    bg_bytes = 2 * Cn * H * W * (2 + 2)
    res["background_gb_per_s"] = bg_bytes / (res["order_stats_background_only_ms_per_frame"] * 1e-3) / 1e9
    print(f"  order_stats / measure_2ch = {res['order_stats_over_measure']:.2f}; cell pass (difference) "
          f"{res['cell_pass_ms_per_frame']:.4f} ms per frame; background passes {res['background_gb_per_s']:.0f} GB/s")
    if not a.no_host:
        for pct in (None, PERCENTILES):
            cells.measure_cells(lab_d, img_d, percentiles=pct)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            df = cells.measure_cells(lab_d, img_d, percentiles=pct)
            key = "measure_cells_percentiles_all_in_ms_per_frame" if pct else "measure_cells_all_in_ms_per_frame"
            res[key] = 1e3 * (time.perf_counter() - t0) / T
            print(f"  measure_cells(percentiles={pct}) all-in {res[key]:8.1f} ms per frame ({len(df)} rows, {len(df.columns)} columns)")
        k = int(off[1])
        t0 = time.perf_counter()
        want = oref.order_stats(labels[:1], off[:2], img[:1], box[:k], ranks[:, :k], bg_ranks[:, :1])
        res["numpy_restatement_s_per_frame_per_core"] = time.perf_counter() - t0
        print(f"  numpy restatement {res['numpy_restatement_s_per_frame_per_core']:8.1f} s per frame on one host core")
        assert want[2] == 0 and np.array_equal(values.cpu().numpy().view(np.uint32)[:, :, :k], want[0]), "device and restatement differ"
        assert np.array_equal(bg_values.cpu().numpy().view(np.uint32)[:, :1], want[1]), "device and restatement differ"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
