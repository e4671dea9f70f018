#!/usr/bin/env python3
"""Per-cell outline measures on the MI355X: device milliseconds per frame of mseg_cell_hull (HIP events around
the whole call: table initialisation, label pass, hull pass) and, alternating in the same process, of mseg_cell_measure
shape-only, the pass that reads the same label bytes; the all-in time of measure_cells with and without hull; the numpy
restatement (tests/hull_ref.py, the monotone chain for every cell) on one frame for one host core.  Synthetic stack as in
tools/bench_cells.py: 2048^2 frames with about 2400 cells each, uint16 labels.  Prints one JSON line at the end.  GPU box only.
  python tools/bench_hull.py [--frames 16] [--reps 9] [--no-host]"""
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
import hull_ref as href  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-host", action="store_true", help="device times only (for a profiler run)")
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(7))
    labels = stack(rng, a.frames)
    T, H, W = labels.shape
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lab_d = torch.from_numpy(labels.view(np.int16)).to(dev)
    off = ref.frame_tables(labels)
    n = int(off[-1])
    off_d = torch.from_numpy(off).to(dev)
    shape = torch.empty((6, n), dtype=torch.int64, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)

    def measure():
        _lib.check(lib.mseg_cell_measure(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, None, 0, 0, 0, 0, 0, 0,
                                         shape.data_ptr(), bbox.data_ptr(), None, None, None, None, st))

    measure()
    box = bbox.cpu().numpy()
    row_off = np.zeros(n + 1, np.int64)
    np.cumsum(np.where(box[:, 2] > box[:, 0], box[:, 2].astype(np.int64) - box[:, 0] + 1, 0), out=row_off[1:])
    n_rows = int(row_off[-1])
    row_d = torch.from_numpy(row_off).to(dev)
    out = torch.empty((10, n), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mseg_cell_hull_workspace_bytes(n, n_rows), dtype=torch.uint8, device=dev)

    def hull():
        _lib.check(lib.mseg_cell_hull(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, bbox.data_ptr(),
                                      row_d.data_ptr(), n_rows, out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                      st))

    print(f"stack {T} x {H} x {W}, {n} cells ({n / T:.0f} per frame), {n_rows} corner rows ({n_rows / max(n, 1):.1f} per cell)")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {"hull": [], "measure_shape_only": []}
    for fn in (hull, measure):
        fn()
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0, "a cell outside its own box"
    for _ in range(a.reps):                                  # alternating: both passes see the same machine state
        for name, fn in (("hull", hull), ("measure_shape_only", measure)):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    res = {"frames": T, "height": H, "width": W, "cells_per_frame": n / T, "rows_per_cell": n_rows / max(n, 1)}
    label_bytes = H * W * 2                                  # what either pass has to move per frame: the labels, once
    for name, v in ms.items():
        med = float(np.median(v))
        res[f"{name}_ms_per_frame"] = med / T
        res[f"{name}_ms_per_frame_min_max"] = [min(v) / T, max(v) / T]
        res[f"{name}_gb_per_s"] = label_bytes / (med / T * 1e-3) / 1e9
        print(f"  {name:20s} {med / T:8.4f} ms per frame ({min(v) / T:.4f} .. {max(v) / T:.4f}), {label_bytes / 1e6:.1f} MB of "
              f"labels per frame -> {res[f'{name}_gb_per_s']:7.0f} GB/s")
    if not a.no_host:
        for flag in (False, True):
            cells.measure_cells(lab_d, hull=flag)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            df = cells.measure_cells(lab_d, hull=flag)
            key = "measure_cells_hull_all_in_ms_per_frame" if flag else "measure_cells_all_in_ms_per_frame"
            res[key] = 1e3 * (time.perf_counter() - t0) / T
            print(f"  measure_cells(hull={flag}) all-in {res[key]:8.1f} ms per frame ({len(df)} rows, {len(df.columns)} columns)")
        t0 = time.perf_counter()
        want = href.hull(labels[:1], off[:2], brute_corners=0)
        res["numpy_restatement_s_per_frame_per_core"] = time.perf_counter() - t0
        print(f"  numpy restatement {res['numpy_restatement_s_per_frame_per_core']:8.1f} s per frame on one host core")
        assert np.array_equal(out.cpu().numpy()[:, :int(off[1])], want), "device and restatement differ"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
