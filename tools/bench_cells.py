#!/usr/bin/env python3
"""Per-cell table on the MI355X: device milliseconds per frame of the measure pass and the link pass against
the bytes each has to move, the all-in time of measure_cells, and the numpy restatement (tests/cells_ref.py) on one frame
for one host core.  Synthetic stack as in tools/bench_analysis.py: 2048^2 frames of 4 x 4 synthetic tiles with 150 cells
each (about 2400 cells per frame), uint16 labels, a 2-channel uint16 image.  Prints one JSON line at the end.  GPU box only.
  python tools/bench_cells.py [--frames 16] [--reps 5] [--all]"""
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
from bench_analysis import stack, timed  # noqa: E402
import cells_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--all", action="store_true", help="time measure_cells plain and with every column family on, --reps calls "
                    "each, instead of the numpy restatement")
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(7))
    labels = stack(rng, a.frames)
    T, H, W = labels.shape
    Cn = 2
    img = (rng.integers(0, 4096, (T, Cn, H, W)) + 2000 * (labels[:, None] > 0)).astype(np.uint16)
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lab_d = torch.from_numpy(labels.view(np.int16)).to(dev)
    img_d = torch.from_numpy(img.view(np.int16)).to(dev)
    off = ref.frame_tables(labels)
    n = int(off[-1])
    off_d = torch.from_numpy(off).to(dev)
    print(f"stack {T} x {H} x {W}, {n} cells ({n / T:.0f} per frame), {Cn} channels")
    shape = torch.empty((6, n), dtype=torch.int64, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    chs = torch.empty((2, Cn, n), dtype=torch.int64, device=dev)
    chm = torch.empty((2, Cn, n), dtype=torch.int32, device=dev)
    bgs = torch.empty((3, T, Cn), dtype=torch.int64, device=dev)
    bgm = torch.empty((2, T, Cn), dtype=torch.int32, device=dev)
    res = {}
    res["measure"] = timed(lambda: _lib.check(lib.mseg_cell_measure(
        lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, img_d.data_ptr(), _lib.PIX_U16, Cn, Cn * H * W, H * W,
        W, 1, shape.data_ptr(), bbox.data_ptr(), chs.data_ptr(), chm.data_ptr(), bgs.data_ptr(), bgm.data_ptr(), st)), a.reps)
    res["measure_shape_only"] = timed(lambda: _lib.check(lib.mseg_cell_measure(
        lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, None, 0, 0, 0, 0, 0, 0, shape.data_ptr(),
        bbox.data_ptr(), None, None, None, None, st)), a.reps)
    k = np.diff(off)
    cap = max(cells.MIN_TABLE, cells._pow2(4 * int((k[1:] + k[:-1]).max()))) if T > 1 else cells.MIN_TABLE
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    ovl = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(T, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mseg_cell_links_workspace_bytes(T, n, cap), dtype=torch.uint8, device=dev)
    res["link"] = timed(lambda: _lib.check(lib.mseg_cell_links(
        lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, cap, pred.data_ptr(), ovl.data_ptr(), status.data_ptr(),
        ws.data_ptr(), ws.numel(), st)), a.reps)
    assert not status.cpu().numpy().any(), "pair table full at the wrapper's starting size"
    # bytes a pass has to move per frame: labels once and every channel once; links: the frame and its predecessor + table
    bytes_measure = H * W * 2 * (1 + Cn)
    bytes_link = 2 * H * W * 2 * (T - 1) / T + 2 * 12 * cap * (T - 1) / T
    out = {"frames": T, "height": H, "width": W, "cells_per_frame": n / T, "channels": Cn, "table_entries": cap}
    for name, ms in res.items():
        b = bytes_link if name == "link" else (H * W * 2 if name == "measure_shape_only" else bytes_measure)
        out[f"{name}_ms_per_frame"] = ms / T
        out[f"{name}_gb_per_s"] = b / (ms / T * 1e-3) / 1e9
        print(f"  {name:20s} {ms / T:8.3f} ms per frame, {b / 1e6:7.1f} MB per frame -> {out[f'{name}_gb_per_s']:7.0f} GB/s")
    cells.measure_cells(lab_d, img_d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    df = cells.measure_cells(lab_d, img_d)
    out["measure_cells_all_in_ms_per_frame"] = 1e3 * (time.perf_counter() - t0) / T
    print(f"  measure_cells all-in {out['measure_cells_all_in_ms_per_frame']:8.1f} ms per frame ({len(df)} rows; host floats and "
          "tracks included)")
    if a.all:      # the host side: ``reps`` calls each after the warm-up above, plain and with every column family on
        every = dict(drift=4, flow=2, flow_tile=64, gap=1, hull=True, midline=True, percentiles=(5, 50), neighbors=3,
                     spots=1000, profile=4)
        no_spots = {k: v for k, v in every.items() if k != "spots"}
        for name, kw in (("plain", {}), ("all_but_spots", no_spots), ("all_on", every)):
            try:
                cells.measure_cells(lab_d, img_d, **kw)
            except TypeError as e:      # drift and spots in one table: commits before the column families raise here
                print(f"  measure_cells {name:13s} not timed: {type(e).__name__}: {e}")
                continue
            runs = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cells.measure_cells(lab_d, img_d, **kw)
                runs.append(1e3 * (time.perf_counter() - t0) / T)
            out[f"{name}_ms_per_frame_runs"] = [round(v, 3) for v in runs]
            out[f"{name}_ms_per_frame_median"] = float(np.median(runs))
            print(f"  measure_cells {name:13s} median {np.median(runs):8.2f} ms per frame, runs {min(runs):.2f} .. {max(runs):.2f}")
        print(json.dumps(out))
        return
    t0 = time.perf_counter()
    ref.table(labels[:2], img[:2], channels=list(range(Cn)), link=True)
    out["numpy_restatement_s_per_frame_per_core"] = (time.perf_counter() - t0) / 2
    print(f"  numpy restatement {out['numpy_restatement_s_per_frame_per_core']:8.1f} s per frame on one host core")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
