#!/usr/bin/env python3
"""Per-cell neighbourhood on the MI355X: device milliseconds per frame of mseg_cell_neighbors for R = 4, 8, 16
and 32 (HIP events around the whole call: initialisation, tile pass with the window scan, table pass, finish pass) and,
alternating in the same process, of mseg_cell_hull, the pass people know the time of; the all-in time of measure_cells with
and without neighbors=8; the numpy restatement (tests/neighbors_ref.py, windowed) on one frame for one host core.  Synthetic
stack as in tools/bench_cells.py: 2048^2 frames with about 2400 cells each, uint16 labels.  Prints one JSON line at the end.
GPU box only.
  python tools/bench_neighbors.py [--frames 16] [--reps 9] [--no-host]"""
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
import neighbors_ref as nref  # noqa: E402

RADII = (4, 8, 16, 32)


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
    _lib.check(lib.mseg_cell_measure(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, None, 0, 0, 0, 0, 0, 0,
                                     shape.data_ptr(), bbox.data_ptr(), None, None, None, None, st))
    box = bbox.cpu().numpy()
    row_off = np.zeros(n + 1, np.int64)
    np.cumsum(np.where(box[:, 2] > box[:, 0], box[:, 2].astype(np.int64) - box[:, 0] + 1, 0), out=row_off[1:])
    n_rows = int(row_off[-1])
    row_d = torch.from_numpy(row_off).to(dev)
    hull_out = torch.empty((10, n), dtype=torch.int64, device=dev)
    hull_status = torch.empty(1, dtype=torch.int32, device=dev)
    hull_ws = torch.empty(lib.mseg_cell_hull_workspace_bytes(n, n_rows), dtype=torch.uint8, device=dev)

    def hull():
        _lib.check(lib.mseg_cell_hull(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, bbox.data_ptr(),
                                      row_d.data_ptr(), n_rows, hull_out.data_ptr(), hull_status.data_ptr(), hull_ws.data_ptr(),
                                      hull_ws.numel(), st))

    cap = max(cells.MIN_TABLE, cells._pow2(8 * int(np.diff(off).max())))         # the table neighbors_raw starts with
    pair_cap = 8 * n
    out = torch.empty((9, n), dtype=torch.int64, device=dev)
    pairs = torch.empty((pair_cap, 5), dtype=torch.int32, device=dev)
    n_pairs = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(T, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mseg_cell_neighbors_workspace_bytes(T, n, cap), dtype=torch.uint8, device=dev)

    def neighbors(R):
        _lib.check(lib.mseg_cell_neighbors(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, R, cap, out.data_ptr(),
                                           pairs.data_ptr(), pair_cap, n_pairs.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                           ws.numel(), st))

    print(f"stack {T} x {H} x {W}, {n} cells ({n / T:.0f} per frame), pair tables of {cap} entries, {ws.numel() / 1e6:.1f} MB "
          "of workspace")
    fns = [("hull", hull)] + [(f"neighbors_r{R}", (lambda R=R: neighbors(R))) for R in RADII]
    res = {"frames": T, "height": H, "width": W, "cells_per_frame": n / T, "table_cap": cap}
    for name, fn in fns:
        fn()
        torch.cuda.synchronize()
        if name != "hull":
            assert not status.cpu().numpy().any(), "a pair table filled up"
            res[f"{name}_pairs_per_frame"] = int(n_pairs.cpu()[0]) / T
            assert res[f"{name}_pairs_per_frame"] * T <= pair_cap
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
        extra = f", {res[f'{name}_pairs_per_frame']:.0f} pairs per frame" if name != "hull" else ""
        print(f"  {name:16s} {med / T:8.4f} ms per frame ({min(v) / T:.4f} .. {max(v) / T:.4f}){extra}")
    if not a.no_host:
        for flag in (None, 8, None, 8):                      # alternating; the second round is the one reported
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            df = cells.measure_cells(lab_d, neighbors=flag)
            key = "measure_cells_neighbors_all_in_ms_per_frame" if flag else "measure_cells_all_in_ms_per_frame"
            res[key] = 1e3 * (time.perf_counter() - t0) / T
            print(f"  measure_cells(neighbors={flag}) all-in {res[key]:8.1f} ms per frame ({len(df)} rows, {len(df.columns)} columns)")
        t0 = time.perf_counter()
        contacts = cells.cell_contacts(lab_d, 8)
        res["cell_contacts_all_in_ms_per_frame"] = 1e3 * (time.perf_counter() - t0) / T
        print(f"  cell_contacts(radius=8) all-in {res['cell_contacts_all_in_ms_per_frame']:8.1f} ms per frame ({len(contacts)} rows)")
        t0 = time.perf_counter()
        want, rows = nref.neighbors(labels[:1], off[:2], 8, fn=nref.windowed)
        res["numpy_restatement_r8_s_per_frame_per_core"] = time.perf_counter() - t0
        print(f"  numpy restatement, R = 8 {res['numpy_restatement_r8_s_per_frame_per_core']:8.1f} s per frame on one host core")
        neighbors(8)
        got = out.cpu().numpy()[:, :int(off[1])]
        got_rows = pairs.cpu().numpy()[:int(n_pairs.cpu()[0])]
        got_rows = got_rows[got_rows[:, 0] == 0]
        got_rows = got_rows[np.lexsort((got_rows[:, 2], got_rows[:, 1]))]
        assert np.array_equal(got, want) and np.array_equal(got_rows, rows), "device and restatement differ"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
