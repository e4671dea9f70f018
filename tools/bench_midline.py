#!/usr/bin/env python3
"""Per-cell midline on the MI355X: device milliseconds per frame of mseg_cell_midline (HIP events around the
whole call: clearing the bit rows, fill pass, thin-and-measure pass; with and without the skeleton image) and, alternating in
the same process for scale, of mseg_cell_hull and of mseg_cell_measure shape-only, the passes that read the same label bytes;
the all-in time of measure_cells with and without midline; the numpy restatement (tests/midline_ref.py) on one frame for one
host core, and the assertion that the device's frame 0 equals it.  Synthetic stack as in tools/bench_hull.py: 2048^2 frames
with about 2400 cells each, uint16 labels.  Prints one JSON line at the end.  GPU box only.
  python tools/bench_midline.py [--frames 16] [--reps 9] [--no-host]"""
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
import midline_ref as mref  # noqa: E402


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
    box = bbox.cpu().numpy().astype(np.int64)
    present = box[:, 2] > box[:, 0]
    row_off, word_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    np.cumsum(np.where(present, box[:, 2] - box[:, 0] + 1, 0), out=row_off[1:])
    np.cumsum(np.where(present, (box[:, 2] - box[:, 0] + 2) * ((box[:, 3] - box[:, 1] + 2 + 63) // 64), 0), out=word_off[1:])
    n_rows, n_words = int(row_off[-1]), int(word_off[-1])
    row_d, word_d = torch.from_numpy(row_off).to(dev), torch.from_numpy(word_off).to(dev)
    hull_out = torch.empty((10, n), dtype=torch.int64, device=dev)
    out = torch.empty((12, n), dtype=torch.int64, device=dev)
    skel = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    hull_ws = torch.empty(lib.mseg_cell_hull_workspace_bytes(n, n_rows), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.mseg_cell_midline_workspace_bytes(n, n_words), dtype=torch.uint8, device=dev)

    def hull():
        _lib.check(lib.mseg_cell_hull(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, bbox.data_ptr(),
                                      row_d.data_ptr(), n_rows, hull_out.data_ptr(), status.data_ptr() + 4, hull_ws.data_ptr(),
                                      hull_ws.numel(), st))

    def midline(image=None):
        _lib.check(lib.mseg_cell_midline(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, bbox.data_ptr(),
                                         word_d.data_ptr(), n_words, out.data_ptr(), image, status.data_ptr(), ws.data_ptr(),
                                         ws.numel(), st))

    def midline_skeleton():
        midline(skel.data_ptr())

    print(f"stack {T} x {H} x {W}, {n} cells ({n / T:.0f} per frame), {n_words} words ({n_words / max(n, 1):.1f} per cell)")
    passes = (("midline", midline), ("midline_skeleton", midline_skeleton), ("hull", hull), ("measure_shape_only", measure))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {name: [] for name, _ in passes}
    for _, fn in passes:
        fn()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0], "a cell outside its own box, or the round cap"
    for _ in range(a.reps):                                  # alternating: all passes see the same machine state
        for name, fn in passes:
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    res = {"frames": T, "height": H, "width": W, "cells_per_frame": n / T, "words_per_cell": n_words / max(n, 1)}
    for name, v in ms.items():
        med = float(np.median(v))
        res[f"{name}_ms_per_frame"] = med / T
        res[f"{name}_ms_per_frame_min_max"] = [min(v) / T, max(v) / T]
        print(f"  {name:20s} {med / T:8.4f} ms per frame ({min(v) / T:.4f} .. {max(v) / T:.4f})")
    res["midline_over_hull"] = res["midline_ms_per_frame"] / res["hull_ms_per_frame"]
    rounds = out[5].cpu().numpy()
    res["rounds_mean_max"] = [float(rounds[rounds > 0].mean()), int(rounds.max())]
    if not a.no_host:
        for flag in (False, True):
            cells.measure_cells(lab_d, midline=flag)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            df = cells.measure_cells(lab_d, midline=flag)
            key = "measure_cells_midline_all_in_ms_per_frame" if flag else "measure_cells_all_in_ms_per_frame"
            res[key] = 1e3 * (time.perf_counter() - t0) / T
            print(f"  measure_cells(midline={flag}) all-in {res[key]:8.1f} ms per frame ({len(df)} rows, {len(df.columns)} columns)")
        res["midline_length_nan_fraction"] = float(df["midline_length"].isna().mean())
        t0 = time.perf_counter()
        want, want_skel = mref.midline(labels[:1], off[:2])
        res["numpy_restatement_s_per_frame_per_core"] = time.perf_counter() - t0
        print(f"  numpy restatement {res['numpy_restatement_s_per_frame_per_core']:8.1f} s per frame on one host core")
        midline_skeleton()
        assert np.array_equal(out.cpu().numpy()[:, :int(off[1])], want), "device and restatement differ"
        assert np.array_equal(skel[0].cpu().numpy(), want_skel[0]), "skeleton image and restatement differ"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
