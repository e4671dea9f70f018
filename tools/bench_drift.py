#!/usr/bin/env python3
"""Drift-compensated linking on the MI355X: device milliseconds per frame pair of the drift score surface at
R = 16 / 32 / 64, of the plain and the shifted link pass (alternating in one process), the all-in time of measure_cells with
and without drift, and the numpy restatement (tests/drift_ref.py) of one score surface on one host core.  Synthetic stack:
a 2560^2 canvas of 5 x 5 synthetic tiles with 150 cells each; frame t is the 2048^2 window of the canvas moved by a known
random walk (up to 12 px per axis and frame), about 2400 cells per frame, uint16 labels, a 2-channel uint16 image.  The
picked shifts must equal the applied ones.  Prints one JSON line at the end.  GPU box only.
  python tools/bench_drift.py [--frames 16] [--reps 5]"""
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
import drift_ref as dref  # noqa: E402

SIZE, MARGIN, STEP = 2048, 256, 12


def drifting(rng, T):
    """-> (labels uint16 [T, 2048, 2048], applied shifts int32 [T, 2], row 0 = (0, 0))"""
    canvas = stack(rng, 1, tiles=5)[0]
    shift = np.zeros((T, 2), np.int32)
    shift[1:] = rng.integers(-STEP, STEP + 1, (T - 1, 2))
    total = np.cumsum(shift, axis=0)
    assert np.abs(total).max() <= MARGIN
    lab = np.stack([canvas[MARGIN - y:MARGIN - y + SIZE, MARGIN - x:MARGIN - x + SIZE] for y, x in total])
    return np.ascontiguousarray(lab), shift


def event_ms(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no MI355X visible: nothing to measure")
    rng = np.random.Generator(np.random.PCG64(7))
    labels, applied = drifting(rng, a.frames)
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
    present = sum(len(np.unique(f)) - 1 for f in labels) / T
    print(f"stack {T} x {H} x {W}, {present:.0f} cells per frame in view, tables of {n / T:.0f} ids per frame")
    out = {"frames": T, "height": H, "width": W, "cells_per_frame": present, "max_step": STEP}

    # ---- the score surface ----
    ws = torch.empty(lib.mseg_stack_drift_workspace_bytes(T, H, W), dtype=torch.uint8, device=dev)
    words = (W + 63) // 64
    for R in (16, 32, 64):
        side = 2 * R + 1
        scores = torch.empty((T - 1, side, side), dtype=torch.int32, device=dev)
        call = lambda: _lib.check(lib.mseg_stack_drift(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), R,
                                                       scores.data_ptr(), ws.data_ptr(), ws.numel(), st))
        call()
        torch.cuda.synchronize()
        ms = float(np.median([event_ms(call) for _ in range(a.reps)])) / (T - 1)
        picked = cells.pick_drift(scores.cpu().numpy().view(np.uint32))
        assert np.array_equal(picked, applied), "the picked shifts are not the applied ones"
        ops = side * side * H * words                     # 64-bit AND + popcount operations per pair (rows moved out included)
        out[f"drift_r{R}_ms_per_pair"] = ms
        out[f"drift_r{R}_gwordops_per_s"] = ops / (ms * 1e-3) / 1e9
        print(f"  mseg_stack_drift R = {R:3d}: {ms:8.3f} ms per pair, {ops / 1e6:8.1f} M word operations -> "
              f"{out[f'drift_r{R}_gwordops_per_s']:7.0f} G/s")

    # ---- plain and shifted links, alternating ----
    k = np.diff(off)
    cap = max(cells.MIN_TABLE, cells._pow2(4 * int((k[1:] + k[:-1]).max())))
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    ovl = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(T, dtype=torch.int32, device=dev)
    lws = torch.empty(lib.mseg_cell_links_workspace_bytes(T, n, cap), dtype=torch.uint8, device=dev)
    shift_d = torch.from_numpy(applied).to(dev)
    plain = lambda: _lib.check(lib.mseg_cell_links(
        lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, cap, pred.data_ptr(), ovl.data_ptr(), status.data_ptr(),
        lws.data_ptr(), lws.numel(), st))
    moved = lambda: _lib.check(lib.mseg_cell_links_shifted(
        lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, cap, shift_d.data_ptr(), pred.data_ptr(),
        ovl.data_ptr(), status.data_ptr(), lws.data_ptr(), lws.numel(), st))
    plain(), moved()
    torch.cuda.synchronize()
    ms = {"links": [], "links_shifted": []}
    for _ in range(a.reps):
        ms["links"].append(event_ms(plain))
        ms["links_shifted"].append(event_ms(moved))
    assert not status.cpu().numpy().any(), "pair table full at the wrapper's starting size"
    for name, v in ms.items():
        out[f"{name}_ms_per_pair"] = float(np.median(v)) / (T - 1)
        print(f"  {name:20s} {out[f'{name}_ms_per_pair']:8.4f} ms per pair (table of {cap} entries)")
    out["table_entries"] = cap

    # ---- measure_cells all-in ----
    for name, drift in (("measure_cells", None), ("measure_cells_drift32", 32), ("measure_cells", None),
                        ("measure_cells_drift32", 32)):          # the first round warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        df = cells.measure_cells(lab_d, img_d, drift=drift)
        out[f"{name}_all_in_ms_per_frame"] = 1e3 * (time.perf_counter() - t0) / T
    moved_tracks, plain_tracks = df["track_id"].nunique(), cells.measure_cells(lab_d, drift=None)["track_id"].nunique()
    out["tracks_with_drift"], out["tracks_without"] = int(moved_tracks), int(plain_tracks)
    print(f"  measure_cells all-in {out['measure_cells_all_in_ms_per_frame']:8.1f} ms per frame, with drift = 32 "
          f"{out['measure_cells_drift32_all_in_ms_per_frame']:8.1f} ms per frame ({len(df)} rows; {moved_tracks} tracks "
          f"under the drift, {plain_tracks} without)")

    # ---- the numpy restatement of one surface ----
    t0 = time.perf_counter()
    want = dref.scores(labels[:2], off[:3], 32)
    out["numpy_restatement_s_per_pair_r32"] = time.perf_counter() - t0
    scores = cells.drift_raw(lab_d[:2], _lib.PIX_U16, off[:3], 32)
    assert np.array_equal(scores, want), "device scores differ from the restatement"
    print(f"  numpy restatement R = 32: {out['numpy_restatement_s_per_pair_r32']:8.1f} s per pair on one host core (equal)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
