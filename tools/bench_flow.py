#!/usr/bin/env python3
"""Linking under a tile-wise displacement field on the MI355X: device milliseconds per frame pair of the tile
score surfaces (mseg_stack_flow) at r = 8 / 16 / 32 and B = 64 / 128, each beside the global surface (mseg_stack_drift) at
R = r, alternating in one process: both do (2r + 1)^2 / 64 word operations per pixel; of the link pass under a field beside
the one under a shift; the all-in time of measure_cells with drift and with drift + flow; and how many cells find their own
predecessor under plain, drift and flow linking.  Synthetic stack: a colony of rods (semi-axes 3 - 6 and 1.5 - 2.5 px) on a
jittered 24 px grid that expands about the centre of a 2048^2 frame by 0.6 % per frame (6 px per frame at 1000 px from the
centre) and jumps with a random walk of up to 4 px per axis and frame; a rod keeps its id.  The device values of one pair
must equal the numpy restatement (tests/flow_ref.py).  Prints one JSON line at the end.  GPU box only.
  python tools/bench_flow.py [--frames 16] [--reps 5]"""
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
from microbeseg_amd import _lib  # noqa: E402
from microbeseg_amd.inference import cells  # noqa: E402
import cells_ref as ref  # noqa: E402
import flow_ref as fref  # noqa: E402

SIZE, PITCH, JITTER, GROWTH, STEP, DRIFT = 2048, 24, 5, 0.006, 4, 16


def colony(rng, T):
    """-> (labels uint16 [T, 2048, 2048], applied jumps int32 [T, 2], row 0 = (0, 0))"""
    g = np.arange(-0.44 * SIZE, 0.44 * SIZE, PITCH)
    p = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2) + rng.uniform(-JITTER, JITTER, (len(g) ** 2, 2))
    a, b, th = rng.uniform(3, 6, len(p)), rng.uniform(1.5, 2.5, len(p)), rng.uniform(0, np.pi, len(p))
    jump = np.zeros((T, 2), np.int32)
    jump[1:] = rng.integers(-STEP, STEP + 1, (T - 1, 2))
    total = np.cumsum(jump, axis=0)
    lab = np.zeros((T, SIZE, SIZE), np.uint16)
    yy, xx = np.mgrid[-7:8, -7:8]
    for t in range(T):
        centres = (SIZE - 1) / 2 + (1 + GROWTH) ** t * p + total[t]
        for k, (cy, cx) in enumerate(centres, start=1):
            y0, x0 = int(round(cy)), int(round(cx))
            if not (7 <= y0 < SIZE - 7 and 7 <= x0 < SIZE - 7):
                continue
            dy, dx = yy + y0 - cy, xx + x0 - cx
            u, v = dy * np.cos(th[k - 1]) + dx * np.sin(th[k - 1]), -dy * np.sin(th[k - 1]) + dx * np.cos(th[k - 1])
            box = lab[t, y0 - 7:y0 + 8, x0 - 7:x0 + 8]
            box[((u / a[k - 1]) ** 2 + (v / b[k - 1]) ** 2 <= 1) & (box == 0)] = k
    return lab, jump


def event_ms(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def own_predecessor(df):
    """-> (cells whose id is also in the previous frame, those of them whose pred_label is their own id)"""
    seen = set(zip(df["frame"], df["label"]))
    both = np.array([(t - 1, l) in seen for t, l in zip(df["frame"], df["label"])])
    return int(both.sum()), int((both & (df["pred_label"] == df["label"]).to_numpy()).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no MI355X visible: nothing to measure")
    rng = np.random.Generator(np.random.PCG64(7))
    labels, jump = colony(rng, a.frames)
    T, H, W = labels.shape
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lab_d = torch.from_numpy(labels.view(np.int16)).to(dev)
    off = ref.frame_tables(labels)
    n = int(off[-1])
    off_d = torch.from_numpy(off).to(dev)
    present = sum(len(np.unique(f)) - 1 for f in labels) / T
    print(f"stack {T} x {H} x {W}, {present:.0f} cells per frame, growth {GROWTH} per frame, jumps up to {STEP} px")
    out = {"frames": T, "height": H, "width": W, "cells_per_frame": present, "growth": GROWTH, "max_step": STEP}
    shift = cells.pick_drift(cells.drift_raw(lab_d, _lib.PIX_U16, off, DRIFT))
    print(f"  global shifts equal the applied jumps for {int((shift == jump).all(axis=1).sum()) - 1} of {T - 1} pairs")
    shift_d = torch.from_numpy(shift).to(dev)

    # ---- the tile surfaces beside the global surface at the same radius, alternating ----
    ws = torch.empty(lib.mseg_stack_flow_workspace_bytes(T, H, W), dtype=torch.uint8, device=dev)
    words = (W + 63) // 64
    for r in (8, 16, 32):
        side = 2 * r + 1
        whole = torch.empty((T - 1, side, side), dtype=torch.int32, device=dev)
        drift = lambda: _lib.check(lib.mseg_stack_drift(lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), r,
                                                        whole.data_ptr(), ws.data_ptr(), ws.numel(), st))
        calls, surfaces = {"drift": drift}, {}
        for B in (64, 128):
            surfaces[B] = torch.empty((T - 1, -(-H // B), -(-W // B), side, side), dtype=torch.int32, device=dev)
            calls[f"flow_b{B}"] = lambda B=B: _lib.check(lib.mseg_stack_flow(
                lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), B, r, shift_d.data_ptr(), surfaces[B].data_ptr(),
                ws.data_ptr(), ws.numel(), st))
        ms = {name: [] for name in calls}
        for rep in range(a.reps + 1):                     # the first round warms up
            for name, call in calls.items():
                ms[name].append(event_ms(call))
        ops = side * side * H * words                     # 64-bit AND + popcount operations per pair, either kernel
        for name, v in ms.items():
            per_pair = float(np.median(v[1:])) / (T - 1)
            out[f"{name}_r{r}_ms_per_pair"] = per_pair
            out[f"{name}_r{r}_ms_per_pair_range"] = [min(v[1:]) / (T - 1), max(v[1:]) / (T - 1)]
            out[f"{name}_r{r}_gwordops_per_s"] = ops / (per_pair * 1e-3) / 1e9
            print(f"  r = {r:2d} {name:10s} {per_pair:8.3f} ms per pair ({min(v[1:]) / (T - 1):.3f} .. {max(v[1:]) / (T - 1):.3f}), "
                  f"{ops / 1e6:7.1f} M word operations -> {out[f'{name}_r{r}_gwordops_per_s']:7.0f} G/s")
        # with base 0 the tile surfaces sum to the global one; here: the sums of both tile sizes agree
        sums = [s.cpu().numpy().view(np.uint32).sum(axis=(1, 2), dtype=np.int64) for s in surfaces.values()]
        assert np.array_equal(sums[0], sums[1]), "the tile surfaces of 64 and 128 px do not sum to the same surface"

    # ---- one pair against the restatement ----
    t0 = time.perf_counter()
    want = fref.scores(labels[:2], off[:3], shift[:2], 8, 64)
    out["numpy_restatement_s_per_pair_r8"] = time.perf_counter() - t0
    got = cells.flow_raw(lab_d[:2], _lib.PIX_U16, off[:3], shift[:2], 8, 64)
    assert np.array_equal(got, want), "device tile scores differ from the restatement"
    field2 = cells.pick_flow(got, shift[:2])
    assert np.array_equal(field2, fref.pick(want, shift[:2]))
    links2 = cells.link_raw(lab_d[:2], _lib.PIX_U16, off[:3], field=field2, tile=64)
    assert all(np.array_equal(x, y) for x, y in zip(links2, fref.links_field(labels[:2], off[:3], field2, 64)))
    print(f"  numpy restatement r = 8, B = 64: {out['numpy_restatement_s_per_pair_r8']:6.1f} s per pair (scores, field and links "
          f"equal)")

    # ---- links under a shift and under a field, alternating ----
    field = cells.pick_flow(cells.flow_raw(lab_d, _lib.PIX_U16, off, shift, 8, 64), shift)
    field_d = torch.from_numpy(field).to(dev)
    k = np.diff(off)
    cap = max(cells.MIN_TABLE, cells._pow2(4 * int((k[1:] + k[:-1]).max())))
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    ovl = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(T, dtype=torch.int32, device=dev)
    lws = torch.empty(lib.mseg_cell_links_workspace_bytes(T, n, cap), dtype=torch.uint8, device=dev)
    moved = lambda: _lib.check(lib.mseg_cell_links_shifted(
        lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, cap, shift_d.data_ptr(), pred.data_ptr(),
        ovl.data_ptr(), status.data_ptr(), lws.data_ptr(), lws.numel(), st))
    under = lambda: _lib.check(lib.mseg_cell_links_field(
        lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, cap, 64, field_d.data_ptr(), pred.data_ptr(),
        ovl.data_ptr(), status.data_ptr(), lws.data_ptr(), lws.numel(), st))
    moved(), under()
    torch.cuda.synchronize()
    ms = {"links_shifted": [], "links_field": []}
    for _ in range(a.reps):
        ms["links_shifted"].append(event_ms(moved))
        ms["links_field"].append(event_ms(under))
    assert not status.cpu().numpy().any(), "pair table full at the wrapper's starting size"
    for name, v in ms.items():
        out[f"{name}_ms_per_pair"] = float(np.median(v)) / (T - 1)
        print(f"  {name:20s} {out[f'{name}_ms_per_pair']:8.4f} ms per pair (table of {cap} entries)")

    # ---- measure_cells all-in, and what the field is for ----
    tables = {}
    for name, kw in 2 * (("drift", {"drift": DRIFT}), ("flow", {"drift": DRIFT, "flow": 8})):       # the first round warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tables[name] = cells.measure_cells(lab_d, **kw)
        out[f"measure_cells_{name}_all_in_ms_per_frame"] = 1e3 * (time.perf_counter() - t0) / T
    tables["plain"] = cells.measure_cells(lab_d)
    for name in ("plain", "drift", "flow"):
        both, own = own_predecessor(tables[name])
        out[f"own_predecessor_{name}"], out[f"tracks_{name}"] = own, int(tables[name]["track_id"].nunique())
        print(f"  {name:5s} linking: {own} of {both} cells find their own predecessor, {out[f'tracks_{name}']} tracks")
    out["in_both_frames"] = both
    print(f"  measure_cells all-in with drift = {DRIFT}: {out['measure_cells_drift_all_in_ms_per_frame']:7.1f} ms per frame, "
          f"with flow = 8 as well: {out['measure_cells_flow_all_in_ms_per_frame']:7.1f} ms per frame")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
