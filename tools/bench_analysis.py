#!/usr/bin/env python3
"""Analysis / Export on the MI355X: device milliseconds per frame of each stage (fill, outline, relabel,
stats, overlay), the all-in time per frame of export_local (host means and the five files included), and the CPU
restatement (tests/analysis_ref.py) on one frame for context.  Synthetic stack: utils/synth.py masks (512^2 tiles, 150 cells
each, 4 x 4 tiles per 2048^2 frame) -> label_polygons -> ROI records.  GPU box only.
  python tools/bench_analysis.py [--frames 16] [--reps 5]"""
import argparse
import ctypes as C
import pathlib
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from microbeseg_amd import _lib  # noqa: E402
from microbeseg_amd.inference import analysis as A  # noqa: E402
from microbeseg_amd.inference.infer import InferWorker  # noqa: E402
from microbeseg_amd.inference.result_export import export_local  # noqa: E402
from microbeseg_amd.utils.synth import synth_instance_mask  # noqa: E402
import analysis_ref as ref  # noqa: E402


def stack(rng, T, tiles=4, tile=512, cells=150):
    base = [synth_instance_mask(rng, tile, cells).astype(np.int64) for _ in range(tiles * tiles)]
    out = np.zeros((T, tiles * tile, tiles * tile), np.uint16)
    for t in range(T):
        order = rng.permutation(len(base))
        nxt = 0
        for i, k in enumerate(order):
            m = base[k][:, ::-1] if (t + i) % 2 else base[k]
            y, x = (i // tiles) * tile, (i % tiles) * tile
            out[t, y:y + tile, x:x + tile] = np.where(m > 0, m + nxt, 0)
            nxt += int(m.max())
    return out


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(7))
    T = a.frames
    labels = stack(rng, T)
    T, H, W = labels.shape
    worker = InferWorker.__new__(InferWorker)
    worker.channel = 0
    rois = [roi for t in range(T) for roi in worker.polygon_rois(labels[t], t)]
    img = (rng.integers(0, 4096, labels.shape) + 2000 * (labels > 0)).astype(np.uint16)
    print(f"stack {T} x {H} x {W}, {len(rois)} polygons ({len(rois) / T:.0f} per frame)")

    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc, voff, frame = A._csr(rois, H, W)
    n = len(frame)
    rc_d, voff_d, fr_d = (torch.from_numpy(v).to(dev) for v in (rc, voff, frame))
    filled = torch.empty((T, H, W), dtype=torch.int32, device=dev)
    outl = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    lab = torch.empty((T, H, W), dtype=torch.int32, device=dev)
    k = torch.empty(T, dtype=torch.int32, device=dev)
    ws_fill = A._ws(lib.mseg_roi_fill_workspace_bytes(n), dev)
    ws_rl = A._ws(lib.mseg_stack_relabel_workspace_bytes(T, H, W), dev)
    res = {}
    res["fill"] = timed(lambda: _lib.check(lib.mseg_roi_fill(rc_d.data_ptr(), voff_d.data_ptr(), fr_d.data_ptr(), n, T, H,
                                                             W, filled.data_ptr(), ws_fill.data_ptr(), ws_fill.numel(),
                                                             st)), a.reps)
    res["outline"] = timed(lambda: _lib.check(lib.mseg_roi_outline(rc_d.data_ptr(), voff_d.data_ptr(), fr_d.data_ptr(), n,
                                                                   int(voff[-1]), T, H, W, outl.data_ptr(), st)), a.reps)
    res["relabel"] = timed(lambda: _lib.check(lib.mseg_stack_relabel(filled.data_ptr(), 2, T, H, W, lab.data_ptr(),
                                                                     k.data_ptr(), ws_rl.data_ptr(), ws_rl.numel(), st)),
                           a.reps)
    kh = k.cpu().numpy().astype(np.int64)
    off = np.zeros(T + 1, np.int64)
    np.cumsum(kh, out=off[1:])
    nl = int(off[-1])
    off_d = torch.from_numpy(off).to(dev)
    area = torch.empty(nl, dtype=torch.int64, device=dev)
    major, minor = (torch.empty(nl, dtype=torch.float64, device=dev) for _ in range(2))
    total = torch.empty(T, dtype=torch.int64, device=dev)
    ws_st = A._ws(lib.mseg_region_stats_workspace_bytes(nl), dev)
    res["stats"] = timed(lambda: _lib.check(lib.mseg_region_stats(lab.data_ptr(), T, H, W, off_d.data_ptr(), nl,
                                                                  area.data_ptr(), major.data_ptr(), minor.data_ptr(),
                                                                  total.data_ptr(), ws_st.data_ptr(), ws_st.numel(), st)),
                         a.reps)
    img_d = torch.from_numpy(img.view(np.int16)).to(dev)
    ov = torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev)
    ws_ov = A._ws(lib.mseg_overlay_workspace_bytes(), dev)
    res["overlay"] = timed(lambda: _lib.check(lib.mseg_overlay_rgb(img_d.data_ptr(), 1, T, H, W, 1, outl.data_ptr(),
                                                                   ov.data_ptr(), ws_ov.data_ptr(), ws_ov.numel(), st)),
                           a.reps)
    for name, ms in res.items():
        print(f"  {name:8s} {ms / T:8.3f} ms per frame ({ms:.2f} ms for the stack)")
    print(f"  device   {sum(res.values()) / T:8.3f} ms per frame")

    with tempfile.TemporaryDirectory() as d:
        export_local(img, rois, pathlib.Path(d) / "warm", "x.tif", text_output=lambda s: None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        export_local(img, rois, pathlib.Path(d) / "run", "x.tif", text_output=lambda s: None)
        torch.cuda.synchronize()
        t_all = (time.perf_counter() - t0) / T
    print(f"  export_local all-in {1e3 * t_all:8.1f} ms per frame (ROI parsing, device pipeline, host means, 5 files)")

    r0 = [roi for roi in rois if roi["theT"] == 0]
    t0 = time.perf_counter()
    coords = [(0,) + tuple(np.asarray(v) for v in ref.make_coordinates(r["points"], W, H)) for r in r0]
    m, _ = ref.rois_to_masks(coords, 1, H, W)
    ref.analyze(m)
    print(f"  CPU restatement {time.perf_counter() - t0:8.1f} s for one frame")


if __name__ == "__main__":
    main()
