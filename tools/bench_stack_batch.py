#!/usr/bin/env python3
"""Stacks of SMALL frames through InferWorker.infer_stack: frame by frame (frame_batch = 1, the default path) against
groups (frame_batch = 0, auto) — fp32 and bf16, 256^2 and 512^2, in one process.

Model: DU [64, 1024] bn / relu with seeded weights (there are no checkpoints offline).  Input: uint16 stacks generated from
a seed.  An untrained network predicts one blob, so realistic distance maps are handed to the post-processing through
InferWorker.prediction_hook, the way bench.py does; the network still runs on every frame.  After both settings are warm
the runs alternate (1, auto, 1, auto, ...); the time is the wall clock around infer_stack, which returns synchronised; the
median over the repeats is reported.  The frame_batch = 1 run is the yardstick: nothing on that path knows about groups.

One JSON line: per size and precision frames/s and Mpx/s of both settings, their ratio, whether the masks are equal, and
the split of one group into network and post-processing (device time of each alone, stream-synchronised).

``--postproc_only N``: nothing but ``--calls`` batched post-processing calls on N frames (after one warm-up call) — for a
kernel trace that counts the launches per group (rocprofv3 --kernel-trace --stats -- python tools/bench_stack_batch.py ...).
"""
import argparse
import json
import pathlib
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

FILTERS = (64, 1024)
NMAPS = 8       # different synthetic predictions per size, handed out round robin


def make_worker(tmp, dev):
    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.utils.unets import build_unet
    torch.manual_seed(0)
    net = build_unet("DU", "relu", "conv", "bn", dev, 1, ch_out=1, filters=FILTERS)
    base = pathlib.Path(tmp) / "distance_model_00"
    torch.save(net.state_dict(), str(base) + ".pth")
    with open(str(base) + ".json", "w") as f:
        json.dump({"architecture": ["DU", "conv", "relu", "bn", list(FILTERS)], "label_type": "distance"}, f)
    return InferWorker(model=str(base), device=str(dev), ths=(0.10, 0.45))


def make_maps(S, seed, dev):
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    maps = []
    for _ in range(NMAPS):
        cell, border = synth.synth_prediction_maps(rng, S, S, max(1, int(2500 * (S / 2048.0) ** 2)), rmin=5.0, rmax=13.0)
        maps.append((torch.from_numpy(border).to(dev)[None, None], torch.from_numpy(cell).to(dev)[None, None]))
    return maps


def median(v):
    return float(np.median(np.asarray(v)))


def time_device(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return 1e3 * median(t)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames256", type=int, default=512)
    ap.add_argument("--frames512", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--frame_batch", type=int, default=0, help="the group setting compared with 1 (0 = auto)")
    ap.add_argument("--postproc_only", type=int, default=0, help="N: only batched post-processing calls on N 256^2 frames")
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from microbeseg_amd.inference import postprocessing as pp
    from microbeseg_amd.inference.infer import frame_batch_for

    if args.postproc_only:
        n, S = args.postproc_only, 256
        maps = make_maps(S, args.seed, dev)
        border = torch.cat([maps[i % NMAPS][0] for i in range(n)])[:, 0]
        cell = torch.cat([maps[i % NMAPS][1] for i in range(n)])[:, 0]
        for _ in range(1 + args.calls):
            labels, n_inst, status = pp.distance_postprocessing_batch_device(border, cell, 0.45, 0.10)
        torch.cuda.synchronize()
        print(json.dumps({"postproc_only": n, "calls_after_warmup": args.calls, "instances": n_inst.cpu().tolist()[:8],
                          "status": status.cpu().tolist()[:8]}))
        return

    result = {"model": "DU [64,1024] bn/relu, seeded weights", "input": "uint16 stacks from a seed; synthetic distance maps "
              "injected through prediction_hook", "repeats": args.repeats, "timing": "wall clock around infer_stack, median"}
    with tempfile.TemporaryDirectory() as tmp:
        worker = make_worker(tmp, dev)
        for S, T in ((256, args.frames256), (512, args.frames512)):
            if T <= 0:
                continue
            rng = np.random.Generator(np.random.PCG64(args.seed + S))
            stack = rng.integers(0, 60000, size=(T, S, S)).astype(np.uint16)
            maps = make_maps(S, args.seed + S, dev)
            count = [0]

            def hook(pred):
                assert tuple(pred[0].shape) == (1, 1, S, S)
                count[0] += 1
                return maps[(count[0] - 1) % NMAPS]
            worker.prediction_hook = hook
            fb = frame_batch_for(S, S, args.frame_batch)
            entry = {"frames": T, "frame_batch": fb}
            for prec in ("fp32", "bf16"):
                worker.precision = prec
                for setting in (1, args.frame_batch):                    # warm both (buffers, weight packs, workspaces)
                    worker.frame_batch = setting
                    count[0] = 0
                    worker.infer_stack(stack[:2 * max(1, fb)])
                torch.cuda.synchronize()
                times, masks = {1: [], args.frame_batch: []}, {}
                for _ in range(args.repeats):
                    for setting in (1, args.frame_batch):
                        worker.frame_batch = setting
                        count[0] = 0
                        t0 = time.perf_counter()
                        masks[setting] = worker.infer_stack(stack)
                        times[setting].append(time.perf_counter() - t0)
                t1, tg = median(times[1]), median(times[args.frame_batch])
                # one group alone: network (normalisation + forward at batch fb) and batched post-processing
                with torch.no_grad():
                    raw = torch.from_numpy(stack[:fb].view(np.int16)).to(dev)
                    from microbeseg_amd import engine
                    net_ms = time_device(lambda: worker._forward_group(engine.normalize_frames(raw)), 5)
                    net1_ms = time_device(lambda: worker._forward(engine.RawFrame(raw[0])), 5)
                    border = torch.cat([maps[i % NMAPS][0] for i in range(fb)])[:, 0]
                    cell = torch.cat([maps[i % NMAPS][1] for i in range(fb)])[:, 0]
                    pp_ms = time_device(lambda: pp.distance_postprocessing_batch_device(border, cell, 0.45, 0.10), 5)
                    pp1_ms = time_device(lambda: pp.distance_postprocessing_device(border[0], cell[0], 0.45, 0.10), 5)
                entry[prec] = {
                    "batch1": {"frames_s": round(T / t1, 1), "Mpx_s": round(T * S * S / t1 / 1e6, 2),
                               "runs_s": [round(t, 4) for t in times[1]]},
                    "group": {"frames_s": round(T / tg, 1), "Mpx_s": round(T * S * S / tg / 1e6, 2),
                              "runs_s": [round(t, 4) for t in times[args.frame_batch]]},
                    "speedup": round(t1 / tg, 3),
                    "masks_equal": bool(np.array_equal(masks[1], masks[args.frame_batch])),
                    "instances_frame0": int(masks[1][0].max()),
                    "group_split_ms": {"network": round(net_ms, 3), "postproc": round(pp_ms, 3)},
                    "single_frame_ms": {"network": round(net1_ms, 3), "postproc": round(pp1_ms, 3)},
                }
            result[f"{S}x{S}"] = entry
        worker.prediction_hook = None
    print(json.dumps(result))


if __name__ == "__main__":
    main()
