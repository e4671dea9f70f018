#!/usr/bin/env python3
"""Inference at a chosen resolution (InferWorker.scale): what a stack costs at scale 0.5 and 2 against
scale 1 of the same process.

Model: DU [64, 1024] bn / relu with seeded weights (there are no checkpoints offline).  Input: uint16 stacks generated from
a seed, 64 frames of 256^2 and 2 frames of 2048^2.  An untrained network predicts one blob, so realistic full-resolution
distance maps are handed to the post-processing through InferWorker.prediction_hook, the way bench.py does; the network
still runs on every frame, at the scaled size.

Per size, in ONE process: scale = 1, 0.5, 2 are warmed, then the runs alternate (1, 0.5, 2, 1, 0.5, ...); the time is the
wall clock around infer_stack, which returns synchronised; the median over the repeats is reported, and scale = s as a
multiple of scale = 1 of the same process.  Then, for one group per scale != 1: the device time (HIP events around a loop
of calls, so launch gaps are included) of mseg_resample_frames and of the two mseg_resample_planes calls alone with the
bytes they must move (source read once + destination written once) and the resulting GB/s, and the kernels' time as a
share of the group's network forward.

The parent process never touches the GPU: every size runs in a child process of its own under a time limit, nothing is
retried, and after a step that failed or ran out of time no further step is started.  One JSON line.
"""
import argparse
import json
import pathlib
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

FILTERS = (64, 1024)
NMAPS = 8
SIZES = {256: 64, 2048: 2}          # edge length -> frames
SCALES = (1.0, 0.5, 2.0)


def median(v):
    import numpy as np
    return float(np.median(np.asarray(v)))


def event_ms(fn, calls, reps=5):
    """median over ``reps`` of the device time of ``calls`` back-to-back calls, per call"""
    import torch
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) / calls)
    return median(t)


def step(S, T, repeats, seed, frame_batch):
    import numpy as np
    import torch
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import resample as R
    from microbeseg_amd.inference.infer import InferWorker, frame_batch_for
    from microbeseg_amd.utils import synth
    from microbeseg_amd.utils.unets import build_unet
    from microbeseg_amd.utils.utils import pad_amounts
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(0)
        net = build_unet("DU", "relu", "conv", "bn", dev, 1, ch_out=1, filters=FILTERS)
        base = pathlib.Path(tmp) / "distance_model_00"
        torch.save(net.state_dict(), str(base) + ".pth")
        with open(str(base) + ".json", "w") as f:
            json.dump({"architecture": ["DU", "conv", "relu", "bn", list(FILTERS)], "label_type": "distance"}, f)
        worker = InferWorker(model=str(base), device=str(dev), ths=(0.10, 0.45))
    worker.frame_batch = frame_batch
    rng = np.random.Generator(np.random.PCG64(seed + S))
    stack = rng.integers(0, 60000, size=(T, S, S)).astype(np.uint16)
    maps = []
    for _ in range(NMAPS):
        cell, border = synth.synth_prediction_maps(rng, S, S, max(1, int(2500 * (S / 2048.0) ** 2)), rmin=5.0, rmax=13.0)
        maps.append((torch.from_numpy(border).to(dev)[None, None], torch.from_numpy(cell).to(dev)[None, None]))
    count = [0]

    def hook(pred):
        assert tuple(pred[0].shape) == (1, 1, S, S)
        count[0] += 1
        return maps[(count[0] - 1) % NMAPS]
    worker.prediction_hook = hook

    def group_of(s):
        hs, ws = R.out_size(S, s), R.out_size(S, s)
        pads = pad_amounts((hs, ws))
        return hs, ws, pads, min(T, frame_batch_for(hs + pads[0], ws + pads[1], frame_batch))
    for s in SCALES:                                # warm every setting: buffers, weight packs, workspaces, tables
        worker.scale = s
        count[0] = 0
        worker.infer_stack(stack[:min(T, 2 * group_of(s)[3])])
    torch.cuda.synchronize()
    times, masks = {s: [] for s in SCALES}, {}
    for _ in range(repeats):
        for s in SCALES:
            worker.scale = s
            count[0] = 0
            t0 = time.perf_counter()
            masks[s] = worker.infer_stack(stack)
            times[s].append(time.perf_counter() - t0)
    t1 = median(times[1.0])
    out = {"frames": T, "frame_batch": frame_batch}
    for s in SCALES:
        ts = median(times[s])
        hs, ws, pads, group = group_of(s)
        out[f"scale{s:g}"] = {"s": round(ts, 4), "frames_s": round(T / ts, 2), "x_scale1": round(ts / t1, 3),
                              "network_input": [hs + pads[0], ws + pads[1]], "frames_per_group": group,
                              "runs_s": [round(t, 4) for t in times[s]],
                              "masks_equal_scale1": bool(np.array_equal(masks[s], masks[1.0]))}
    # one group per scale != 1: the kernels alone, and the group's forward
    worker.prediction_hook = None
    lib = _lib.load()
    for s in SCALES[1:]:
        worker.scale = s
        hs, ws, pads, n = group_of(s)
        with torch.no_grad():
            raw = torch.from_numpy(stack[:n].view(np.int16)).to(dev)
            minmax = torch.empty((n, 2), dtype=torch.int32, device=dev)
            _lib.check(lib.mseg_frames_minmax(raw.data_ptr(), _lib.PIX_U16, n, S * S, minmax.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "minmax")
            ydown, xdown, yup, xup = R.axis(S, hs, dev), R.axis(S, ws, dev), R.axis(hs, S, dev), R.axis(ws, S, dev)
            x = R.frames(raw, ydown, xdown, pads, minmax)
            heads = [torch.randn((n, 1, hs + pads[0], ws + pads[1]), device=dev) for _ in range(2)]

            def down():
                R.frames(raw, ydown, xdown, pads, minmax)

            def up():
                for h in heads:                                      # border and cell
                    R.planes(h, yup, xup, pads=pads)

            def forward():
                worker._forward_group(x[:, None])
            calls = 50 if S <= 512 else 10
            down_ms, up_ms = event_ms(down, calls), event_ms(up, calls)
            fwd_ms = event_ms(forward, 2 if max(hs, ws) > 512 else 5)
        down_bytes = n * S * S * 2 + n * (hs + pads[0]) * (ws + pads[1]) * 4
        up_bytes = 2 * n * (hs * ws + S * S) * 4
        out[f"group_scale{s:g}"] = {
            "frames": n, "taps": [ydown.taps, yup.taps],
            "resample_frames": {"ms": round(down_ms, 4), "bytes": down_bytes, "GB_s": round(down_bytes / down_ms / 1e6, 1),
                                "launches": 1},
            "resample_planes": {"ms": round(up_ms, 4), "bytes": up_bytes, "GB_s": round(up_bytes / up_ms / 1e6, 1),
                                "launches": 2},
            "forward_ms": round(fwd_ms, 3),
            "kernels_share_of_forward": round((down_ms + up_ms) / fwd_ms, 4),
        }
    print("STEP_JSON " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--frame_batch", type=int, default=1)
    ap.add_argument("--step_timeout", type=int, default=240, help="seconds per size (a child process of its own)")
    ap.add_argument("--step", type=int, default=0, help="(internal) run the step of this edge length in this process")
    args = ap.parse_args()
    if args.step:
        step(args.step, SIZES[args.step], args.repeats, args.seed, args.frame_batch)
        return
    result = {"model": "DU [64,1024] bn/relu, seeded weights", "input": "uint16 stacks from a seed; synthetic distance "
              "maps injected through prediction_hook", "repeats": args.repeats,
              "timing": "wall clock around infer_stack, median; kernels: HIP events around a loop of calls"}
    for S in SIZES:
        cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--step", str(S), "--repeats", str(args.repeats),
               "--seed", str(args.seed), "--frame_batch", str(args.frame_batch)]
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            result[f"{S}x{S}"] = {"error": f"ran longer than {args.step_timeout} s"}
            break
        lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("STEP_JSON ")]
        if proc.returncode != 0 or not lines:
            result[f"{S}x{S}"] = {"error": f"exit status {proc.returncode}", "stderr": proc.stderr[-400:]}
            break
        result[f"{S}x{S}"] = json.loads(lines[-1][len("STEP_JSON "):])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
