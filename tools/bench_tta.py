#!/usr/bin/env python3
"""Test-time augmentation (InferWorker.tta): what K members per frame cost.

Model: DU [64, 1024] bn / relu with seeded weights (there are no checkpoints offline).  Input: uint16 stacks generated from
a seed, 64 frames of 256^2 and 2 frames of 2048^2.  An untrained network predicts one blob, so realistic distance maps are
handed to the post-processing through InferWorker.prediction_hook, the way bench.py does; the network still runs on
every member.

Per size, in ONE process: tta = 1, 2, 4, 8 are warmed, then the runs alternate (1, 2, 4, 8, 1, 2, ...); the time is the
wall clock around infer_stack, which returns synchronised; the median over the repeats is reported, and tta = K as a
multiple of tta = 1 of the same process.  Then, for one group at tta = 8: the device time (HIP events around a loop of
calls, so launch gaps are included) of mseg_tta_expand and mseg_tta_merge alone with the bytes they must move (expand:
the source once + every member written; merge: (K + 1) * 4 bytes per output element) and the resulting GB/s, and the
two kernels' time as a share of the group's network forwards.

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
TTAS = (1, 2, 4, 8)


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
    from microbeseg_amd.inference import tta
    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.utils import synth
    from microbeseg_amd.utils.unets import build_unet
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
    for K in TTAS:                                  # warm every setting: buffers, weight packs, workspaces
        worker.tta = K
        count[0] = 0
        worker.infer_stack(stack[:min(T, 2 * tta.chunk_members(S, S, frame_batch, K)[1])])
    torch.cuda.synchronize()
    times, masks = {K: [] for K in TTAS}, {}
    for _ in range(repeats):
        for K in TTAS:
            worker.tta = K
            count[0] = 0
            t0 = time.perf_counter()
            masks[K] = worker.infer_stack(stack)
            times[K].append(time.perf_counter() - t0)
    t1 = median(times[1])
    out = {"frames": T, "frame_batch": frame_batch}
    for K in TTAS:
        tk = median(times[K])
        m, group = tta.chunk_members(S, S, frame_batch, K)
        out[f"tta{K}"] = {"s": round(tk, 4), "frames_s": round(T / tk, 2), "x_tta1": round(tk / t1, 3),
                          "members_per_forward": m, "frames_per_group": group, "runs_s": [round(t, 4) for t in times[K]],
                          "masks_equal_tta1": bool(np.array_equal(masks[K], masks[1]))}
    # one group at tta = 8: the two kernels alone, and the group's forwards
    K = 8
    worker.tta, worker.prediction_hook = K, None
    m, n = tta.chunk_members(S, S, frame_batch, K)
    n = min(n, T)
    classes = tta.shape_classes(tta.member_codes(K), S, S)
    lib = _lib.load()
    with torch.no_grad():
        raw = torch.from_numpy(stack[:n].view(np.int16)).to(dev)
        minmax = torch.empty((n, 2), dtype=torch.int32, device=dev)
        _lib.check(lib.mseg_frames_minmax(raw.data_ptr(), _lib.PIX_U16, n, S * S, minmax.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "minmax")
        xs = [tta.expand(raw, cs, pads, minmax) for cs, _, pads in classes]
        preds = [torch.randn((x.shape[0] * n, 1, S, S), device=dev) for x in xs]

        def expand_all():
            for cs, _, pads in classes:
                tta.expand(raw, cs, pads, minmax)

        def merge_all():
            members = {}
            for (cs, _, pads), p in zip(classes, preds):
                for ci, c in enumerate(cs):
                    members[c] = tta.member(p, c, first=ci * n, pads=pads)
            for _ in range(2):                                   # border and cell
                tta.merge([members[c] for c in sorted(members)], n, 1, S, S)

        def forwards():
            for x in xs:
                x = x.view(-1, 1, S, S)
                for c0 in range(0, x.shape[0], m):
                    worker._forward_group(x[c0:c0 + m])
        calls = 50 if S <= 512 else 10
        exp_ms, mrg_ms = event_ms(expand_all, calls), event_ms(merge_all, calls)
        fwd_ms = event_ms(forwards, 2 if S > 512 else 5)
    exp_bytes = n * S * S * 2 + K * n * S * S * 4
    mrg_bytes = 2 * (K + 1) * 4 * n * S * S
    out["group_tta8"] = {
        "frames": n,
        "expand": {"ms": round(exp_ms, 4), "bytes": exp_bytes, "GB_s": round(exp_bytes / exp_ms / 1e6, 1), "launches": 2},
        "merge": {"ms": round(mrg_ms, 4), "bytes": mrg_bytes, "GB_s": round(mrg_bytes / mrg_ms / 1e6, 1), "launches": 2},
        "forwards_ms": round(fwd_ms, 3),
        "kernels_share_of_forwards": round((exp_ms + mrg_ms) / fwd_ms, 4),
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
