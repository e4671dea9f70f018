#!/usr/bin/env python3
"""Gap closing in cell tracks on the MI355X: device milliseconds per frame pair of the sparse pass across a gap
(mseg_cell_links_gap at gap 2 and 3, with the orphan / open-end flags of the stack itself) beside the ordinary pass under a
shift (mseg_cell_links_shifted) from the same run, alternating; the all-in time of measure_cells with gap = 2 against without;
the track counts with and without; and the time of the numpy restatement (tests/gap_ref.py) for one frame pair on one core,
whose values the device must equal.  Synthetic stack: 2048^2 x 16 uint16, about 2400 static cells (ellipses with semi-axes
4 - 8 and 2 - 3 px on a jittered 41 px grid: they do not touch); 5 % of them are blanked in one frame, 1 % in two
consecutive frames.  No figure is fixed in advance.  Prints one JSON line at the end.  GPU box only.

The process that is started never touches the GPU: it runs the measurement in a child under a time limit.
  python tools/bench_gap.py [--frames 16] [--reps 5] [--limit 420]"""
import argparse
import json
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
SIZE, PITCH, JITTER = 2048, 41, 6
ONE_FRAME, TWO_FRAMES = 0.05, 0.01


def stack(T, seed=7):
    """-> (labels uint16 [T, 2048, 2048], missed bool [T, n]: cell k + 1 is blanked in frame t)"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.arange(PITCH // 2 + 2, SIZE - PITCH // 2 - 2, PITCH, dtype=np.float64)
    p = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2) + rng.uniform(-JITTER, JITTER, (len(g) ** 2, 2))
    n = len(p)
    a, b, th = rng.uniform(4, 8, n), rng.uniform(2, 3, n), rng.uniform(0, np.pi, n)
    frame = np.zeros((SIZE, SIZE), np.uint16)
    yy, xx = np.mgrid[-9:10, -9:10]
    for k, (cy, cx) in enumerate(p, start=1):
        y0, x0 = int(round(cy)), int(round(cx))
        dy, dx = yy + y0 - cy, xx + x0 - cx
        u, v = dy * np.cos(th[k - 1]) + dx * np.sin(th[k - 1]), -dy * np.sin(th[k - 1]) + dx * np.cos(th[k - 1])
        box = frame[y0 - 9:y0 + 10, x0 - 9:x0 + 10]
        assert not box[(u / a[k - 1]) ** 2 + (v / b[k - 1]) ** 2 <= 1].any(), "cells touch"
        box[(u / a[k - 1]) ** 2 + (v / b[k - 1]) ** 2 <= 1] = k
    missed = np.zeros((T, n), bool)
    draw = rng.random(n)
    for k in np.nonzero(draw < ONE_FRAME + TWO_FRAMES)[0]:
        two = draw[k] < TWO_FRAMES
        t = int(rng.integers(1, T - 1 - two))                # never the first or the last frame: every gap has two ends
        missed[t:t + 1 + two, k] = True
    labels = np.zeros((T, SIZE, SIZE), np.uint16)
    for t in range(T):
        keep = np.concatenate([[0], np.where(missed[t], 0, np.arange(1, n + 1))]).astype(np.uint16)
        labels[t] = keep[frame]
    return labels, missed


def child(a):
    import ctypes as C

    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    from microbeseg_amd import _lib
    from microbeseg_amd.inference import cells
    import cells_ref as ref
    import gap_ref as gref

    if not torch.cuda.is_available():
        raise SystemExit("no MI355X visible: nothing to measure")

    def event_ms(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    labels, missed = stack(a.frames)
    T, H, W = labels.shape
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lab_d = torch.from_numpy(labels.view(np.int16)).to(dev)
    off = ref.frame_tables(labels)
    n = int(off[-1])
    off_d = torch.from_numpy(off).to(dev)
    present = float((~missed).sum()) / T
    one = int(((missed.sum(axis=0) == 1)).sum())
    two = int(((missed.sum(axis=0) == 2)).sum())
    print(f"stack {T} x {H} x {W}, {present:.0f} cells per frame; {one} cells missed in one frame, {two} in two consecutive")
    out = {"frames": T, "height": H, "width": W, "cells_per_frame": present, "missed_one_frame": one, "missed_two_frames": two}

    # ---- the flags of the stack itself: orphans and open ends after the ordinary links ----
    pred, ovl = cells.link_raw(lab_d, _lib.PIX_U16, off)
    frame = np.repeat(np.arange(T), np.diff(off))
    linked = pred > 0
    area = cells.measure_raw(lab_d, _lib.PIX_U16, off)["shape"][0] > 0
    want, open_ = ~linked & area, area.copy()
    open_[off[frame[linked] - 1] + pred[linked] - 1] = False
    out["orphans"], out["open_ends"] = int(want[int(off[1]):].sum()), int(open_[:int(off[T - 1])].sum())
    print(f"  after the ordinary links: {out['orphans']} orphans in frames 1 .., {out['open_ends']} open ends before the last frame")

    # ---- one frame pair against the restatement, on one core ----
    sub = slice(0, 3)
    t0 = time.perf_counter()
    ref_pred, ref_ovl = gref.links_gap(labels[sub], off[:4], 2, want[:int(off[3])], open_[:int(off[3])])
    out["numpy_restatement_s_per_pair"] = time.perf_counter() - t0
    got = cells.link_gap_raw(lab_d[sub], _lib.PIX_U16, off[:4], 2, want[:int(off[3])], open_[:int(off[3])])
    assert np.array_equal(got[0], ref_pred) and np.array_equal(got[1], ref_ovl), "device gap links differ from the restatement"
    print(f"  numpy restatement, gap 2: {out['numpy_restatement_s_per_pair']:6.2f} s per frame pair ({int((ref_pred > 0).sum())} links, "
          f"equal to the device's)")

    # ---- the gap pass beside the ordinary pass under a shift, alternating ----
    k = np.diff(off)
    cap = max(cells.MIN_TABLE, cells._pow2(4 * int((k[1:] + k[:-1]).max())))
    flags = torch.from_numpy(np.concatenate([want, open_]).astype(np.uint8)).to(dev)
    shift_d = torch.zeros((T, 2), dtype=torch.int32, device=dev)
    res = torch.empty((2, n), dtype=torch.int32, device=dev)
    status = torch.empty(T, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mseg_cell_links_workspace_bytes(T, n, cap), dtype=torch.uint8, device=dev)
    calls = {"links_shifted": lambda: _lib.check(lib.mseg_cell_links_shifted(
        lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, cap, shift_d.data_ptr(), res[0].data_ptr(),
        res[1].data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), st))}
    for g in (2, 3):
        calls[f"links_gap{g}"] = lambda g=g: _lib.check(lib.mseg_cell_links_gap(
            lab_d.data_ptr(), _lib.PIX_U16, T, H, W, off_d.data_ptr(), n, cap, g, 0, shift_d.data_ptr(), flags.data_ptr(),
            flags.data_ptr() + n, res[0].data_ptr(), res[1].data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), st))
    ms = {name: [] for name in calls}
    for rep in range(a.reps + 1):                         # the first round warms up
        for name, call in calls.items():
            ms[name].append(event_ms(call))
            assert not status.cpu().numpy().any(), "pair table full at the wrapper's starting size"
    for name, v in ms.items():
        pairs = T - (int(name[-1]) if name != "links_shifted" else 1)
        out[f"{name}_ms_per_pair"] = float(np.median(v[1:])) / pairs
        out[f"{name}_ms_per_pair_range"] = [min(v[1:]) / pairs, max(v[1:]) / pairs]
        print(f"  {name:14s} {out[f'{name}_ms_per_pair']:8.4f} ms per frame pair ({min(v[1:]) / pairs:.4f} .. {max(v[1:]) / pairs:.4f}; "
              f"table of {cap} entries, memset and best / out passes included)")

    # ---- measure_cells all-in, and what gap closing is for ----
    tables = {}
    for name, kw in 2 * (("plain", {}), ("gap2", {"gap": 2})):           # the first round warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tables[name] = cells.measure_cells(lab_d, **kw)
        out[f"measure_cells_{name}_all_in_ms_per_frame"] = 1e3 * (time.perf_counter() - t0) / T
    for name, df in tables.items():
        out[f"tracks_{name}"] = int(df["track_id"].nunique())
    out["closed_gaps"] = int((tables["gap2"]["pred_gap"] > 1).sum())
    assert out["closed_gaps"] == one + two and out["tracks_gap2"] == missed.shape[1], "a gap of the stack was not closed"
    print(f"  measure_cells all-in: {out['measure_cells_plain_all_in_ms_per_frame']:7.1f} ms per frame, with gap = 2: "
          f"{out['measure_cells_gap2_all_in_ms_per_frame']:7.1f} ms per frame; {out['tracks_plain']} tracks without, "
          f"{out['tracks_gap2']} with ({out['closed_gaps']} gaps closed)")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--child", "--frames", str(a.frames), "--reps", str(a.reps)]
    try:
        done = subprocess.run(cmd, timeout=a.limit)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"the measurement did not finish within {a.limit} s"}))
        raise SystemExit(1)
    raise SystemExit(done.returncode)


if __name__ == "__main__":
    main()
