#!/usr/bin/env python3
"""What the data route costs a training run: ``TrainWorker`` epochs fed by the data loader against the device-resident set.

A synthetic set (``--train`` / ``--val`` crops of ``--size``^2, both label types) is written once.  Per configuration the
product's own driver (``TrainWorker.start_training``, device augmentation on) runs ``--epochs`` epochs on each route, the
routes alternating in one process, ``--repeats`` times; the first epoch of every run is warm-up.  Reported per
configuration and route:

  crops_per_s        train-phase crops per second (median over the timed epochs of all repeats)
  wait / feeder / step   share of the train phase the host spends waiting for the next batch (file reads, collation and
                     pinning in the workers, or the gather launches), in ``_Feeder`` (upload + augmentation launches) and
                     in the step; the step's share includes waiting for the device at ``loss.item()``
  load_s             the one-off read + upload of the resident set
  bare_crops_per_s   the ceiling: the same driver stepping on one fixed, already augmented device batch (no data work)

One JSON object on the last line.  The loader route uses ``--workers`` processes (at most 16).
"""
import argparse
import json
import pathlib
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

CONFIGS = (
    dict(name="DU[64,1024] b32 fp32", label_type="distance", batch=32, precision="fp32"),
    dict(name="DU[64,1024] b32 bf16", label_type="distance", batch=32, precision="bf16"),
    dict(name="DU[64,1024] b4 bf16", label_type="distance", batch=4, precision="bf16"),
    dict(name="U[64,1024] boundary b32 bf16", label_type="boundary", batch=32, precision="bf16"),
)
FILTERS = [64, 1024]


class _Clock:
    def __init__(self):
        self.reset()

    def reset(self):
        self.wait = self.feeder = 0.0


CLOCK = _Clock()


class _TimedBatches:
    """times the host's wait for every batch of a phase's loader"""

    def __init__(self, loader):
        self.loader = loader

    def __iter__(self):
        t0 = time.perf_counter()
        it = iter(self.loader)
        CLOCK.wait += time.perf_counter() - t0
        return self._timed(it)

    @staticmethod
    def _timed(it):
        while True:
            t0 = time.perf_counter()
            try:
                batch = next(it)
            except StopIteration:
                return
            finally:
                CLOCK.wait += time.perf_counter() - t0
            yield batch


class _FixedBatches:
    """the bare route: one fixed, already augmented device batch for every step of the plan"""

    def __init__(self, plan, batch):
        self.plan, self.batch = plan, batch

    def __iter__(self):
        return (tuple(t[:len(indices)] for t in self.batch) for indices in list(self.plan))


def make_worker(T, route, args):
    base_feeder = T._Feeder

    class Feeder(base_feeder):
        def __call__(self, samples, training):
            if route == "bare":
                return samples[0], tuple(samples[1:])
            t0 = time.perf_counter()
            out = super().__call__(samples, training)
            CLOCK.feeder += time.perf_counter() - t0
            return out

    class Worker(T.TrainWorker):
        epochs_s, load_s = None, None

        def _resident_set(self, datasets, configs, device):
            fresh = self.resident and self._resident_state is None
            t0 = time.perf_counter()
            rset = super()._resident_set(datasets, configs, device)
            if fresh:
                torch.cuda.synchronize()
                self.load_s = time.perf_counter() - t0
            return rset

        def _loaders(self, datasets, configs, device, world, rank):
            plans, loaders = super()._loaders(datasets, configs, device, world, rank)
            if route == "bare":
                from microbeseg_amd.training.resident_set import ResidentSet, load_host
                rset = ResidentSet(load_host(datasets['train'].root_dir, configs['label_type']), configs['label_type'],
                                   device, 0, 65535, raw_train=True)
                feeder = base_feeder(configs['label_type'], device, datasets['train'].transform)
                fixed = {}
                for x in T.PHASES:
                    n = min(configs['batch_size'], len(datasets[x]))
                    img, labels = feeder(rset.batch(x, list(range(n)), x == 'train'), x == 'train')
                    fixed[x] = _FixedBatches(plans[x], (img,) + tuple(labels))
                rset.release()
                return plans, fixed
            return plans, {x: _TimedBatches(loaders[x]) for x in T.PHASES}

        def _run_phase(self, phase, *a, **k):
            if phase != 'train':
                return super()._run_phase(phase, *a, **k)
            CLOCK.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = super()._run_phase(phase, *a, **k)
            torch.cuda.synchronize()
            self.epochs_s.append((time.perf_counter() - t0, CLOCK.wait, CLOCK.feeder))
            return out

    w = Worker()
    w.epochs_s = []
    w.num_workers = args.workers
    w.resident = route == "resident"
    return w, Feeder


def run(T, route, cfg, data, args, tmp, tag):
    models = pathlib.Path(tmp) / "models_{}".format(tag)
    models.mkdir()
    torch.manual_seed(1)
    np.random.seed(1)
    random.seed(1)
    w, feeder = make_worker(T, route, args)
    w.precision = cfg["precision"]
    said = []
    w.text_output.connect(said.append)
    original, T._Feeder = T._Feeder, feeder
    try:
        w.start_training(data, models, cfg["label_type"], 1, "adam", cfg["batch"], torch.device(args.device), 1, False,
                         filters=FILTERS, max_epochs=args.epochs)
    finally:
        T._Feeder = original
    if route == "resident" and any(m.startswith("Resident training set not used") for m in said):
        raise RuntimeError("the resident route fell back: " + "; ".join(said))
    if len(w.epochs_s) != args.epochs:
        raise RuntimeError("{} epochs instead of {}: {}".format(len(w.epochs_s), args.epochs, said[-3:]))
    return w.epochs_s[1:], w.load_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=512)
    ap.add_argument("--val", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=3, help="per run; the first one is warm-up")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--configs", type=int, nargs="*", default=None, help="indices into CONFIGS (default: all)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    args.workers = max(0, min(args.workers, 16))
    if args.epochs < 2:
        raise SystemExit("--epochs must be at least 2 (the first epoch is warm-up)")
    from microbeseg_amd.training import train as T
    from microbeseg_amd.utils import synth
    result = {"train": args.train, "val": args.val, "size": args.size, "epochs": args.epochs, "repeats": args.repeats,
              "workers": args.workers, "configs": []}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        data = synth.write_training_set(pathlib.Path(tmp) / "set", args.train, args.val, size=args.size, seed=7)
        result["write_set_s"] = time.perf_counter() - t0
        for ci, cfg in enumerate(CONFIGS):
            if args.configs is not None and ci not in args.configs:
                continue
            epochs = {"loader": [], "resident": []}
            load_s = []
            for rep in range(args.repeats):
                for route in ("loader", "resident"):
                    e, load = run(T, route, cfg, data, args, tmp, "{}_{}_{}".format(ci, route, rep))
                    epochs[route] += e
                    if load is not None:
                        load_s.append(load)
            bare, _ = run(T, "bare", cfg, data, args, tmp, "{}_bare".format(ci))
            row = {"config": cfg["name"], "batch": cfg["batch"], "precision": cfg["precision"],
                   "bare_crops_per_s": args.train / float(np.median([e[0] for e in bare])),
                   "load_s": float(np.median(load_s))}
            for route, es in epochs.items():
                total, wait, feeder = (float(np.median([e[k] for e in es])) for k in range(3))
                row[route] = {"crops_per_s": args.train / total, "train_phase_s": total, "wait": wait / total,
                              "feeder": feeder / total, "step": max(0.0, 1.0 - (wait + feeder) / total)}
            row["resident_over_loader"] = row["resident"]["crops_per_s"] / row["loader"]["crops_per_s"]
            result["configs"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
