#!/usr/bin/env python3
"""Training-set preparation on the device: crop proposals with pre-labelling, batched against crop by crop, and the import.

Model: DU [64, 1024] bn / relu with seeded weights (there are no checkpoints offline).  Input: ``--frames`` uint16 frames
of ``--size``^2 generated from a seed, crops of ``--crop``.  An untrained network predicts one blob, so realistic distance
maps are handed to the post-processing through ``prediction_hook``, the way bench.py does; the network still runs on
every crop.  Two routes alternate in one process after both are warm, masks asserted equal:

  batched    DataCropWorker.crops_local with pre-labelling at batch_frames = 8: one upload, one statistics pass and one
             extraction launch per frame, ONE forward and one batched post-processing call for the crops of 8 frames,
             one outline and one overlay launch per group
  one_crop   the reference's structure on the one-crop entry points: crops_local without pre-labelling frame by frame,
             then per crop DataCropWorker.inference (host normalisation, forward at batch 1, one-frame post-processing)
             and the ROIs / overlay of that crop alone

The import part writes ``--images`` annotated images of ``--size``^2 (about 2400 cells each; ``--distinct`` different files,
repeated) and times DataImportWorker.import_local on them, files read and written included.

One JSON line: crops/s of both routes (median over the repeats), their ratio, and crops/s of the import.
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

FILTERS = (64, 1024)
NMAPS = 8


def make_model(tmp, dev):
    from microbeseg_amd.utils.unets import build_unet
    torch.manual_seed(0)
    net = build_unet("DU", "relu", "conv", "bn", dev, 1, ch_out=1, filters=FILTERS)
    base = pathlib.Path(tmp) / "distance_model_00"
    torch.save(net.state_dict(), str(base) + ".pth")
    with open(str(base) + ".json", "w") as f:
        json.dump({"architecture": ["DU", "conv", "relu", "bn", list(FILTERS)], "label_type": "distance"}, f)
    return base.with_suffix(".json")


def make_hook(S, dev):
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(3))
    maps = []
    for _ in range(NMAPS):
        cell, border = synth.synth_prediction_maps(rng, S, S, max(1, int(2500 * (S / 2048.0) ** 2)), rmin=5.0, rmax=13.0)
        maps.append((torch.from_numpy(border).to(dev)[None, None], torch.from_numpy(cell).to(dev)[None, None]))
    count = [0]

    def hook(pred):
        count[0] += 1
        return maps[(count[0] - 1) % NMAPS]
    return hook, count


def run_batched(worker, frames, crop, count):
    count[0] = 0
    t0 = time.perf_counter()
    out = worker.crops_local(frames, crop, rng=random.Random(1), batch_frames=8)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, [d['mask'] for g in out for d in g]


def run_one_crop(worker, frames, crop, count, dev):
    count[0] = 0
    rng = random.Random(1)
    masks = []
    t0 = time.perf_counter()
    for frame in frames:
        for g in worker.crops_local([frame], crop, pre_labeling=False, rng=rng, batch_frames=1):
            for d in g:
                mask = worker.inference(d['img'], np.min(frame), np.max(frame))
                m_d = torch.from_numpy(mask.view(np.int16)).to(dev)[None]
                d['roi'], rgb = worker._rois_and_overlays(m_d, torch.from_numpy(d['img_show']).to(dev)[None])
                d['roi_show'] = rgb[0]
                masks.append(mask)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, masks


def annotated_pair(size, seed):
    """image / mask of size^2 with about 2400 cells per 2048^2: a 256^2 tile of cells repeated with fresh ids"""
    from microbeseg_amd.utils import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    tile = synth.synth_instance_mask(rng, 256, 38, rmin=5.0, rmax=13.0)
    k = int(tile.max())
    reps = size // 256
    mask = np.zeros((size, size), np.uint16)
    for i in range(reps):
        for j in range(reps):
            mask[i * 256:(i + 1) * 256, j * 256:(j + 1) * 256] = np.where(tile > 0, tile + (i * reps + j) * k, 0)
    img = np.clip((mask > 0) * 30000 + rng.normal(8000, 1500, mask.shape), 0, 65535).astype(np.uint16)
    return img, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    from microbeseg_amd.utils import tiffio
    from microbeseg_amd.utils.data_cropping import DataCropWorker
    from microbeseg_amd.utils.data_import import DataImportWorker
    dev = torch.device(args.device)
    result = {"frames": args.frames, "size": args.size, "crop": args.crop}
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        worker = DataCropWorker(crop_size=args.crop, pre_labeling=True, model=make_model(tmp, dev), device=dev,
                                ths=[0.10, 0.45])
        worker.prediction_hook, count = make_hook(args.crop, dev)
        rng = np.random.Generator(np.random.PCG64(1))
        frames = [rng.integers(200 * t, 20000 + 500 * t, size=(args.size, args.size)).astype(np.uint16)
                  for t in range(args.frames)]
        run_batched(worker, frames[:8], args.crop, count)                    # warm-up of both routes
        run_one_crop(worker, frames[:2], args.crop, count, dev)
        tb, to = [], []
        for _ in range(args.repeats):
            t, mb = run_batched(worker, frames, args.crop, count)
            tb.append(t)
            t, mo = run_one_crop(worker, frames, args.crop, count, dev)
            to.append(t)
            assert len(mb) == len(mo) and all(np.array_equal(a, b) for a, b in zip(mb, mo)), "masks differ"
        n = len(mb)
        result.update(crops=n, instances=int(sum(int(m.max()) for m in mb)),
                      batched_crops_per_s=n / float(np.median(tb)), one_crop_crops_per_s=n / float(np.median(to)),
                      ratio=float(np.median(to)) / float(np.median(tb)), masks_equal=True)
        del worker
        src = pathlib.Path(tmp) / "annotated"
        src.mkdir()
        ids = []
        for k in range(args.distinct):
            img, mask = annotated_pair(args.size, 10 + k)
            tiffio.imwrite(str(src / f"img_{k:02d}.tif"), img)
            tiffio.imwrite(str(src / f"mask_{k:02d}.tif"), mask)
            ids.append(src / f"img_{k:02d}.tif")
        ids = [ids[k % args.distinct] for k in range(args.images)]
        importer = DataImportWorker()
        importer.import_local(ids[:1], False, args.crop, pathlib.Path(tmp) / "warm", 0.8, 0.1, 0.1, rng=random.Random(1),
                              text_output=lambda s: None, device=dev)
        t0 = time.perf_counter()
        records = importer.import_local(ids, False, args.crop, pathlib.Path(tmp) / "set", 0.8, 0.1, 0.1,
                                        rng=random.Random(1), text_output=lambda s: None, device=dev)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        result.update(import_images=len(ids), import_cells_per_image=int(mask.max()), import_crops=len(records),
                      import_crops_per_s=len(records) / t, import_seconds=t)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
