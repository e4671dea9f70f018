#!/usr/bin/env python3
"""Prepare a training set from local files on the MI355X: the first steps of the workflow without an OMERO server.

``prepare_script.py crops``  proposes training crops for every frame of the .tif images / stacks of ``--img_dir`` (the
reference's DataCropWorker): ``img_<k>.tif`` (the crop), ``show_<k>.tif`` (its 8-bit view) and ``crops.json`` (the crop
records); with ``--model`` the crops are pre-labelled: ``mask_<k>.tif`` is the predicted instance mask, ``overlay_<k>.tif`` is the view with the outlines and ``rois_<k>.json`` holds the polygon strings.

``prepare_script.py import``  turns annotated images (``img<name>`` + ``mask<name>``) into ``<out>/train|val|test`` with
``img_extNNN.tif`` / ``mask_extNNN.tif`` (the reference's DataImportWorker followed by its training-set export).
"""
import argparse
import json
import random
from pathlib import Path

import torch


def crops_main(args):
    from infer_script_local import select_frames
    from microbeseg_amd.utils import tiffio as tiff
    from microbeseg_amd.utils.data_cropping import DataCropWorker
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    file_ids = sorted(Path(args.img_dir).glob('*.tif*'))
    if len(file_ids) == 0:
        print('No files found')
        return
    if len(args.thresholds) != 2:
        raise Exception(f"{len(args.thresholds)} threshold given, needed are 2")
    pre = args.model is not None
    worker = DataCropWorker(crop_size=args.crop_size, pre_labeling=pre, model=Path(args.model) if pre else None,
                            device=args.device, ths=args.thresholds)
    worker.precision = args.precision
    worker.text_output.connect(print)
    frames, origin = [], []
    for img_id in file_ids:
        stack = select_frames(tiff.imread(str(img_id)), args.channel, img_id.name)
        if stack is None:
            continue
        for t in range(0, len(stack), max(1, args.step)):
            frames.append(stack[t])
            origin.append((img_id.name, t))
    crops = worker.crops_local(frames, args.crop_size, rng=random.Random(args.seed))
    records, k = [], 0
    for frame_crops in crops:
        for crop in frame_crops:
            name, t = origin[crop['frame']]
            tiff.imwrite(str(out / f"img_{k}.tif"), crop['img'])
            tiff.imwrite(str(out / f"show_{k}.tif"), crop['img_show'])
            record = {key: crop[key] for key in ('crop_size', 'min_frame', 'max_frame', 'mean_frame', 'std_frame',
                                                  'pre_labeled', 'x_start', 'y_start')}
            record.update({'file': f"img_{k}.tif", 'image': name, 'frame': str(t), 'channel': str(args.channel)})
            if pre:
                tiff.imwrite(str(out / f"mask_{k}.tif"), crop['mask'])
                tiff.imwrite(str(out / f"overlay_{k}.tif"), crop['roi_show'][None])
                with open(out / f"rois_{k}.json", 'w', encoding='utf-8') as f:
                    json.dump({'file': f"img_{k}.tif", 'rois': crop['roi']}, f)
            records.append(record)
            k += 1
    with open(out / 'crops.json', 'w', encoding='utf-8') as f:
        json.dump(records, f, ensure_ascii=False, indent=2)
    print(f'{k} crops written to {out}')


def import_main(args):
    from microbeseg_amd.utils.data_import import DataImportWorker, SUFFIXES
    img_ids = sorted(p for p in Path(args.img_dir).iterdir() if p.name.startswith('img') and p.suffix.lower() in SUFFIXES)
    if len(img_ids) == 0:
        print('No files found')
        return
    worker = DataImportWorker()
    records = worker.import_local(img_ids, args.keep_normalization, args.crop_size, Path(args.out),
                                  1 - args.p_val - args.p_test, args.p_val, args.p_test, rng=random.Random(args.seed),
                                  raw_masks=args.raw_masks, device=args.device)
    print(f'{len(records)} crops written to {args.out}')


def main():
    parser = argparse.ArgumentParser(description='microbeSEG training-set preparation on local files (MI355X-native)')
    sub = parser.add_subparsers(dest='command', required=True)
    c = sub.add_parser('crops', help='propose training crops, optionally pre-labelled by a model')
    c.add_argument('--img_dir', '-i', required=True, type=str, help='Directory with .tif images / stacks')
    c.add_argument('--crop_size', '-s', required=True, type=int, help='Crop size')
    c.add_argument('--out', '-r', required=True, type=str, help='Directory for the crops')
    c.add_argument('--model', '-m', default=None, type=str, help='Model for pre-labelling (<name>.json beside <name>.pth)')
    c.add_argument('--thresholds', '-t', default=[0.10, 0.45], nargs='+', type=float,
                   help='Thresholds for distance method: th_cell th_seed')
    c.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'], help='network arithmetic of the pre-labelling')
    c.add_argument('--channel', '-c', default=0, type=int, help='Channel to crop')
    c.add_argument('--step', default=1, type=int, help='Use every step-th frame of a stack')
    c.add_argument('--seed', default=None, type=int, help='Seed of the crop positions')
    c.add_argument('--device', '-d', default='cuda:0', type=str, help='"cuda:N"')
    c.set_defaults(run=crops_main)
    m = sub.add_parser('import', help='import annotated images (img* + mask*) into train / val / test')
    m.add_argument('--img_dir', '-i', required=True, type=str, help='Directory with img<name> / mask<name> pairs')
    m.add_argument('--crop_size', '-s', required=True, type=int, help='Crop size')
    m.add_argument('--out', '-r', required=True, type=str, help='Training set directory')
    m.add_argument('--keep_normalization', default=False, action='store_true',
                   help='Keep the initial normalization (range of the dtype instead of the image extrema)')
    m.add_argument('--p_val', default=0.2, type=float, help='Probability of the val set')
    m.add_argument('--p_test', default=0.2, type=float, help='Probability of the test set')
    m.add_argument('--seed', default=None, type=int, help='Seed of the split')
    m.add_argument('--raw_masks', default=False, action='store_true',
                   help='[extension] write the mask crops as they are instead of their polygons\' fill')
    m.add_argument('--device', '-d', default='cuda:0', type=str, help='"cuda:N"')
    m.set_defaults(run=import_main)
    args = parser.parse_args()
    if 'cuda' in args.device and not torch.cuda.is_available():
        raise ValueError('No MI355X visible: this build has no CPU path')
    torch.set_grad_enabled(False)
    args.run(args)


if __name__ == "__main__":
    main()
