#!/usr/bin/env python3
"""Segment local TIFF images / 2D+t stacks with a trained model on the MI355X hot path.

Same flags and output as the reference ``infer_script_local.py`` (:17-25, :164-165): ``--img_dir/-i``, ``--model/-m``,
``--thresholds/-t`` (th_cell th_seed, default 0.10 0.45), ``--result_path/-r``, ``--channel/-c``, ``--device/-d``,
``--overwrite/-o``; writes ``mask_<stem>_channel<c>.tif`` (uint16, [T, H, W] squeezed); ``--export`` adds the files of
the GUI's Export button (inference/result_export.py) for the segmented channel of uint8 / uint16 stacks;
``--frame_batch N`` sends the frames of a stack through the network and the post-processing in groups of N;
``--clahe`` enhances every uint8 / uint16 frame first, like the reference's ``ContrastEnhancement(apply_clahe=True)``;
``--cells`` adds ``mask_<stem>_channel<c>_cells.csv``, one row per cell and frame (inference/cells.py);
``--tta K`` segments the average of the predictions of K flipped / rotated copies of every frame (inference/tta.py);
``--scale S`` predicts every frame at S times its resolution and segments at its own (inference/resample.py);
``--drift [R]`` with ``--cells``: cells are linked under the stage drift found within +-R pixels (inference/cells.py);
``--flow [r] [--flow_tile B]`` with ``--cells --drift``: cells are linked under one shift per B px tile, within +-r pixels of the drift;
``--gap [G]`` with ``--cells``: a cell missed in up to G consecutive frames keeps its track (inference/cells.py);
``--hull`` with ``--cells``: perimeter, convex hull and Feret length / width / angle of every cell (inference/cells.py);
``--midline`` with ``--cells``: the thinned midline of every cell: its length, for bent and filamentous cells (inference/cells.py);
``--percentiles [P ...]`` with ``--cells``: percentiles (default 50, the median) of every cell's pixel values and of the background;
``--neighbors [R]`` with ``--cells``: every cell's contacts and nearest neighbour within R pixels, and ``..._contacts.csv``, the pairs;
``--spots THR [--spot_scale S]`` with ``--cells``: every cell's fluorescent foci of at least THR grey levels, and ``..._spots.csv``, the spots.
``--profile [N]`` with ``--cells``: every cell's intensity profile along its axis in N bins (default 16), and ``..._profiles.csv``, the profiles.
"""
import argparse
from pathlib import Path

import numpy as np
import torch


def select_frames(img, channel, name):
    """-> [T, H, W] (same rules as infer_script_local.py:85-101); None = unsupported shape."""
    if img.ndim == 2:
        return img[None, ...]
    if img.ndim == 3:
        if img.shape[-1] == 3:
            return img[..., channel][None, ...]
        if img.shape[0] == 3:
            return img[channel, ...][None, ...]
        return img
    if img.ndim == 4:
        return img[:, channel, ...]
    if img.ndim == 5:
        print(f'Skip {name} (not supported image shape)')
        return None
    raise Exception('Adapt script for your data format!')


def select_channels(img, channels, name):
    """The sibling of select_frames for the cell table: the ``channels`` of the source image as a [T, C, H, W] VIEW
    (strides, no copy) whose frames are those select_frames returns.  Sources without a channel axis ([H, W], [T, H, W])
    have the single channel 0.  A channel the image does not have raises ValueError; None = unsupported shape."""
    if img.ndim == 2:
        view = img[None, None]
    elif img.ndim == 3:
        if img.shape[-1] == 3:
            view = np.moveaxis(img, -1, 0)[None]
        elif img.shape[0] == 3:
            view = img[None]
        else:
            view = img[:, None]
    elif img.ndim == 4:
        view = img
    else:
        return None
    missing = [c for c in channels if c < 0 or c >= view.shape[1]]
    if missing:
        raise ValueError(f'{name}: channel(s) {missing} requested for the cell table, the image has {view.shape[1]}')
    step = channels[1] - channels[0] if len(channels) > 1 else 1
    if step > 0 and all(b - a == step for a, b in zip(channels, channels[1:])):
        return view[:, channels[0]:channels[-1] + 1:step]           # basic slicing: still a view
    return view[:, list(channels)]


def scale_argument(text):
    """--scale: a real number in [0.25, 4] (the rule of InferWorker.scale)"""
    from microbeseg_amd.inference.resample import check_scale
    try:
        return check_scale(float(text))
    except ValueError as err:
        raise argparse.ArgumentTypeError(str(err))


class Parser(argparse.ArgumentParser):
    """reports the combinations the worker would refuse as command-line errors, before a model is loaded"""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.flow is not None:
            if not ns.cells:
                self.error('--flow needs --cells (it changes how the cell table links frames)')
            if ns.drift is None:
                self.error('--flow needs --drift (the tiles search around the stage drift of every frame pair)')
            if not 0 <= ns.flow <= 32:
                self.error(f'--flow: a search radius of 0 .. 32 pixels expected, got {ns.flow}')
        if ns.gap is not None:
            if not ns.cells:
                self.error('--gap needs --cells (it changes how the cell table links frames)')
            if not 1 <= ns.gap <= 4:
                self.error(f'--gap: 1 .. 4 missed frames expected, got {ns.gap}')
        if ns.drift is not None:
            if not ns.cells:
                self.error('--drift needs --cells (it changes how the cell table links frames)')
            if not 0 <= ns.drift <= 128:
                self.error(f'--drift: a search radius of 0 .. 128 pixels expected, got {ns.drift}')
        if ns.hull and not ns.cells:
            self.error('--hull needs --cells (it adds columns to the cell table)')
        if ns.midline and not ns.cells:
            self.error('--midline needs --cells (it adds columns to the cell table)')
        if ns.percentiles is not None:
            if not ns.cells:
                self.error('--percentiles needs --cells (it adds columns to the cell table)')
            from microbeseg_amd.inference.cells import check_percentiles
            try:
                ns.percentiles = list(check_percentiles(ns.percentiles or [50]))     # the bare flag: the median
            except ValueError as e:
                self.error(f'--percentiles: {e}')
        if ns.neighbors is not None:
            if not ns.cells:
                self.error('--neighbors needs --cells (it adds columns to the cell table)')
            from microbeseg_amd.inference.cells import check_neighbors
            try:
                ns.neighbors = check_neighbors(ns.neighbors)
            except ValueError as e:
                self.error(f'--neighbors: {e}')
        if ns.spots is not None:
            if not ns.cells:
                self.error('--spots needs --cells (it adds columns to the cell table)')
            from microbeseg_amd.inference.cells import check_spots
            try:
                ns.spots, ns.spot_scale = check_spots(ns.spots, ns.spot_scale)
            except ValueError as e:
                self.error(f'--spots: {e}')
        if ns.profile is not None:
            if not ns.cells:
                self.error('--profile needs --cells (it adds columns to the cell table)')
            from microbeseg_amd.inference.cells import check_profile
            try:
                ns.profile = check_profile(ns.profile)
            except ValueError as e:
                self.error(f'--profile: {e}')
        if ns.scale != 1:
            if ns.tta > 1:
                self.error('--scale and --tta > 1 cannot be combined')
            if ns.sliding_window:
                self.error('--scale and --sliding_window cannot be combined')
        return ns


def build_parser():
    parser = Parser(description='microbeSEG inference on local files (MI355X-native hot path)')
    parser.add_argument('--img_dir', '-i', required=True, type=str, help='Directory with .tif images / stacks')
    parser.add_argument('--model', '-m', required=True, type=str, help='Model to use (path without suffix)')
    parser.add_argument('--thresholds', '-t', default=[0.10, 0.45], nargs='+', type=float,
                        help='Thresholds for distance method: th_cell th_seed')
    parser.add_argument('--result_path', '-r', default=None, type=str, help='Path for saving results')
    parser.add_argument('--channel', '-c', default=0, type=int, help='Channel to segment')
    parser.add_argument('--device', '-d', default='cuda:0', type=str, help='"cuda:N"')
    parser.add_argument('--overwrite', '-o', default=False, action='store_true', help='Overwrite existing results')
    parser.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'],
                        help='[extension] bf16 = bf16 matrix-core inputs for the network (faster; masks are no longer '
                             'guaranteed identical to the fp32 reference arithmetic)')
    parser.add_argument('--sliding_window', default=False, action='store_true',
                        help='[extension] tiled inference (2048 px tiles + 128 px halo; same prediction as whole-frame '
                             'inference for the BatchNorm models training produces); lifts the 8192 px frame limit')
    parser.add_argument('--frame_batch', default=1, type=int,
                        help='[extension] frames of a stack that share one upload, one network forward and one batched '
                             'post-processing call (made for stacks of small frames, 128-512 px; capped so that a group '
                             'holds at most 2048 x 2048 pixels; same masks for fp32). 1 = frame by frame, 0 = auto')
    parser.add_argument('--clahe', default=False, action='store_true',
                        help='[extension] contrast-enhance every frame on the device before it is normalised: the CLAHE of '
                             'the reference\'s ContrastEnhancement(apply_clahe=True), i.e. scikit-image\'s '
                             'equalize_adapthist(clip_limit=0.01), bit for bit; uint8 / uint16 images only, other stacks are '
                             'segmented without it')
    parser.add_argument('--tta', default=1, type=int, choices=[1, 2, 4, 8],
                        help='[extension] test-time augmentation: every frame is predicted under K flips / rotations '
                             '(2: + left-right flip; 4: + up-down flip and 180 degrees; 8: all symmetries of the square), '
                             'the predictions are mapped back and averaged, and the average is segmented.  K network '
                             'forwards per frame; whole-frame inference only (not with --sliding_window).  1 = off')
    parser.add_argument('--scale', default=1.0, type=scale_argument,
                        help='[extension] predict at another resolution: every frame is resampled to S times its size on '
                             'the device (anti-aliased linear), predicted there, and the prediction is resampled back and '
                             'segmented at the frame\'s own resolution, so the mask has the frame\'s size and the '
                             'thresholds keep their meaning.  For images of another magnification than the training data; '
                             'S < 1 is also faster.  0.25 <= S <= 4; whole-frame inference only (not with --sliding_window '
                             'or --tta > 1).  1 = off')
    parser.add_argument('--rois', default=False, action='store_true',
                        help='[extension] also write <mask file stem>_rois.json: one polygon ROI per cell and frame, the '
                             'records the OMERO route of infer_script.py uploads (traced on the device)')
    parser.add_argument('--export', default=False, action='store_true',
                        help='[extension] also export each stack like the GUI\'s Export button: <image stem>.tif, _mask.tif, '
                             '_overlay.tif, _outlines.tif and _analysis.csv from the device-traced ROIs into '
                             '<result_path>/<image stem>_channel<c>_export/.  The exported image and overlay hold the '
                             'segmented channel only (the GUI exports every channel); uint8 / uint16 images only, other '
                             'stacks are segmented but not exported')
    parser.add_argument('--cells', default=False, action='store_true',
                        help='[extension] also write <mask file stem>_cells.csv: one row per cell and frame with area, '
                             'centroid, bounding box, axis lengths, orientation, the intensity of the measured channels '
                             '(mean, std, min, max, sum, background mean) and pred_label / overlap / track_id / '
                             'parent_track.  Tracks come from OVERLAP linking (a cell follows the cell of the previous '
                             'frame it shares the most pixels with): there is no motion model, and no gap closing unless '
                             '--gap is given')
    parser.add_argument('--measure_channels', default=None, nargs='+', type=int,
                        help='[extension] with --cells: channels of the source image to measure (default: the segmented '
                             'channel; images without a channel axis have channel 0).  uint8 / uint16 images only: other '
                             'images get the shape and link columns.  A channel an image does not have is an error')
    parser.add_argument('--min_overlap', default=1, type=int,
                        help='[extension] with --cells: links that share fewer pixels are dropped before tracks are built')
    parser.add_argument('--drift', nargs='?', const=32, default=None, type=int,
                        help='[extension] with --cells: take the stage drift out before linking.  For every frame pair the '
                             'whole-pixel shift within +-R pixels (default R = 32, 0 <= R <= 128) under which the two '
                             'masks overlap most is found on the device, cells are linked under it, and the table gains '
                             'drift_y / drift_x (the shift against frame 0) and centroid_y_reg / centroid_x_reg.  '
                             'Translation in whole pixels only: no rotation, no scaling, no registered image stack')
    parser.add_argument('--flow', nargs='?', const=8, default=None, type=int, metavar='r',
                        help='[extension] with --cells --drift: link under a tile-wise displacement field, for cells that '
                             'move against each other (a colony expanding from its centre).  Every tile of a frame gets the '
                             'whole-pixel shift within +-r pixels of the pair\'s stage drift (default r = 8, 0 <= r <= 32) '
                             'under which it overlaps the previous mask most, found on the device; cells are linked under '
                             'that field, and the table gains flow_y / flow_x (the shift of the cell\'s tile against the '
                             'previous frame, drift included).  One shift per tile: no smoothing or interpolation of the '
                             'field, no rotation, no per-cell search; gaps are closed by --gap, not by the field')
    parser.add_argument('--flow_tile', default=64, type=int, choices=[64, 128, 256],
                        help='[extension] with --flow: the tile edge in pixels (default 64)')
    parser.add_argument('--gap', nargs='?', const=1, default=None, type=int, metavar='G',
                        help='[extension] with --cells: close gaps in the tracks.  A cell that the segmentation missed in up '
                             'to G consecutive frames (default G = 1, 1 <= G <= 4) is linked to the cell that ended 2 .. G + 1 '
                             'frames before it and shares the most pixels with it, under the --drift / --flow shifts summed '
                             'over the gap (for --flow per tile index: an approximation), if they share at least '
                             '--min_overlap pixels; its track goes on, and the table gains pred_gap: the number of frames '
                             'back to the cell pred_label names (1 = an ordinary link).  Overlap only: no motion model, no '
                             'per-cell search, no rows for the missed frames')
    parser.add_argument('--hull', default=False, action='store_true',
                        help='[extension] with --cells: add the measures of every cell\'s pixel outline: perimeter (exposed '
                             'pixel edges), convex_area and solidity, feret_max / feret_min (largest and smallest caliper: '
                             'the length and width of a rod), feret_angle and the end points of the longest chord.  '
                             'Computed on the device from the pixel squares: no sub-pixel contour is fitted')
    parser.add_argument('--midline', default=False, action='store_true',
                        help='[extension] with --cells: thin every cell to its one-pixel skeleton on the device (Guo-Hall) and '
                             'add skeleton_pixels / skeleton_length / skeleton_ends / skeleton_branches, midline_length (the '
                             'skeleton\'s chain length extended to the cell\'s edge at both ends: the length of a bent or '
                             'filamentous cell, where feret_max is only its chord; NaN for branched or ring skeletons), '
                             'midline_width = area / midline_length and the two end points.  Whole pixels: no pruning, no '
                             'sub-pixel midline; for straight rods feret_max (--hull) is the better length')
    parser.add_argument('--percentiles', nargs='*', default=None, type=int, metavar='P',
                        help='[extension] with --cells: add p{P}_ch{c}, the P-th percentile of every cell\'s pixel values '
                             'per measured channel, and bg_p{P}_ch{c}, the same over the frame\'s background (label 0): the '
                             'robust counterparts of mean / max / bg_mean.  1 to 8 distinct whole numbers in 0 .. 100; the '
                             'bare flag means 50, the median.  Exact order statistics from the device, linear '
                             'interpolation as numpy\'s default; uint8 / uint16 images')
    parser.add_argument('--neighbors', nargs='?', const=8, default=None, type=int, metavar='R',
                        help='[extension] with --cells: add every cell\'s neighbourhood within its frame: contact_length / '
                             'border_length / contact_fraction (pixel edges shared with other cells, with the frame\'s border, '
                             'and the share of the former in the perimeter), n_touching, n_neighbors (cells within R pixels, '
                             'default R = 8, 1 <= R <= 32), nn_label / nn_distance / nn_gap (the nearest of them) and '
                             'contact_label / contact_max (the cell sharing the most edges); also write <mask file '
                             'stem>_contacts.csv, one row per pair of cells within R: frame, label_a, label_b, contact, '
                             'distance.  Whole pixels, centre-to-centre distances: no sub-pixel contour, nothing beyond R, no '
                             'Voronoi or Delaunay neighbourhood')
    parser.add_argument('--spots', default=None, type=int, metavar='THR',
                        help='[extension] with --cells: add every cell\'s fluorescent foci per measured channel: n_spots_ch{c}, '
                             'the local maxima of an exact band-pass response (difference of two binomial smoothings) of at '
                             'least THR grey levels (1 .. 65535) under the cell, spot_max_ch{c} / spot_sum_ch{c}, their '
                             'largest and summed response, and bg_spots_ch{c}, the frame\'s spots on the background; also '
                             'write <mask file stem>_spots.csv, one row per spot on a cell: frame, channel, label, y, x, '
                             'value, response, axis_pos, axis_off (the position along and across the cell, +-1 = the poles; '
                             'the sign of axis_pos is arbitrary).  Whole pixels, a fixed threshold: no sub-pixel fit, no '
                             'automatic threshold, no linking of spots over time; uint8 / uint16 images')
    parser.add_argument('--spot_scale', default=2, type=int, metavar='S',
                        help='[extension] with --spots: the size of the foci, 1 .. 5 (default 2): the band-pass is the '
                             'difference of Gaussians with sigma = sqrt(S / 2) and sqrt(S) pixels')
    parser.add_argument('--profile', nargs='?', const=16, default=None, type=int, metavar='N',
                        help='[extension] with --cells: add where along the cell the signal of every measured channel sits, for '
                             'signals that form no foci (a polar cap, a septal band, a gradient).  Every cell\'s pixels are '
                             'projected on its orientation and the projected extent is cut into N bins from pole to pole '
                             '(default N = 16, 2 <= N <= 32), on the device; the table gains axis_extent (the pole-to-pole '
                             'length in pixels), pole_mid_ratio_ch{c} (mean of the outer quarters over the mean of the rest), '
                             'pole_asym_ch{c} (0 = both poles alike, 1 = all at one pole) and profile_peak_ch{c} (the centre of '
                             'the brightest bin, -1 .. 1; the sign is arbitrary); also write <mask file stem>_profiles.csv, one '
                             'row per cell, channel and bin: frame, channel, label, bin, bin_pos, count, sum, mean.  Whole '
                             'pixels, along the straight orientation axis: a bent cell is folded onto its chord; no '
                             'background subtraction, no normalisation across cells, no demograph image; uint8 / uint16 images')
    return parser


def measured_channels(args, img):
    """channels of ``img`` that --cells measures: --measure_channels, else the segmented channel (0 without channel axis)"""
    if args.measure_channels is not None:
        return list(args.measure_channels)
    has_axis = img.ndim == 4 or (img.ndim == 3 and 3 in (img.shape[0], img.shape[-1]))
    return [args.channel if has_axis else 0]


def main():
    args = build_parser().parse_args()

    imgs_path = Path(args.img_dir)
    result_path = (Path(__file__).parent / 'results') if args.result_path is None else Path(args.result_path)
    result_path.mkdir(exist_ok=True)
    if len(args.thresholds) != 2:
        raise Exception(f"{len(args.thresholds)} threshold given, needed are 2")
    if 'cuda' in args.device and not torch.cuda.is_available():
        raise ValueError('No MI355X visible: this build has no CPU inference path')

    from microbeseg_amd.inference.infer import InferWorker
    from microbeseg_amd.utils import tiffio as tiff

    file_ids = sorted(imgs_path.glob('*.tif*'))
    if len(file_ids) == 0:
        print('No files found')
        return
    if args.cells:                      # a channel an image does not have stops the run before any inference
        for img_id in file_ids:
            img = tiff.imread(str(img_id))
            select_channels(img, measured_channels(args, img), img_id.name)
        del img
    worker = InferWorker(model=args.model, device=args.device, ths=args.thresholds, channel=args.channel,
                         sliding_window=args.sliding_window)
    worker.precision = args.precision
    worker.frame_batch = args.frame_batch
    worker.apply_clahe = args.clahe
    worker.min_overlap = args.min_overlap
    worker.drift = args.drift
    worker.flow = args.flow
    worker.flow_tile = args.flow_tile
    worker.gap = args.gap
    worker.hull = args.hull
    worker.midline = args.midline
    worker.percentiles = tuple(args.percentiles) if args.percentiles else None
    worker.neighbors = args.neighbors
    worker.spots = args.spots
    worker.spot_scale = args.spot_scale
    worker.profile = args.profile
    worker.tta = args.tta
    worker.scale = args.scale
    if args.drift is not None:
        print(f'Cell table: linking under the stage drift found within +-{args.drift} px per frame pair')
    if args.flow is not None:
        print(f'Cell table: linking under a displacement field of {args.flow_tile} px tiles, each searched within '
              f'+-{args.flow} px of the stage drift')
    if args.gap is not None:
        print(f'Cell table: closing gaps of up to {args.gap} missed frame(s) in the tracks')
    if args.hull:
        print('Cell table: with the outline measures (perimeter, convex hull, Feret length / width / angle)')
    if args.midline:
        print('Cell table: with the midline measures (thinned skeleton, midline length / width, end points)')
    if args.percentiles:
        print('Cell table: with the percentiles ' + ', '.join(str(q) for q in args.percentiles) +
              ' of every cell and of the background per measured channel')
    if args.neighbors is not None:
        print(f'Cell table: with the neighbourhood of every cell within {args.neighbors} px (contacts, nearest neighbour); '
              'the pairs go to ..._contacts.csv')
    if args.spots is not None:
        print(f'Cell table: with the fluorescent foci of every cell (response >= {args.spots} grey levels at scale '
              f'{args.spot_scale}); the spots go to ..._spots.csv')
    if args.profile is not None:
        print(f'Cell table: with the intensity profile of every cell along its axis in {args.profile} bins; the profiles go '
              'to ..._profiles.csv')
    if args.scale != 1:
        print(f'Inference at {args.scale} x the resolution of the frames')
    if args.tta > 1:
        print(f'Test-time augmentation: {args.tta} network forwards per frame')
    worker.text_output.connect(print)
    torch.set_grad_enabled(False)
    print('--- Start inference ---')
    for img_id in file_ids:
        out_file = result_path / f"mask_{img_id.stem}_channel{args.channel}.tif"
        img = tiff.imread(str(img_id))
        frames = select_frames(img, args.channel, img_id.name)
        if frames is None:
            continue
        if out_file.is_file() and not args.overwrite:
            print(f'Skip {img_id.stem} (already processed and overwriting not enabled)')
            continue
        export = args.export
        if export and frames.dtype not in (np.uint8, np.uint16):
            print(f'Skip export of {img_id.stem} (the overlay needs uint8 / uint16 images, got {frames.dtype})')
            export = False
        print(f'Process {img_id.stem} (channel: {args.channel})')
        results = worker.infer_stack(frames)
        tiff.imwrite(str(out_file), np.squeeze(results))
        if args.rois or export:
            rois = [roi for t in range(len(results)) for roi in worker.polygon_rois(results[t], t)]
        if args.rois:
            import json
            with open(out_file.with_name(out_file.stem + '_rois.json'), 'w', encoding='utf-8') as f:
                json.dump({'image': img_id.name, 'channel': args.channel, 'rois': rois}, f)
        if export:
            from microbeseg_amd.inference.result_export import export_local
            export_local(frames, rois, result_path / f"{img_id.stem}_channel{args.channel}_export", img_id.name)
        if args.cells:
            from microbeseg_amd.inference.cells import write_cells
            channels = measured_channels(args, img)
            view = select_channels(img, channels, img_id.name)
            if view.dtype not in (np.uint8, np.uint16):
                print(f'Skip intensity columns of {img_id.stem} (they need uint8 / uint16 images, got {view.dtype})')
                view, channels = None, []
            worker.spots = args.spots if view is not None else None      # the spot columns are intensity columns
            worker.profile = args.profile if view is not None else None  # so are the profile columns
            write_cells(worker.cell_table(results, view, channels), out_file.with_name(out_file.stem + '_cells.csv'))
            if args.neighbors is not None:
                write_cells(worker.contact_table(results), out_file.with_name(out_file.stem + '_contacts.csv'))
            if worker.spots is not None:
                write_cells(worker.spot_table(results, view, channels), out_file.with_name(out_file.stem + '_spots.csv'))
            if worker.profile is not None:
                write_cells(worker.profile_table(results, view, channels),
                            out_file.with_name(out_file.stem + '_profiles.csv'))
    print('--- Finished ---')


if __name__ == "__main__":
    main()
