#!/usr/bin/env python3
"""Generate tests/golden/prepare_crops.npz and prepare_import.npz.

Run with an interpreter that has numpy and scikit-image (the real skimage.draw.polygon / polygon_perimeter):
    PYTHONDONTWRITEBYTECODE=1 python3 -W ignore tools/gen_golden_prepare.py
The crop / import arithmetic is the numpy restatement of tests/prepare_ref.py (reference src/utils/data_cropping.py:
157-264,286, src/utils/data_import.py:125-194, src/utils/data_export.py:61-70,100-101); contours come from
oracle/contour_ref.py (OpenCV is not available, as for DESIGN.md §6e), instance masks of the pre-labelling case from the C
oracle of the post-processing (oracle/postproc_ref.py).  Only inputs and expected outputs are stored.
"""
import pathlib
import random
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = ROOT / "tests" / "golden"
S = 64

import prepare_ref as R  # noqa: E402
from oracle import contour_ref  # noqa: E402
from skimage.draw import polygon, polygon_perimeter  # noqa: E402


def rois_and_outlines(mask):
    """data_cropping.py:217-235: ROI strings in iteration order and the outlines of one predicted crop"""
    rois, outlines = [], np.zeros(mask.shape, bool)
    for polys in contour_ref.label_polygons(mask).values():
        for p in polys:
            rois.append(contour_ref.points_string(p))
            rr, cc = polygon_perimeter(p[0], p[1], shape=mask.shape, clip=True)
            outlines[rr, cc] = True
    return rois, outlines


def round_trip(mask_crop):
    """data_import.py:240-253 then data_export.py:61-70,127-145 -> uint16 mask, number of polygons"""
    out = np.zeros(mask_crop.shape, np.uint16)
    cell_id = 1
    for polys in contour_ref.label_polygons(mask_crop).values():
        for p in polys:
            r, c = [], []
            for token in contour_ref.points_string(p).split(' '):
                xy = token.split(',')
                if len(xy) == 1:
                    continue
                r.append(min(max(int(round(float(xy[1]))), 0), mask_crop.shape[1] - 1))
                c.append(min(max(int(round(float(xy[0]))), 0), mask_crop.shape[1] - 1))
            rr, cc = polygon(r, c)
            out[rr, cc] = cell_id
            cell_id += 1
    return out, cell_id - 1


def crops_fixture():
    fx = {"shapes": np.asarray(R.SHAPES, np.int32), "crop_size": np.int32(S)}
    branches = set()
    for i, shape in enumerate(R.SHAPES):
        frame = R.frame_for(shape, np.uint16, 100 + i)
        fx[f"frame_{i}"] = frame
        for seed in (1, 2, 3):
            got = R.origins_ref(frame, S, random.Random(seed))
            fx[f"origins_s{seed}_{i}"] = np.zeros((0, 2), np.int32) if got is None else np.asarray(got[1], np.int32)
            if got is None:
                branches.add("skipped")
                continue
            padded, origins = got
            branches.add(f"{len(origins)} crops")
            if padded.shape != frame.shape:
                if padded.shape[0] != frame.shape[0]:
                    branches.add("padded y")
                if padded.shape[1] != frame.shape[1]:
                    branches.add("padded x")
                if len(origins) == 3:
                    branches.add("padded plus three crops")
            if all(o == (0, 0) for o in origins):
                branches.add("zero origins")
            if any(a == padded.shape[0] - S and padded.shape[0] > S or b == padded.shape[1] - S and padded.shape[1] > S
                   for a, b in origins):
                branches.add("last valid position")
            if seed != 1:
                continue
            lo, hi = np.min(frame), np.max(frame)
            img, show, x, _ = R.crop_views(padded, origins, S, lo, hi)
            fx[f"img_{i}"], fx[f"show_{i}"] = img, show
            if shape in ((60, 75), (75, 225), (58, 300)):
                fx[f"x_{i}"] = x
            fx[f"stats_{i}"] = np.asarray([str(lo), str(hi), str(np.mean(frame)), str(np.std(frame))])
    want = {"skipped", "1 crops", "2 crops", "3 crops", "padded y", "padded x", "padded plus three crops",
            "zero origins", "last valid position"}
    assert want <= branches, want - branches

    # pre-labelling: the three crops of frame (75, 225) with synthetic prediction maps, one of them quantised
    from microbeseg_amd.utils import synth
    from oracle import postproc_ref
    rng = np.random.Generator(np.random.PCG64(77))
    borders, cells, masks, outl, shows, n_rois = [], [], [], [], [], []
    show3 = fx["show_3"]
    for k in range(3):
        cell, border = synth.synth_prediction_maps(rng, S, S, 6 + k, rmin=3.0, rmax=7.0)
        if k == 1:
            cell = (np.round(cell * 16) / 16).astype(np.float32)
        mask = postproc_ref.distance_postprocessing(border[..., None], cell[..., None], 0.45, 0.10)
        assert int(mask.max()) >= 5, int(mask.max())
        rois, outlines = rois_and_outlines(mask)
        borders.append(border.astype(np.float32)), cells.append(cell.astype(np.float32)), masks.append(mask)
        outl.append(outlines), shows.append(R.overlay_ref(show3[k], outlines)), n_rois.append(len(rois))
        fx[f"pl_rois_{k}"] = np.asarray(rois)
    fx.update(pl_border=np.stack(borders), pl_cell=np.stack(cells), pl_mask=np.stack(masks).astype(np.uint16),
              pl_outlines=np.stack(outl), pl_roi_show=np.stack(shows), pl_ths=np.asarray([0.10, 0.45], np.float32))
    np.savez_compressed(OUT / "prepare_crops.npz", **fx)
    print("prepare_crops.npz:", sorted(branches), "rois", n_rois)


def import_fixture():
    fx = {"crop_size": np.int32(S)}
    cases = {}
    # A: uint16, remainders 22 (even, y) and 11 (odd, x): trimmed rows 11..139, columns 5..197; grid 2 x 3
    cells_a = [(1, 40, 40, 12, 9), (255, 30, 69, 8, 10), (256, 75, 100, 9, 14), (65535, 100, 30, 10, 8),
               (7, 74, 68, 9, 9),            # spans four crops (corner at row 75, column 69)
               (12, 60, 180, 9, 6), (13, 40, 150, 7, 7),      # crop (1, 2) stays empty
               (300, 5, 100, 3, 20),         # lies in the trimmed border only
               (14, 135, 120, 3, 3)]         # a small cell in crop (1, 1)
    mask_a = R.cell_mask((150, 203), cells_a, 0)
    cases["A"] = (R.frame_for((150, 203), np.uint16, 41), mask_a)
    # B: uint8 image, uint8 mask, remainders 7 (odd, y) and 12 (even, x); grid 2 x 2, one crop empty, one nearly empty
    cells_b = [(3, 30, 30, 12, 12), (4, 40, 100, 10, 13), (200, 100, 100, 14, 9), (5, 70, 38, 2, 2)]
    cases["B"] = (R.frame_for((135, 140), np.uint8, 42), R.cell_mask((135, 140), cells_b, 0).astype(np.uint8))
    # C: smaller than the crop on both axes (pads 14 and 5: centred, the odd pixel at the left)
    cases["C"] = (R.frame_for((50, 59), np.uint16, 43), R.cell_mask((50, 59), [(1, 20, 20, 8, 8), (2, 35, 45, 6, 9)], 0))
    # D: too much pads; E: empty mask; F: exactly one crop
    cases["D"] = (R.frame_for((20, 64), np.uint16, 44), R.cell_mask((20, 64), [(1, 10, 30, 5, 5)], 0))
    cases["E"] = (R.frame_for((64, 64), np.uint16, 45), np.zeros((64, 64), np.uint16))
    cases["F"] = (R.frame_for((64, 64), np.uint16, 46), R.cell_mask((64, 64), [(1, 20, 20, 8, 8), (2, 40, 45, 9, 9),
                                                                                 (3, 41, 21, 1, 1)], 0))
    accepted = rej_empty = rej_small = 0
    for name, (img, mask) in cases.items():
        fx[f"img_{name}"], fx[f"mask_{name}"] = img, mask
        for keep in (False, True):
            tag = f"{name}_keep" if keep else name
            ref = None if int(mask.max()) == 0 else R.import_ref(img, mask, S, keep)
            fx[f"skipped_{tag}"] = np.bool_(ref is None)
            if ref is None:
                continue
            fx[f"stats_{tag}"] = np.asarray([str(ref["min_frame"]), str(ref["max_frame"]), str(ref["mean_frame"]),
                                             str(ref["std_frame"])])
            offs, u16, rt, raw, npoly = [], [], [], [], []
            for img_crop, mask_crop, x_start, y_start in ref["crops"]:
                offs.append((x_start, y_start))
                u16.append(R.export_image_ref(img_crop, ref["min_frame"], ref["max_frame"]))
                m, n = round_trip(mask_crop)
                rt.append(m), raw.append(mask_crop), npoly.append(n)
            fx[f"offsets_{tag}"] = np.asarray(offs, np.int32).reshape(-1, 2)
            fx[f"u16_{tag}"] = np.stack(u16) if u16 else np.zeros((0, S, S), np.uint16)
            if not keep:
                fx[f"roundtrip_{name}"] = np.stack(rt) if rt else np.zeros((0, S, S), np.uint16)
                fx[f"rawmask_{name}"] = np.stack(raw) if raw else np.zeros((0, S, S), mask.dtype)
                fx[f"npoly_{name}"] = np.asarray(npoly, np.int32)
                accepted += len(offs)
                rej_empty += ref["rejected_empty"]
                rej_small += ref["rejected_small"]
                print(name, "accepted", offs, "rejected empty / small", ref["rejected_empty"], ref["rejected_small"],
                      "polygons", npoly)
    assert accepted >= 4 and rej_empty >= 1 and rej_small >= 1, (accepted, rej_empty, rej_small)
    # the ids named by the census test, an id that spans four crops, one present in the trimmed border only
    trimmed = mask_a[11:139, 5:197]
    assert {1, 255, 256, 65535} <= set(np.unique(trimmed).tolist()) and 300 in mask_a and 300 not in trimmed
    assert all(7 in trimmed[y:y + 64, x:x + 64] for y in (0, 64) for x in (0, 64))
    assert bool(fx["skipped_D"]) and bool(fx["skipped_E"])
    np.savez_compressed(OUT / "prepare_import.npz", **fx)


if __name__ == "__main__":
    crops_fixture()
    import_fixture()
    for f in ("prepare_crops.npz", "prepare_import.npz"):
        print(f, (OUT / f).stat().st_size, "bytes")
