#!/opt/conda/bin/python3.9
"""Generate tests/golden/cells_regionprops.npz with scikit-image's own regionprops (0.18.3 in the conda environment).

Run:  PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 -W ignore tools/gen_golden_cells.py
Each case is one label frame (uint16) plus one intensity image (uint16) and, per present label in ascending order, the
library's regionprops(label, intensity_image) values: area, centroid, bbox, major_axis_length, minor_axis_length,
orientation, mean_intensity, min_intensity, max_intensity.  Cases: elongated random ellipses, touching cells, 1-pixel and
2 x 2 cells among other tiny ones, cells on the border.
"""
import pathlib
import sys

import numpy as np
from skimage.draw import ellipse
from skimage.measure import regionprops

sys.dont_write_bytecode = True
OUT = pathlib.Path(__file__).resolve().parents[1] / "tests" / "golden" / "cells_regionprops.npz"
H, W = 96, 128


def ellipses(rng, n, border=False):
    lab = np.zeros((H, W), np.uint16)
    k = 0
    for _ in range(400):
        if k == n:
            break
        major, minor = rng.uniform(6, 14), rng.uniform(2, 4.5)          # elongated: a well-defined angle
        cy, cx = (rng.uniform(-3, H + 3), rng.uniform(-3, W + 3)) if border else (rng.uniform(16, H - 16),
                                                                                  rng.uniform(16, W - 16))
        rr, cc = ellipse(cy, cx, major, minor, shape=(H, W), rotation=rng.uniform(-np.pi / 2, np.pi / 2))
        if rr.size < 12 or lab[max(rr.min() - 1, 0):rr.max() + 2, max(cc.min() - 1, 0):cc.max() + 2].any():
            continue
        if border and not (rr.min() == 0 or cc.min() == 0 or rr.max() == H - 1 or cc.max() == W - 1) and k % 2 == 0:
            continue
        k += 1
        lab[rr, cc] = k
    return lab


def touching(rng):
    """long cells cut into touching pieces, and a block of touching stripes"""
    lab = np.zeros((H, W), np.uint16)
    k = 0
    for cy, cx, rot in ((20, 30, 0.3), (25, 90, -0.8), (60, 40, 1.2), (70, 100, 0.1)):
        rr, cc = ellipse(cy, cx, 18, 5, shape=(H, W), rotation=rot)
        cut = (rr * np.cos(rot) + cc * np.sin(rot)) > (cy * np.cos(rot) + cx * np.sin(rot)) + rng.uniform(-3, 3)
        lab[rr[cut], cc[cut]] = k + 1
        lab[rr[~cut], cc[~cut]] = k + 2
        k += 2
    for i in range(5):
        lab[82:93, 10 + 4 * i:14 + 4 * i] = k + 1 + i
    return lab


def small():
    lab = np.zeros((H, W), np.uint16)
    k = 0
    for y, x in ((3, 3), (3, 5), (10, 127), (95, 0), (40, 41), (41, 42)):     # 1-pixel cells, two of them diagonal neighbours
        k += 1
        lab[y, x] = k
    k += 1
    lab[20:22, 20:22] = k                                                     # 2 x 2: no defined angle
    for sl in ((slice(30, 31), slice(10, 13)), (slice(30, 33), slice(20, 21)), (slice(50, 52), slice(60, 65)),
               (slice(60, 67), slice(70, 72)), (slice(70, 71), slice(5, 7))):
        k += 1
        lab[sl] = k
    k += 1
    lab[80:83, 80] = k
    lab[82, 80:84] = k                                                        # an L
    return lab


def main():
    rng = np.random.default_rng(20240611)
    cases = {"ellipses": ellipses(rng, 24), "touching": touching(rng), "small": small(),
             "border": ellipses(rng, 14, border=True)}
    out = {"names": np.array(list(cases))}
    for name, lab in cases.items():
        img = rng.integers(0, 65536, (H, W)).astype(np.uint16)
        img[::7, ::5] = 65535
        img[3::11, 1::3] = 0
        props = regionprops(lab.astype(np.int32), intensity_image=img)
        out[f"{name}_label"] = lab
        out[f"{name}_img"] = img
        out[f"{name}_ids"] = np.array([p.label for p in props], np.int64)
        out[f"{name}_area"] = np.array([p.area for p in props], np.int64)
        out[f"{name}_centroid"] = np.array([p.centroid for p in props], np.float64)
        out[f"{name}_bbox"] = np.array([p.bbox for p in props], np.int64)
        out[f"{name}_major"] = np.array([p.major_axis_length for p in props], np.float64)
        out[f"{name}_minor"] = np.array([p.minor_axis_length for p in props], np.float64)
        out[f"{name}_orientation"] = np.array([p.orientation for p in props], np.float64)
        out[f"{name}_mean"] = np.array([p.mean_intensity for p in props], np.float64)
        out[f"{name}_min"] = np.array([p.min_intensity for p in props], np.int64)
        out[f"{name}_max"] = np.array([p.max_intensity for p in props], np.int64)
        print(name, len(props), "cells")
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
