#!/usr/bin/env python3
"""Writes tests/golden/clahe_library.npz: synthetic images and what scikit-image's CLAHE makes of them, exactly as the
reference calls it (src/training/mytransforms.py:92-95, src/inference/inference_dataset.py:63-77):

    (65535 * equalize_adapthist(np.squeeze(img), clip_limit=0.01)).astype(np.uint16)

Needs an interpreter with scikit-image (the reference pins 0.18.3); the version used is recorded in the file.  The test
suite only reads the file (tests/test_clahe_host.py, tests/test_gpu_clahe.py).

    python tools/gen_golden_clahe.py [--out tests/golden/clahe_library.npz]
"""
import argparse
import pathlib

import numpy as np
import skimage
from skimage.exposure import equalize_adapthist

ROOT = pathlib.Path(__file__).resolve().parents[1]


def textured(rng, h, w, dtype=np.uint16, lo=300, hi=9000):
    """smooth illumination gradient + a few bright blobs + noise: every tile gets a different histogram"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = lo + (hi - lo) * (0.25 + 0.2 * np.sin(x / (0.21 * w + 1)) * np.cos(y / (0.17 * h + 1)))
    for _ in range(max(3, h * w // 600)):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1.5, 0.12 * min(h, w) + 2)
        img += (hi - lo) * rng.uniform(0.2, 0.6) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    img += rng.normal(0, 0.02 * (hi - lo), (h, w))
    top = np.iinfo(dtype).max
    return np.clip(img, 0, top).astype(dtype)


def sparse_blobs(rng, h, w):
    """a nearly flat background (three grey levels) with a handful of cells: most tiles clip almost everything"""
    img = (500 + rng.integers(0, 3, (h, w))).astype(np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, 6)
        img += 4000 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    return img.astype(np.uint16)


def cases():
    rng = np.random.default_rng(20240917)
    yield "c1_32x32_u16", textured(rng, 32, 32)
    yield "c2_40x56_u16", textured(rng, 40, 56)
    yield "c3_67x93_u16", textured(rng, 67, 93, hi=40000)
    yield "c4_100x130_u16_blobs", sparse_blobs(rng, 100, 130)
    yield "c5_64x64_u8", textured(rng, 64, 64, dtype=np.uint8, lo=10, hi=200)
    yield "c6_32x32_u16_const", np.full((32, 32), 500, np.uint16)
    yield "c7_256x256_u16", textured(rng, 256, 256, hi=30000)
    yield "c8_16x24_u16", textured(rng, 16, 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "clahe_library.npz"))
    args = ap.parse_args()
    data = {"skimage_version": np.array(skimage.__version__), "names": None}
    names = []
    for name, img in cases():
        out = (65535 * equalize_adapthist(np.squeeze(img), clip_limit=0.01)).astype(np.uint16)
        data["in_" + name], data["out_" + name] = img, out
        names.append(name)
        print(f"{name}: {img.dtype} {img.shape} -> out {int(out.min())}..{int(out.max())}")
    data["names"] = np.array(names)
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out} ({pathlib.Path(args.out).stat().st_size} bytes), scikit-image {skimage.__version__}")


if __name__ == "__main__":
    main()
