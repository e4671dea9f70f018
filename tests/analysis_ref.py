"""numpy / scipy restatement of the reference's Analysis / Export loops (src/inference/analysis.py:112-170,
src/inference/result_export.py:112-190): ROI strings -> filled uint16/int32 stack + outlines -> per-frame relabel ->
per-frame statistics, and the RGB overlay.  It is the CPU checker of the HIP pipeline (microbeseg_amd/csrc/analysis.hip)
and is itself pinned to the reference's own outputs by tests/golden/analysis_*.npz.

Pixel rule of skimage.draw.polygon (0.18.3, recovered by probing): the O'Rourke crossing test on the
bounding box rows int(max(0, min r)) .. ceil(max r) and columns likewise.  For pixel (y, x) and every edge (j -> i) of the
closed polygon, with x0 = c_i - x, y0 = r_i - y, x1 = c_j - x, y1 = r_j - y:
  x0 == 0 and y0 == 0                                    -> vertex: the pixel is filled;
  (y0 > 0) != (y1 > 0) and (x0*y1 - x1*y0)/(y1 - y0) > 0 -> one right crossing;
  (y0 < 0) != (y1 < 0) and (x0*y1 - x1*y0)/(y1 - y0) < 0 -> one left crossing;
the pixel is filled iff the right or the left crossing count is odd (inside, or 'edge' when the parities differ).
"""
import numpy as np

from oracle.eval_ref import label_image

WRAP_FIRST, CAST_AT = 65536, 66535   # uint16 wrap of cell ids 65536..66534; the stack becomes int32 at cell_id == 66535


def make_coordinates(polystr, size_x, size_y):
    r, c = [], []
    for tok in polystr.split(' '):
        xy = tok.split(',')
        if len(xy) == 1:
            continue
        r.append(min(max(int(round(float(xy[1]))), 0), size_y - 1))
        c.append(min(max(int(round(float(xy[0]))), 0), size_x - 1))
    return r, c


def _fill_batch(polys):
    """polys: list of (r, c) int arrays -> list of (rr, cc); vectorised over polygons padded to a common shape (the last
    vertex repeated: a zero-length edge neither crosses nor adds a vertex)."""
    nv = max(len(r) for r, _ in polys)
    P = len(polys)
    R = np.empty((P, nv), np.float64)
    Cc = np.empty((P, nv), np.float64)
    for k, (r, c) in enumerate(polys):
        R[k, :len(r)] = r
        R[k, len(r):] = r[-1]
        Cc[k, :len(c)] = c
        Cc[k, len(c):] = c[-1]
    r0 = np.maximum(0, R.min(1)).astype(np.int64)
    c0 = np.maximum(0, Cc.min(1)).astype(np.int64)
    bh = int((np.ceil(R.max(1)).astype(np.int64) - r0).max()) + 1
    bw = int((np.ceil(Cc.max(1)).astype(np.int64) - c0).max()) + 1
    y = (r0[:, None, None] + np.arange(bh)[None, :, None]).astype(np.float64)
    x = (c0[:, None, None] + np.arange(bw)[None, None, :]).astype(np.float64)
    y, x = np.broadcast_to(y, (P, bh, bw)), np.broadcast_to(x, (P, bh, bw))
    rc = np.zeros((P, bh, bw), np.int32)
    lc = np.zeros((P, bh, bw), np.int32)
    vert = np.zeros((P, bh, bw), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(nv):
            j = i - 1 if i else nv - 1
            x0 = Cc[:, i, None, None] - x
            y0 = R[:, i, None, None] - y
            x1 = Cc[:, j, None, None] - x
            y1 = R[:, j, None, None] - y
            vert |= (x0 == 0) & (y0 == 0)
            q = (x0 * y1 - x1 * y0) / (y1 - y0)
            rc += ((y0 > 0) != (y1 > 0)) & (q > 0)
            lc += ((y0 < 0) != (y1 < 0)) & (q < 0)
    inside = vert | (rc & 1).astype(bool) | (lc & 1).astype(bool)
    rmax = np.ceil(R.max(1)).astype(np.int64)
    cmax = np.ceil(Cc.max(1)).astype(np.int64)
    inside &= y <= rmax[:, None, None]
    inside &= x <= cmax[:, None, None]
    out = []
    for k in range(P):
        yy, xx = np.nonzero(inside[k])
        out.append((yy + r0[k], xx + c0[k]))
    return out


def fill_polygons(polys, chunk=256):
    """skimage.draw.polygon(r, c) (no shape) for every polygon of the list -> list of (rr, cc) in raster order."""
    if not polys:
        return []
    polys = [(np.asarray(r, np.int64), np.asarray(c, np.int64)) for r, c in polys]
    area = [(int(np.ptp(r)) + 1) * (int(np.ptp(c)) + 1) * len(r) for r, c in polys]
    order = np.argsort(area, kind="stable")
    out = [None] * len(polys)
    for s in range(0, len(order), chunk):
        idx = order[s:s + chunk]
        for k, rc in zip(idx, _fill_batch([polys[i] for i in idx])):
            out[k] = rc
    return out


def line(r0, c0, r1, c1):
    """skimage.draw.line (Bresenham, _draw.pyx _line)"""
    steep = False
    r, c = r0, c0
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sc = 1 if c1 - c > 0 else -1
    sr = 1 if r1 - r > 0 else -1
    if dr > dc:
        steep = True
        r, c, dr, dc, sr, sc = c, r, dc, dr, sc, sr
    d = 2 * dr - dc
    rr, cc = [], []
    for _ in range(dc):
        rr.append(r)                       # (r, c) are swapped back below for a steep line
        cc.append(c)
        while d >= 0:
            r += sr
            d -= 2 * dc
        c += sc
        d += 2 * dr
    if steep:
        rr, cc = cc, rr
    rr.append(r1)
    cc.append(c1)
    return np.array(rr, np.int64), np.array(cc, np.int64)


def perimeter(r, c, shape):
    """polygon_perimeter(r, c, shape, clip=True) for clamped integer vertices: Bresenham along every edge of the closed
    polygon, in-image pixels only (also defined here for < 3 distinct vertices, where the reference raises)."""
    rr, cc = [], []
    n = len(r)
    for i in range(n):
        a, b = line(int(r[i]), int(c[i]), int(r[(i + 1) % n]), int(c[(i + 1) % n]))
        rr.append(a)
        cc.append(b)
    rr, cc = np.concatenate(rr), np.concatenate(cc)
    keep = (rr >= 0) & (rr < shape[0]) & (cc >= 0) & (cc < shape[1])
    return rr[keep], cc[keep]


def cell_value(k):
    """value the reference's stack holds for the k-th polygon (1-based over the whole stack)"""
    return k & 0xFFFF if WRAP_FIRST <= k < CAST_AT else k


def rois_to_masks(coords, T, H, W):
    """coords: [(t, r, c), ...] in iteration order -> (mask uint16 / int32 [T,H,W] after the per-frame relabel,
    outlines bool [T,H,W]) exactly as analysis.py:112-144."""
    owner = np.zeros((T, H, W), np.int64)
    outl = np.zeros((T, H, W), bool)
    fills = fill_polygons([(r, c) for _, r, c in coords])
    for k, ((t, r, c), (rr, cc)) in enumerate(zip(coords, fills), start=1):
        owner[t, rr, cc] = k
        pr, pc = perimeter(r, c, (H, W))
        outl[t, pr, pc] = True
    vals = np.zeros(len(coords) + 1, np.int64)
    vals[1:] = [cell_value(k) for k in range(1, len(coords) + 1)]
    filled = vals[owner]
    cast = len(coords) + 1 >= CAST_AT
    lab = np.stack([label_image(f) for f in filled]) if T else filled
    if cast:
        mask = lab.astype(np.uint16) if lab.max(initial=0) <= 65535 else lab.astype(np.int32)
    else:
        mask = lab.astype(np.uint16)
    return mask, outl


def region_axes(frame):
    """-> (areas, major, minor) per label 1..max of one relabelled frame, as regionprops area / axis_major_length /
    axis_minor_length (inertia tensor eigenvalues, 4 sqrt(lambda))"""
    f = np.asarray(frame).astype(np.int64)
    K = int(f.max(initial=0))
    ys, xs = np.nonzero(f)
    lab = f[ys, xs]
    n = np.bincount(lab, minlength=K + 1)[1:].astype(np.int64)
    s = {}
    for name, v in (("y", ys), ("x", xs), ("yy", ys * ys), ("xx", xs * xs), ("xy", xs * ys)):
        s[name] = np.bincount(lab, weights=v.astype(np.float64), minlength=K + 1)[1:].astype(np.int64)
    major, minor = np.zeros(K), np.zeros(K)
    for i in range(K):
        if n[i] == 0:
            continue
        nn = float(n[i]) ** 2
        a = (n[i] * s["yy"][i] - s["y"][i] ** 2) / nn
        c = (n[i] * s["xx"][i] - s["x"][i] ** 2) / nn
        b = (n[i] * s["xy"][i] - s["x"][i] * s["y"][i]) / nn
        ev = np.clip(np.linalg.eigvalsh(np.array([[c, -b], [-b, a]])), 0, None)
        major[i], minor[i] = 4 * np.sqrt(ev[1]), 4 * np.sqrt(ev[0])
    return n[n > 0], major[n > 0], minor[n > 0]


def analyze(mask):
    """the results dict of analysis.py:151-167 (np.mean of empty lists -> NaN)"""
    res = {k: [] for k in ("frame", "counts", "mean_area", "total_area", "mean_minor_axis_length",
                           "mean_major_axis_length")}
    with np.errstate(invalid="ignore", divide="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for t in range(len(mask)):
                res["frame"].append(t)
                res["counts"].append(int(np.max(mask[t])))
                res["total_area"].append(int(np.sum(mask[t])))
                a, M, m = region_axes(mask[t])
                res["mean_area"].append(np.mean(a.astype(np.int64)))
                res["mean_minor_axis_length"].append(np.mean(m))
                res["mean_major_axis_length"].append(np.mean(M))
    return res


def overlay(img, outlines):
    """result_export.py:183-190"""
    img = np.asarray(img)
    ov = np.clip(255 * img.astype(np.float32) / np.max(img), 0, 255).astype(np.uint8)
    if img.ndim == 3:
        ov = np.concatenate((ov[..., None], ov[..., None], ov[..., None]), axis=-1)
    ov[outlines, 0] = 255
    ov[outlines, 1] = 255
    ov[outlines, 2] = 0
    return ov
