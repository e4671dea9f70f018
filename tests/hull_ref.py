"""Plain numpy / Python-integer restatement of the per-cell outline measures (include/mseg_hip.h: mseg_cell_hull; DESIGN.md
§6p), written from the definitions: a cell is the union of the closed unit squares of its pixels, its corners are integer
points.  ``brute`` is the definition itself, O(corners^3); ``andrew`` is the textbook monotone chain over ALL corners sorted
as points, followed by the O(k^2) calipers, for cells too large for ``brute``.  Neither uses row extents (the route of the
kernels).  Imports nothing from the package."""
import math
from fractions import Fraction

import numpy as np

PLANES = ["perimeter", "hull_n", "hull_area2", "feret2", "ay", "ax", "by", "bx", "minw_num", "minw_den2"]
BRUTE_CORNERS = 60        # hull(): cells with more corners go through andrew


def _crop(frame, l):
    """-> (boolean mask of cell l cut to its bounding box, (row, column) of the cut's origin), or (None, None)"""
    m = np.asarray(frame) == l
    if not m.any():
        return None, None
    ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
    return m[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1], (int(ys[0]), int(xs[0]))


def corners(mask, origin=(0, 0)):
    """the corners of the pixels of a boolean mask: list of (y, x) Python integers in (y, x) order"""
    h, w = mask.shape
    c = np.zeros((h + 1, w + 1), bool)
    c[:-1, :-1] |= mask
    c[1:, :-1] |= mask
    c[:-1, 1:] |= mask
    c[1:, 1:] |= mask
    return [(int(y) + origin[0], int(x) + origin[1]) for y, x in np.argwhere(c)]


def perimeter(mask):
    """unit edges between a pixel of the mask and a pixel outside it (or the outside of the array): four shifted comparisons"""
    p = np.pad(mask, 1)
    inner = p[1:-1, 1:-1]
    return int((inner & ~p[:-2, 1:-1]).sum() + (inner & ~p[2:, 1:-1]).sum() + (inner & ~p[1:-1, :-2]).sum() +
               (inner & ~p[1:-1, 2:]).sum())


def _farthest(points):
    """points in (y, x) order -> (d2, a, b): the first pair in (a, b) order among those with the largest distance"""
    best = (-1, None, None)
    for i, a in enumerate(points):
        for b in points[i + 1:]:
            d2 = (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
            if d2 > best[0]:
                best = (d2, a, b)
    return best


def _width_key(ey, ex, far):
    g = math.gcd(abs(ey), abs(ex))
    assert far % g == 0
    num, den2 = far // g, (ey * ey + ex * ex) // (g * g)
    return (Fraction(num * num, den2), den2), num, den2


def brute(frame, l):
    """the ten integers of cell l of one frame straight from the definitions"""
    mask, origin = _crop(frame, l)
    if mask is None:
        return [0] * 10
    P = corners(mask, origin)
    A = np.array(P, np.int64)
    d2, a, b = _farthest(P)
    width, nxt = None, {}
    for i, p in enumerate(P):
        E = A - A[i]
        cr = E[:, :1] * E[None, :, 1] - E[:, 1:] * E[None, :, 0]         # cr[q, c]: corner c against the line p -> q
        lo, hi = cr.min(axis=1), cr.max(axis=1)
        for j in np.nonzero((lo >= 0) | (hi <= 0))[0]:                   # every corner on one side of the line
            if j == i:
                continue
            ey, ex = int(E[j, 0]), int(E[j, 1])
            cand = _width_key(ey, ex, int(max(-lo[j], hi[j])))
            if width is None or cand[0] < width[0]:
                width = cand
            if lo[j] >= 0:                                               # a directed side of the hull; its two far ends
                along = E[cr[j] == 0] @ E[j]
                if along.min() == 0 and along.max() == int(E[j] @ E[j]):
                    nxt[p] = P[j]
    poly, v = [P[0]], nxt[P[0]]
    while v != P[0]:
        poly.append(v)
        v = nxt[v]
    assert len(poly) == len(nxt)
    area2 = abs(sum(p[0] * q[1] - p[1] * q[0] for p, q in zip(poly, poly[1:] + poly[:1])))
    return [perimeter(mask), len(poly), area2, d2, a[0], a[1], b[0], b[1], width[1], width[2]]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(points):
    """Andrew's monotone chain over points sorted as tuples; strict (collinear points dropped); one closed loop"""
    pts = sorted(set(points))
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def andrew(frame, l):
    """the ten integers of cell l through the sorted-points monotone chain and O(k^2) calipers over the hull's vertices"""
    mask, origin = _crop(frame, l)
    if mask is None:
        return [0] * 10
    poly = convex_hull(corners(mask, origin))
    area2 = abs(sum(p[0] * q[1] - p[1] * q[0] for p, q in zip(poly, poly[1:] + poly[:1])))
    d2, a, b = _farthest(sorted(poly))
    width = None
    for p, q in zip(poly, poly[1:] + poly[:1]):
        ey, ex = q[0] - p[0], q[1] - p[1]
        far = max(abs(ey * (v[1] - p[1]) - ex * (v[0] - p[0])) for v in poly)
        cand = _width_key(ey, ex, far)
        if width is None or cand[0] < width[0]:
            width = cand
    return [perimeter(mask), len(poly), area2, d2, a[0], a[1], b[0], b[1], width[1], width[2]]


def hull(labels, off, brute_corners=BRUTE_CORNERS):
    """labels [T, H, W]; off int64 [T + 1] -> int64 [10, n], the output of mseg_cell_hull: ids 1 .. K_t of frame t, ids beyond
    the table and negative ids are not a cell; cells of up to ``brute_corners`` corners by ``brute``, larger ones by ``andrew``"""
    labels = np.asarray(labels)
    out = np.zeros((10, int(off[-1])), np.int64)
    for t in range(labels.shape[0]):
        for l in range(1, int(off[t + 1] - off[t]) + 1):
            mask, _ = _crop(labels[t], l)
            if mask is None:
                continue
            few = len(corners(mask)) <= brute_corners
            out[:, int(off[t]) + l - 1] = (brute if few else andrew)(labels[t], l)
    return out
