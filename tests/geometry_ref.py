"""Deterministic worst-case frames for the post-processing, relabelling and label-creation kernels (numpy only, no RNG).

Every generator returns its inputs plus a dict of structural FACTS — counts of components, bounding boxes, seed sizes, ties —
that are computed on the host from the oracle's smoothing (oracle.postproc_ref.gaussian05) and scipy.ndimage.label, never
from the device.  tests/test_geometry_host.py asserts the facts a pattern was built for; the GPU module
(tests/test_gpu_postproc_geometry.py) sends the same frames through the HIP entries and compares bit for bit.

  distance patterns   (cell, border, facts)   float32 (H, W) maps; facts at a (th_cell, th_seed) pair, AFTER smoothing
  boundary patterns   (probs, facts)          float32 (H, W, 3); p1 = 0.9 on seeds, so mask and seeds are exact
  label images        (image, facts)          integer instance masks for the relabelling / label-creation entries
"""
import numpy as np
from scipy import ndimage as ndi

from oracle import postproc_ref as R

THS = ((0.10, 0.45), (0.02, 0.30))          # (th_cell, th_seed): the defaults and a low pair that merges cells
SCAN_TILE = 2048                            # csrc/postproc.hip
S8 = np.ones((3, 3), bool)


# ---- facts ---------------------------------------------------------------------------------------------------------------
def _kept(seed_bin, distance_rule):
    """8-connected seed components that survive the small-seed rule -> (labels of the kept ones 1..K in raster order, K)"""
    lab, k = ndi.label(seed_bin, structure=S8)
    if k == 0:
        return lab, 0, np.zeros(0, np.int64)
    area = np.bincount(lab.ravel(), minlength=k + 1)[1:]
    min_area = max(0.10 * float(area.mean()), 4.0) if distance_rule else 4.0
    keep = area > min_area
    remap = np.zeros(k + 1, np.int64)
    remap[1:][keep] = np.arange(1, int(keep.sum()) + 1)
    return remap[lab], int(keep.sum()), area


def _mask_facts(mask, kept):
    H, W = mask.shape
    mlab, nm = ndi.label(mask)                                         # 4-connected
    f = {"n_mask_comp": int(nm), "mask_area": int(mask.sum())}
    boxes = ndi.find_objects(mlab)
    f["box_is_frame"] = [b[0].start == 0 and b[0].stop == H and b[1].start == 0 and b[1].stop == W for b in boxes]
    # instances (kept seeds inside the mask) per mask component: >= 2 means that labels meet inside it
    f["max_inst_per_comp"] = None                                      # (not counted for frames of many components)
    if nm <= 64:
        per = [len(np.unique(kept[(mlab == c) & (kept > 0)])) for c in range(1, nm + 1)]
        f["max_inst_per_comp"] = max(per, default=0)
    return f, mlab


def distance_facts(cell, border, th_cell=0.10, th_seed=0.45):
    """what the reference chain sees at these thresholds: mask / seed components after gaussian(0.5), kept seeds, ties"""
    cs = R.gaussian05(cell)
    b = np.clip(border, 0, 1).astype(np.float32)
    t = np.tan((b * b).astype(np.float64)).astype(np.float32)
    t[t < np.float32(0.05)] = 0
    t = np.clip(t, 0, 1)
    mask = cs > np.float32(th_cell)
    seed_bin = (cs - t) > np.float32(th_seed)
    kept, n_kept, area = _kept(seed_bin, True)
    f, mlab = _mask_facts(mask, kept * mask)
    f.update(n_seed_comp=len(area), n_kept=n_kept, seed_areas=area.tolist() if len(area) <= 64 else None)
    mk = (kept > 0) & mask                                            # initial markers of the flood
    f["n_inst"] = n_kept
    # ties between initial markers of one mask component (the only ties the per-component flood has to care about)
    ties = 0
    if f["n_mask_comp"] <= 64:
        for c in range(1, f["n_mask_comp"] + 1):
            v = cs[mk & (mlab == c)]
            ties += len(v) - len(np.unique(v))
    else:
        ties = -1
    f["marker_ties"] = ties
    f["seed_max"] = [cs[kept == k].max() for k in range(1, n_kept + 1)] if n_kept <= 256 else None
    idx = np.flatnonzero(kept.ravel() > 0)
    f["kept_first_px"], f["kept_last_px"] = (int(idx[0]), int(idx[-1])) if len(idx) else (-1, -1)
    return f


def boundary_facts(probs):
    p0, p1, p2 = probs[..., 0], probs[..., 1], probs[..., 2]
    mask = (p1 > p0) & (p1 >= p2)                                      # np.argmax == 1 (first maximum wins)
    seed_bin = p1 * (np.float32(1) - p2) > np.float32(0.5)
    kept, n_kept, area = _kept(seed_bin, False)
    f, _ = _mask_facts(mask, kept * mask)
    f.update(n_seed_comp=len(area), n_kept=n_kept, n_inst=n_kept)
    idx = np.flatnonzero(kept.ravel() > 0)
    f["kept_first_px"], f["kept_last_px"] = (int(idx[0]), int(idx[-1])) if len(idx) else (-1, -1)
    return f


def boundary_probs(mask, seeds=None):
    """(H, W, 3) probabilities whose argmax == 1 exactly on `mask` and whose seed rule p1 * (1 - p2) > 0.5 holds exactly on
    `seeds` (default: the mask).  On seeds p = (0.05, 0.9, 0.05), on the rest of the mask (0.3, 0.45, 0.25), off it
    (0.9, 0.05, 0.05)."""
    mask = np.asarray(mask, bool)
    seeds = mask if seeds is None else (np.asarray(seeds, bool) & mask)
    p = np.empty(mask.shape + (3,), np.float32)
    p[...] = (0.9, 0.05, 0.05)
    p[mask] = (0.3, 0.45, 0.25)
    p[seeds] = (0.05, 0.9, 0.05)
    return p


def ramp(H, W):
    """strictly monotone in the raster index, with an irrational step along x so that mirror-symmetric pixels differ"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (0.75 + 0.25 * (yy * W + xx * 0.6180339887) / float(H * W)).astype(np.float32)


# ---- winding lines: serpentine, spiral, comb --------------------------------------------------------------------------------
def _serpentine_path(H, W, pitch):
    if (H - 1) % pitch:
        assert (W - 1) % pitch == 0, "pitch must divide H - 1 or W - 1 (the line has to reach the far edge)"
        return [(x, y) for y, x in _serpentine_path(W, H, pitch)]
    path = []
    for k, y in enumerate(range(0, H, pitch)):
        xs = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + pitch < H:
            path += [(yy, path[-1][1]) for yy in range(y + 1, y + pitch)]
    return path


def _spiral_path(H, W, pitch):
    line = np.zeros((H, W), bool)
    y = x = d = 0
    line[0, 0] = True
    path = [(0, 0)]
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while True:
        for _ in range(2):
            dy, dx = dirs[d]
            ok = 0 <= y + dy < H and 0 <= x + dx < W
            for k in range(1, pitch + 1):
                yy, xx = y + dy * k, x + dx * k
                if ok and 0 <= yy < H and 0 <= xx < W and line[yy, xx]:
                    ok = False
            if ok:
                break
            d = (d + 1) % 4
        if not ok:
            return path
        y, x = y + dy, x + dx
        line[y, x] = True
        path.append((y, x))


def winding(kind, H, W, pitch):
    """-> (1 px wide 4-connected line (bool) that touches all four frame edges, [pixels of end A], [pixels of end B]);
    the ends are the first / last 7 pixels of the line (serpentine, spiral) or the tips of the outer teeth (comb)"""
    line = np.zeros((H, W), bool)
    if kind == "comb":
        assert (W - 1) % pitch == 0
        line[0, :] = True
        line[:, ::pitch] = True
        a = [(y, 0) for y in range(H - 7, H)]
        b = [(y, W - 1) for y in range(H - 7, H)]
        return line, a, b
    path = _serpentine_path(H, W, pitch) if kind == "serpentine" else _spiral_path(H, W, pitch)
    for y, x in path:
        line[y, x] = True
    return line, path[:7], path[-7:]


def winding_distance(kind, H, W, pitch=8, ramped=False):
    """the line at 0.5 (inside the mask at either th_cell, a seed only at the low pair) with 1.0 on its two ends: two seeds
    at the default pair, whose labels meet somewhere along ONE mask component that spans the frame"""
    line, a, b = winding(kind, H, W, pitch)
    cell = np.where(line, np.float32(0.5), np.float32(0))
    for y, x in a + b:
        cell[y, x] = 1.0
    if ramped:
        cell = cell * ramp(H, W)
    cell = cell.astype(np.float32)
    border = np.zeros_like(cell)
    return cell, border, distance_facts(cell, border)


def winding_boundary(kind, H, W, pitch=2):
    line, a, b = winding(kind, H, W, pitch)
    seeds = np.zeros_like(line)
    for y, x in a + b:
        seeds[y, x] = True
    probs = boundary_probs(line, seeds)
    return probs, boundary_facts(probs)


# ---- distance patterns ------------------------------------------------------------------------------------------------------
DEGENERATE_SHAPES = [(1, 1), (1, 2), (2, 1), (1, 64), (65, 1), (2, 2), (3, 5), (5, 3), (3, 63), (3, 64), (3, 65)]
DEGENERATE_KINDS = ["ones", "zeros", "ramp"]


def degenerate(H, W, kind):
    """frames smaller than the gaussian's reach / narrower than a wavefront: all ones, all zeros, a ramp 0.2 .. 1.0"""
    if kind == "ones":
        cell = np.ones((H, W), np.float32)
    elif kind == "zeros":
        cell = np.zeros((H, W), np.float32)
    else:
        cell = (0.2 + 0.8 * (np.arange(H * W, dtype=np.float64).reshape(H, W) + 1) / (H * W)).astype(np.float32)
    border = np.zeros_like(cell)
    return cell, border, distance_facts(cell, border)


def degenerate_boundary(H, W, kind):
    if kind == "ones":
        mask = np.ones((H, W), bool)
    elif kind == "zeros":
        mask = np.zeros((H, W), bool)
    else:                                                   # "ramp": the second half of the raster
        mask = np.arange(H * W).reshape(H, W) >= (H * W) // 2
    probs = boundary_probs(mask)
    return probs, boundary_facts(probs)


SCAN_SHAPES = [(23, 89), (32, 64), (3, 683)]                # 2047, 2048 and 2049 pixels: around one tile of the prefix sum


def _corner_blocks(H, W):
    m = np.zeros((H, W), bool)
    m[:3, :3] = True
    m[-3:, -3:] = True
    return m


def scan_edges(H, W):
    """a 3 x 3 seed in the first and in the last corner: kept seeds hold pixel 0 and pixel n - 1"""
    cell = _corner_blocks(H, W).astype(np.float32)
    border = np.zeros_like(cell)
    return cell, border, distance_facts(cell, border)


def scan_edges_boundary(H, W):
    probs = boundary_probs(_corner_blocks(H, W))
    return probs, boundary_facts(probs)


def lattice(H, W, pitch, r, ramped=False):
    """identical cones of radius r on a square lattice of this pitch (2 r > pitch: the cells overlap into ONE mask component);
    integer centre offsets, so all cells hold bit-identical values: every marker ties.  ramped: each cone is tilted by the
    same small plane, so the pixels of ONE cell differ from each other and the ties are those between cells alone."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    cell = np.zeros((H, W), np.float32)
    for cy in range(pitch // 2, H, pitch):
        for cx in range(pitch // 2, W, pitch):
            d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
            cone = np.clip(1 - d / np.float32(r), 0, 1).astype(np.float32)
            if ramped:
                cone = cone * (np.float32(0.9) + np.float32(0.004) * (yy - cy) + np.float32(0.0025) * (xx - cx))
            cell = np.maximum(cell, cone.astype(np.float32))
    border = np.zeros_like(cell)
    return cell, border, distance_facts(cell, border)


MIRROR_AXES = ["vertical", "horizontal", "point"]


def mirror_pair(axis, H=40, W=48, ramped=False):
    """a tilted elliptical cone and its mirror image on a pedestal of 0.2 (one mask component), the two seeds a few pixels
    apart.  vertical: columns flipped; horizontal: rows flipped; point: both (the pair sits diagonally).  The smoothing
    adds its symmetric taps pairwise, so it commutes with these flips bit for bit (it does not with a transposition: its
    two passes round to float32 in between) and the two seeds hold the same values.  ramped: the cone is tilted before it
    is mirrored, so no two pixels of ONE seed are equal and every tie is one between the two labels."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    cy, cx = {"vertical": (19.0, 17.0), "horizontal": (12.5, 24.0), "point": (13.0, 17.5)}[axis]
    c, s = np.float32(np.cos(0.5)), np.float32(np.sin(0.5))
    u, v = (yy - cy) * c + (xx - cx) * s, -(yy - cy) * s + (xx - cx) * c
    blob = np.clip(1 - np.sqrt((u / 9) ** 2 + (v / 6) ** 2), 0, 1).astype(np.float32)
    if ramped:
        blob = (blob * ramp(H, W)).astype(np.float32)
    mirrored = {"vertical": blob[:, ::-1], "horizontal": blob[::-1], "point": blob[::-1, ::-1]}[axis]
    cell = np.maximum(blob, mirrored)
    ped = np.zeros((H, W), np.float32)
    ped[4:H - 4, 4:W - 4] = 0.2
    cell = np.maximum(cell, ped)
    border = np.zeros_like(cell)
    f = distance_facts(cell, border)
    seeds = ndi.label(R.gaussian05(cell) > np.float32(0.45), structure=S8)[0]
    if seeds.max() == 2:
        d = ndi.distance_transform_cdt(seeds != 1, metric="chessboard")
        f["seed_gap"] = int(d[seeds == 2].min()) - 1        # background pixels between the two seeds
    return cell, border, f


def row_wrap(H=12, W=40):
    """a frame narrower than a wavefront with a Z-shaped seed: its second row starts at x = 0 right behind the end of its
    first row, which starts at x = 20 — in raster order ONE run of equal roots across the row end.  The seed's column-major
    key is that of the pixel at x = 0, and a second seed at x = 5 lies between the two candidates."""
    cell = np.zeros((H, W), np.float32)
    cell[2:4, 20:] = 1.0
    cell[4:6, :] = 1.0
    cell[8:11, 5:8] = 1.0
    border = np.zeros_like(cell)
    return cell, border, distance_facts(cell, border)


def row_wrap_boundary(H=12, W=40):
    m = np.zeros((H, W), bool)
    m[2, 20:] = True
    m[3, :] = True
    m[8:11, 5:8] = True
    seeds = m.copy()
    seeds[3, :12] = False                       # the flood has to walk back along the lower row
    probs = boundary_probs(m, seeds)
    return probs, boundary_facts(probs)


def plateau(H=46, W=56):
    """a pedestal of 0.25 over the whole frame with ONE raised square: one seed, and every other key of the flood equal"""
    cell = np.full((H, W), 0.25, np.float32)
    cell[20:26, 25:31] = 0.8
    border = np.zeros_like(cell)
    return cell, border, distance_facts(cell, border)


def terraces(H=46, W=56):
    """two levels: the pedestal and 2 x 3 identical raised squares — six tied seeds whose floods meet on a constant floor"""
    cell = np.full((H, W), 0.25, np.float32)
    for y in (9, 31):
        for x in (7, 25, 43):
            cell[y:y + 6, x:x + 6] = 0.8
    border = np.zeros_like(cell)
    return cell, border, distance_facts(cell, border)


def disk_one_seed(H=200, W=200, r=90, ramped=False):
    """a flat disk with one small seed in the middle: the flood's queue grows as long as the disk's perimeter"""
    yy, xx = np.mgrid[0:H, 0:W]
    disk = (yy - H // 2) ** 2 + (xx - W // 2) ** 2 <= r * r
    cell = np.where(disk, np.float32(0.25), np.float32(0))
    cell[H // 2 - 1:H // 2 + 2, W // 2 - 1:W // 2 + 2] = 0.8
    if ramped:
        cell = cell * ramp(H, W)
    cell = cell.astype(np.float32)
    border = np.zeros_like(cell)
    return cell, border, distance_facts(cell, border)


MANY_TH = (0.30, 0.45)      # at th_cell 0.30 the 1 px gaps (smoothed to 0.21) stay out of the mask: squares stay apart


def many_squares(H=1028, W=1024):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy % 4 < 3) & (xx % 4 < 3)


def many_instances(H=1028, W=1024):
    """3 x 3 squares on a pitch of 4: 257 * 256 = 65 792 instances, more than uint16 holds; 514 tiles of the prefix sum"""
    cell = many_squares(H, W).astype(np.float32)
    border = np.zeros_like(cell)
    return cell, border, {"n_squares": (H // 4) * (W // 4), "scan_tiles": -(-H * W // SCAN_TILE)}


def many_instances_boundary(H=1028, W=1024):
    return boundary_probs(many_squares(H, W)), {"n_squares": (H // 4) * (W // 4), "scan_tiles": -(-H * W // SCAN_TILE)}


SEPARATOR_CASES = [(1, False), (2, False), (7, False), (2, True), (7, True)]      # (H, touch only diagonally)


def separator(H, diagonal=False, N=3, W=66):
    """N frames whose facing rows — the last of frame k, the first of frame k + 1 — are foreground over the full width (or,
    diagonal: over complementary halves, so that they touch in one corner only).  Frames of ONE row cannot hold two such
    rows, and with two rows the frames alone and the stack give the same single instance: for H <= 2 the middle frames are
    0.4 instead — inside the mask, a seed only if a neighbour's row leaked into their smoothing.
    -> (cell (N, H, W), border, facts); facts['merged_differs']: the oracle on the frames stacked WITHOUT a separator gives
    other labels than frame by frame."""
    cell = np.zeros((N, H, W), np.float32)
    lo, hi = (slice(0, W // 2), slice(W // 2, W)) if diagonal else (slice(None), slice(None))
    if H <= 2 and not diagonal:
        cell[0, H - 1, :] = 1.0
        cell[N - 1, 0, :] = 1.0
        cell[1:N - 1] = 0.4
    else:
        for k in range(N - 1):
            cell[k, H - 1, lo] = 1.0
            cell[k + 1, 0, hi] = 1.0
    border = np.zeros_like(cell)
    per = np.stack([R.distance_postprocessing(border[k][..., None], cell[k][..., None], 0.45, 0.10) for k in range(N)])
    tall = R.distance_postprocessing(border.reshape(N * H, W, 1), cell.reshape(N * H, W, 1), 0.45, 0.10)
    f = {"merged_differs": not np.array_equal(per.reshape(N * H, W), tall), "n_inst": [int(p.max()) for p in per]}
    return cell, border, f


def checkerboard(H, W):
    """every second pixel: ceil(n / 2) one-pixel mask components (4-connected), ONE seed (8-connected) — label 1 on all of them"""
    yy, xx = np.mgrid[0:H, 0:W]
    probs = boundary_probs((yy + xx) % 2 == 0)
    return probs, boundary_facts(probs)


def fixture_distance_cases():
    """the cases of tests/golden/postproc_geometry.npz (tools/gen_golden_postproc.py runs the real reference on them)"""
    c = {"lattice_61x67": lattice(61, 67, 12, 8), "lattice_120x130": lattice(120, 130, 10, 7),
         "serpentine_65x70": winding_distance("serpentine", 65, 70, 8), "plateau": plateau()}
    for axis in MIRROR_AXES:
        c[f"mirror_{axis}"] = mirror_pair(axis)
    return c


def fixture_boundary_cases():
    return {"checkerboard_64x65": checkerboard(64, 65), "serpentine_129x131": winding_boundary("serpentine", 129, 131, 2)}


# ---- label images for the relabelling entries -------------------------------------------------------------------------------
def label_shapes(H=64, W=65):
    """name -> (uint16 label image, facts with n_labels = components of EQUAL value, 8-connected)"""
    out = {}
    m = np.zeros((H, W), np.uint16)
    m[5:15, 5:20] = 5
    m[30:40, 30:50] = 5
    out["one_id_two_pieces"] = (m, {"n_labels": 2})
    m = np.zeros((H, W), np.uint16)
    m[10:30, 10:25] = 3
    m[10:30, 25:40] = 4
    out["two_ids_adjacent"] = (m, {"n_labels": 2})
    m = np.zeros((H, W), np.uint16)
    m[10:20, 10:20] = 7
    m[20:30, 20:30] = 7
    out["same_id_diagonal"] = (m, {"n_labels": 1})
    yy, xx = np.mgrid[0:H, 0:W]
    out["checkerboard_two_ids"] = ((1 + (yy + xx) % 2).astype(np.uint16), {"n_labels": 2})
    line, _, _ = winding("serpentine", H, W, 2)
    m = np.where(line, 9, 0).astype(np.uint16)
    out["serpentine"] = (m, {"n_labels": 1})
    return out


def border_shapes(H=64, W=65):
    """a serpentine that touches the frame (visible inside any field of interest) on every second row pair, with small
    instances in the free rows: some only inside the 3 px border, some only inside the 10 px border, some in the middle"""
    line, _, _ = winding("serpentine", H, W, 8)
    m = np.where(line, 9, 0).astype(np.uint16)
    m[2:5, 0:2] = 11                 # inside the 3 px border only
    m[2:5, 5:9] = 12                 # inside the 10 px border, visible at width 3
    m[26:30, 30:40] = 13             # in the middle
    m[H - 3:H - 1, 20:24] = 14       # bottom border
    m[10:13, W - 2:W] = 11           # a second piece of 11, also in the border
    return m


def stack_shapes(T=3, H=64, W=65):
    """frames whose facing rows carry the same value (a relabelling of the stack as one tall image would merge them)"""
    base = label_shapes(H, W)
    names = ["serpentine", "checkerboard_two_ids", "one_id_two_pieces"]
    frames = np.stack([base[names[t % 3]][0] for t in range(T)]).astype(np.int32)
    frames[:, 0, :] = 21
    frames[:, H - 1, :] = 21
    return frames


# ---- instance masks for label creation (csrc/labels.hip) -------------------------------------------------------------------
def _carve_gap(lab, width):
    """background between the two cells: pixels of cell 2 next to cell 1 (width 1), and of cell 1 next to that (width 2)"""
    lab = lab.copy()
    g = (lab == 2) & ndi.binary_dilation(lab == 1, structure=S8)
    lab[g] = 0
    if width == 2:
        g2 = (lab == 1) & ndi.binary_dilation(g, structure=S8)
        lab[g2] = 0
    return lab


def two_cells_winding_gap(width, H=96, W=112):
    """two large cells that fill the frame up to a 4 px margin, separated by a sine-shaped gap `width` px wide (radius of
    curvature above the closing's disk, so that no cell's own closing cuts it): ONE long gap component"""
    yy, xx = np.mgrid[0:H, 0:W]
    edge = np.round(48 + 12 * np.sin(2 * np.pi * xx / 56.0))
    lab = np.where(yy < edge, 1, 2).astype(np.uint16)
    lab = _carve_gap(lab, width)
    lab[:4] = 0
    lab[-4:] = 0
    lab[:, :4] = 0
    lab[:, -4:] = 0
    return lab


def comb_cells(width, H=96, W=112):
    """two interlocked combs: cell 1 hangs its teeth from the top, cell 2 fills the space between them from below"""
    yy, xx = np.mgrid[0:H, 0:W]
    one = (yy < 20) | (((xx // 7) % 2 == 0) & (yy < 76))
    lab = np.where(one, 1, 2).astype(np.uint16)
    lab = _carve_gap(lab, width)
    lab[:4] = 0
    lab[-4:] = 0
    lab[:, :4] = 0
    lab[:, -4:] = 0
    return lab
