"""TEST INFRASTRUCTURE ONLY — structured worst-case stacks for the per-cell table (csrc/cells.hip: mseg_cell_measure and the
mseg_cell_links calls) and a Python model of how cm_kernel splits a stack.  Pure numpy, importable without a GPU.

A case is a function -> (labels [T, H, W], label_off int64 [T + 1], image [T, C, H, W] or None), all read-only.

What each family is for (the code path of the kernels that it puts on the line):
  M1 tiny_frames   4099 / 4101 wave steps over 4096 waves: a wave owns two steps and changes frame between them (the background
                   flush of `t != tcur`), at a chunk boundary (a) and in the middle of a frame (b); the waves past the last step idle
  M2 three_steps   8454 steps: three per wave, 2818 chunks per frame (no multiple of 3), a cell of more than 2^20 pixels
  M3 long_runs     one step per wave: runs of 8m + r pixels up to 527 at every offset against the wave step: every step d of
                   the segmented scan merges and stops, a run fills a whole wave, a run is cut at the wave's first and last lane
  M4 alternation   a new run every 1, 2, 3, 7, 8, 9 pixels at W = 63, 64, 65; one label over a whole frame whose rows are
                   64, 8, 4, 1 and 5000 pixels: a row end in every lane, every pixel its own row
  M5 id_edges      uint16 ids with the top bit set at the table's last entry and just past it; negative int32 ids
  M6 wide_frame    columns beyond 2^21: the closed form of sum_xx passes 64 bits
  L1 exact_fill    exactly 64 and 65 distinct pairs for a table of 64
  L2 one_over_many / many_over_one   about 2000 candidates tied at 6 pixels for one cell; one candidate for 2000 cells

model() restates the decomposition that the comment above cm_kernel describes (steps per wave, lanes of 8 pixels, link_in /
link_out, the scan with its `go` flag, the background flush on a frame change) on whole arrays; it is no copy of the kernel.
It returns the six outputs and counters of what the case made the decomposition do, and takes one named defect."""
import functools

import numpy as np

CHUNK, LANES, PPL, WAVES_PER_GROUP, MAX_GROUPS = 512, 64, 8, 4, 1024
SCAN_STEPS = (1, 2, 4, 8, 16, 32)
WRAP = 1 << 21                                     # from this column on m (m + 1) (2m + 1) passes 64 bits
DEFECTS = ("drop_scan_d16", "drop_scan_d32", "no_bg_flush_on_frame_change", "link_across_x0", "u16_top_bit_is_sign",
           "negative_is_background", "u64_sum_xx")
M3_M = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)
M3_R = (0, 1, 7)
M3_BEGIN, M3_END = (0, 5, 8), (3, 0, 8)            # pixels after a wave step's first pixel / before its last


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _image(seed, shape, dtype):
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def launch(T, H, W):
    """the launch of mseg_cell_measure: -> (chunks per frame, steps, waves, steps per wave)"""
    chunks = -(-(H * W) // CHUNK)
    steps = T * chunks
    groups = min(max(-(-steps // WAVES_PER_GROUP), 1), MAX_GROUPS)
    waves = groups * WAVES_PER_GROUP
    return chunks, steps, waves, -(-steps // waves)


# ---- measure cases ------------------------------------------------------------------------------------------------------------
def _tiny_frames(T, H, W, seed):
    """0 to 3 cells per frame.  Frame kinds: 0 all background; 1 no background at all (three cells side by side); 2 the only
    label lies beyond the table; 3 .. 5 up to three random rectangles, now and then one id beyond the table as well"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((T, H, W), np.uint16)
    K = np.zeros(T, np.int64)
    kind = rng.integers(0, 6, T)
    kind[:6] = np.arange(6)                        # every kind at least once
    for t in range(T):
        if kind[t] == 0:
            K[t] = rng.integers(0, 4)
        elif kind[t] == 1:
            K[t] = 3
            lab[t, :, :W // 3], lab[t, :, W // 3:2 * W // 3], lab[t, :, 2 * W // 3:] = 1, 2, 3
        elif kind[t] == 2:
            K[t] = rng.integers(0, 3)
            y, x = rng.integers(0, H - 3), rng.integers(0, W - 5)
            lab[t, y:y + rng.integers(1, 4), x:x + rng.integers(1, 6)] = K[t] + 1 + rng.integers(0, 3)
        else:
            K[t] = rng.integers(1, 4)
            for k in range(1, int(K[t]) + 1 + int(rng.random() < 0.2)):
                if rng.random() < 0.8:
                    y, x = rng.integers(0, H), rng.integers(0, W)
                    lab[t, y:y + rng.integers(1, H), x:x + rng.integers(1, W)] = k
    off = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    return lab, off, kind


def tiny_frames_a():
    """T = 4099, 16 x 32: one chunk per frame, 4099 steps, two per wave: every wave but the last used one changes frame once"""
    lab, off, _ = _tiny_frames(4099, 16, 32, 21)
    return _ro(lab, off, _image(22, (4099, 2, 16, 32), np.uint16))


def tiny_frames_b():
    """T = 1367, 11 x 131: three chunks per frame, 4101 steps, two per wave: a third of the used waves change frame"""
    lab, off, _ = _tiny_frames(1367, 11, 131, 23)
    return _ro(lab, off, _image(24, (1367, 1, 11, 131), np.uint8))


M2_SHAPE, M2_BLOCK, M2_X0 = (3, 1201, 1201), (7, 9), 870


def three_steps():
    """T = 3, 1201 x 1201, uint8 image.  Columns 870 .. 1193 of rows 0 .. 1196 hold 171 x 36 = 6156 touching blocks of 7 x 9
    pixels per frame, their ids permuted anew in every frame, 20 % of their pixels holes (0) and 2 % of the ids absent; all
    other pixels are one cell, id 6157, the same 1 054 573 > 2^20 pixels in all three frames.  (The frame cannot hold
    30 000 such blocks beside a cell of 2^20 pixels: 3 x 6156 blocks it is.)"""
    T, H, W = M2_SHAPE
    bh, bw = M2_BLOCK
    rng = np.random.default_rng(31)
    gy, gx = (H - 1) // bh, (W - M2_X0) // bw
    big = gy * gx + 1
    lab = np.full((T, H, W), big, np.uint16)
    for t in range(T):
        ids = rng.permutation(gy * gx) + 1
        ids[rng.random(ids.size) < 0.02] = 0
        block = np.repeat(np.repeat(ids.reshape(gy, gx), bh, axis=0), bw, axis=1)
        block[rng.random(block.shape) < 0.2] = 0
        lab[t, :gy * bh, M2_X0:M2_X0 + gx * bw] = block
    off = np.arange(T + 1, dtype=np.int64) * big
    return _ro(lab, off, _image(32, (T, 1, H, W), np.uint8))


def _long_runs():
    """T = 48 + 2, 6 x 1544 (19 chunks a frame, 950 steps on 952 waves).  Frame t < 48 holds one run per row, all of 8m + r
    pixels: rows 0 .. 2 begin 0, 5, 8 pixels after a wave step's first pixel, rows 3 .. 5 end 3, 0, 8 pixels before a wave
    step's last.  Frame 48: every row filled whole by an id of its own; frame 49: all six rows by id 1."""
    H, W = 6, 1544
    lengths = [8 * m + r for m in M3_M for r in M3_R]
    lab = np.zeros((len(lengths) + 2, H, W), np.int32)
    for t, n in enumerate(lengths):
        for row in range(H):
            if row < 3:
                p = -(-(row * W) // CHUNK) * CHUNK + M3_BEGIN[row]                      # first step boundary in the row
            else:
                p = ((row + 1) * W) // CHUNK * CHUNK - 1 - M3_END[row - 3] - (n - 1)      # last step boundary in the row
            assert row * W <= p and p + n <= (row + 1) * W
            lab[t].reshape(-1)[p:p + n] = row + 1
    lab[-2] = np.arange(1, H + 1)[:, None]
    lab[-1] = 1
    off = np.arange(lab.shape[0] + 1, dtype=np.int64) * H
    return lab, off


def long_runs_i32():
    lab, off = _long_runs()
    return _ro(lab, off, _image(41, (lab.shape[0], 1) + lab.shape[1:], np.uint8))


def long_runs_u16():
    lab, off = _long_runs()
    return _ro(lab.astype(np.uint16), off, _image(42, (lab.shape[0], 2) + lab.shape[1:], np.uint16))


M4_PERIODS = (1, 2, 3, 7, 8, 9)


def alternation(W):
    """T = 6, 40 x W: frame j changes label every M4_PERIODS[j] pixels of the flat order (so runs also meet the row end with
    the same label on both sides), through 1, 3, 5, 0 with a table of 3 entries: id 2 is absent, id 5 lies beyond the table"""
    H = 40
    p = np.arange(H * W)
    palette = np.array([1, 3, 5, 0], np.uint16)
    lab = np.stack([palette[(p // q) % 4].reshape(H, W) for q in M4_PERIODS])
    off = np.arange(len(M4_PERIODS) + 1, dtype=np.int64) * 3
    return _ro(lab, off, _image(50 + W, (len(M4_PERIODS), 2, H, W), np.uint8))


def fill(H, W):
    """T = 1: one label over the whole frame"""
    return _ro(np.ones((1, H, W), np.uint16), np.array([0, 1], np.int64), _image(60 + W, (1, 1, H, W), np.uint16))


def _id_frames(ids, dtype):
    """T = 2, 24 x 40: one rectangle per id, moved by (1, 2) in frame 1; a 1-pixel cell of every id in a corner region too"""
    lab = np.zeros((2, 24, 40), dtype)
    for t in range(2):
        for j, k in enumerate(ids):
            y, x = 2 + 5 * (j // 3) + t, 1 + 13 * (j % 3) + 2 * t
            lab[t, y:y + 3, x:x + 9 + j] = k
            lab[t, 22 + t, 3 * j] = k
    return lab


def id_edges_u16(K):
    """ids 1, 32767, 32768, 65535 in a table of K = 65535 (all cells) or 65534 (65535 lies beyond it) entries per frame"""
    lab = _id_frames((1, 32767, 32768, 65535), np.uint16)
    return _ro(lab, np.array([0, K, 2 * K], np.int64), _image(70, (2, 2, 24, 40), np.uint16))


def id_edges_i32():
    """cells 1, 2, 3 beside the ids -1, INT32_MIN and 2^31 - 1: these pixels are neither cell nor background"""
    lab = _id_frames((1, -1, 2, -2 ** 31, 3, 2 ** 31 - 1), np.int32)
    return _ro(lab, np.array([0, 3, 6], np.int64), _image(71, (2, 1, 24, 40), np.uint8))


M6_W = 2_200_000
# (id, row, first column, last column) of every run of wide_frame
M6_RUNS = ((1, 0, 2_097_100, 2_097_144), (3, 0, 2_097_145, 2_097_152), (1, 0, 2_097_153, 2_097_199),
           (2, 1, 0, 2_097_099), (1, 1, 2_097_100, 2_097_199))


def wide_frame():
    """T = 1, 2 x 2 200 000: the runs of M6_RUNS.  Cell 3 (8 pixels) ends on column 2^21, cell 1 spans it in both rows"""
    lab = np.zeros((1, 2, M6_W), np.uint16)
    for k, y, a, b in M6_RUNS:
        lab[0, y, a:b + 1] = k
    return _ro(lab, np.array([0, 3], np.int64), _image(80, (1, 1, 2, M6_W), np.uint8))


def wide_frame_sums():
    """shape [6][3] and bbox [3][4] of wide_frame from M6_RUNS in Python integers"""
    shape, bbox = [[0] * 3 for _ in range(6)], [[2, M6_W, 0, 0] for _ in range(3)]
    sq = lambda m: m * (m + 1) * (2 * m + 1) // 6
    for k, y, a, b in M6_RUNS:
        n, sx = b - a + 1, (a + b) * (b - a + 1) // 2
        for j, v in enumerate((n, y * n, sx, y * y * n, sq(b) - sq(a - 1), y * sx)):
            shape[j][k - 1] += v
        bb = bbox[k - 1]
        bbox[k - 1] = [min(bb[0], y), min(bb[1], a), max(bb[2], y + 1), max(bb[3], b + 1)]
    return shape, bbox


def old_sum_xx(a, b):
    """the closed form as it was before the fix: every product and difference modulo 2^64"""
    M = 1 << 64
    sb = (b * (b + 1) % M * (2 * b + 1) % M) // 6
    sa = 0 if a == 0 else ((a - 1) * a % M * (2 * a - 1) % M) // 6
    return (sb - sa) % M


MEASURE = {
    "M1_tiny_frames_a": tiny_frames_a, "M1_tiny_frames_b": tiny_frames_b, "M2_three_steps": three_steps,
    "M3_long_runs_i32": long_runs_i32, "M3_long_runs_u16": long_runs_u16,
    "M4_alternation_w63": functools.partial(alternation, 63), "M4_alternation_w64": functools.partial(alternation, 64),
    "M4_alternation_w65": functools.partial(alternation, 65),
    "M4_fill_w64": functools.partial(fill, 1000, 64), "M4_fill_w8": functools.partial(fill, 1000, 8),
    "M4_fill_w4": functools.partial(fill, 1000, 4), "M4_fill_w1": functools.partial(fill, 1000, 1),
    "M4_fill_h1": functools.partial(fill, 1, 5000),
    "M5_id_edges_u16_k65535": functools.partial(id_edges_u16, 65535),
    "M5_id_edges_u16_k65534": functools.partial(id_edges_u16, 65534), "M5_id_edges_i32": id_edges_i32,
    "M6_wide_frame": wide_frame,
}


# ---- links cases --------------------------------------------------------------------------------------------------------------
L1_CAP = 64


def exact_fill():
    """T = 3, 32 x 48: an 8 x 8 grid of 3 x 5 blocks, ids 1 .. 64, at the same places in all frames: 64 distinct pairs for
    frame 1.  In frame 2 block 1 is two columns wider and reaches block 2 of frame 1: 65 pairs"""
    lab = np.zeros((3, 32, 48), np.uint16)
    for j in range(64):
        y, x = 4 * (j // 8), 6 * (j % 8)
        lab[:, y:y + 3, x:x + 5] = j + 1
    lab[2, 0:3, 0:7] = 1
    return _ro(lab, np.array([0, 64, 128, 192], np.int64), None)


def _grid_frame(rng, H=96, W=128):
    """the frame of test_gpu_cells.random_small_labels: permuted ids on a grid of 2 x 3 pixels, 3 % of them missing"""
    gy, gx = H // 2, W // 3
    ids = rng.permutation(gy * gx) + 1
    ids[rng.random(ids.size) < 0.03] = 0
    f = np.zeros((H, W), np.uint16)
    f[:2 * gy, :3 * gx] = np.repeat(np.repeat(ids.reshape(gy, gx), 2, axis=0), 3, axis=1)
    return f, gy * gx


def one_over_many():
    """frame 1 is one cell over about 2000 cells of 6 pixels: the smallest id of them is the answer"""
    grid, k = _grid_frame(np.random.default_rng(91))
    return _ro(np.stack([grid, np.ones_like(grid)]), np.array([0, k, k + 1], np.int64), None)


def many_over_one():
    grid, k = _grid_frame(np.random.default_rng(92))
    return _ro(np.stack([np.ones_like(grid), grid]), np.array([0, 1, k + 1], np.int64), None)


def _labels_only(case):
    lab, off, _ = case()
    return lab, off, None


LINKS = {
    "L1_exact_fill": exact_fill, "L2_one_over_many": one_over_many, "L2_many_over_one": many_over_one,
    "L3_three_steps": functools.partial(_labels_only, three_steps),
    "L4_id_edges_u16_k65535": functools.partial(_labels_only, functools.partial(id_edges_u16, 65535)),
    "L4_id_edges_u16_k65534": functools.partial(_labels_only, functools.partial(id_edges_u16, 65534)),
    "L4_id_edges_i32": functools.partial(_labels_only, id_edges_i32),
}


# ---- the model ----------------------------------------------------------------------------------------------------------------
BIG = np.uint64(0xFFFFFFFF)


def _down(a, d, fill):
    """a[step, lane + d] (what lane reads from the lane d places on); past the wave's last lane: fill (never used: a lane
    that still goes on has a successor)"""
    out = np.full_like(a, fill)
    out[:, :LANES - d] = a[:, d:]
    return out


def _by_slot(slot, n):
    order = np.argsort(slot, kind="stable")
    s = slot[order]
    first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    return order, first, s[first]


def _sum_xx(a, b, wrap):
    """sum of x^2 over a .. b per run.  wrap: the 64-bit closed form everywhere (numpy's uint64 wraps as the device's does);
    else Python integers for the runs that reach column 2^21"""
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    one, two, six = np.uint64(1), np.uint64(2), np.uint64(6)
    am = np.where(a > 0, a - one, 0).astype(np.uint64)
    out = b * (b + one) * (two * b + one) // six - am * (am + one) * (two * am + one) // six
    if not wrap:
        sq = lambda m: m * (m + 1) * (2 * m + 1) // 6
        for i in np.flatnonzero(b >= np.uint64(WRAP)):
            out[i] = sq(int(b[i])) - sq(int(a[i]) - 1)
    return out


def model(labels, off, img=None, defect=None):
    """-> (the outputs of cells_ref.measure, info).  info: chunks, steps, waves, per, idle (waves without a step), crossing
    (waves that change frame), merged / stopped {d: count} (lanes that took a piece in / whose run ended at scan step d),
    full_wave_runs (runs of 512 pixels added at once), longest_run, runs = (y, x0, pixels) of everything added"""
    assert defect is None or defect in DEFECTS, defect
    T, H, W = labels.shape
    HW, C, n = H * W, 0 if img is None else img.shape[1], int(off[-1])
    chunks, steps, waves, per = launch(T, H, W)
    off = np.asarray(off, np.int64)
    raw = np.zeros((T, chunks * CHUNK), np.int64)
    raw[:, :HW] = (labels.view(np.int16) if defect == "u16_top_bit_is_sign" and labels.dtype == np.uint16
                   else labels).reshape(T, HW)
    inside = np.broadcast_to(np.arange(chunks * CHUNK) < HW, raw.shape)
    K = np.diff(off)
    e = np.where((raw > 0) & (raw <= K[:, None]), raw, 0).reshape(-1)            # the run label: 0 = no cell of the frame
    is_bg = (inside & ((raw <= 0) if defect == "negative_is_background" else (raw == 0))).reshape(-1)
    q = np.arange(chunks * CHUNK)
    Y, X = np.tile(q // W, T), np.tile(q % W, T)
    vals = np.zeros((C, T, chunks * CHUNK), np.uint64)
    for c in range(C):
        vals[c, :, :HW] = img[:, c].reshape(T, HW)
    vals = vals.reshape(C, T * chunks * CHUNK)
    N = steps * LANES                                                            # lanes in all

    # a lane's pieces: pixels of one label, cut where the label changes, at a row's first pixel, at the lane's first pixel
    k = np.arange(e.size) % PPL
    prev = np.r_[0, e[:-1]]
    begins = (e > 0) & ((k == 0) | (e != prev) | (X == 0))
    f = np.flatnonzero(begins)
    cell = e > 0
    if f.size == 0:
        f = np.zeros(0, np.int64)
    cnt = np.add.reduceat(cell.astype(np.int64), f) if f.size else np.zeros(0, np.int64)
    acc = {"s": [], "q": [], "mn": [], "mx": []}
    for c in range(C):
        v = vals[c]
        acc["s"].append(np.add.reduceat(np.where(cell, v, 0).astype(np.uint64), f) if f.size else np.zeros(0, np.uint64))
        acc["q"].append(np.add.reduceat(np.where(cell, v * v, 0).astype(np.uint64), f) if f.size else np.zeros(0, np.uint64))
        acc["mn"].append(np.minimum.reduceat(np.where(cell, v, BIG), f) if f.size else np.zeros(0, np.uint64))
        acc["mx"].append(np.maximum.reduceat(np.where(cell, v, 0).astype(np.uint64), f) if f.size else np.zeros(0, np.uint64))
    lane = f // PPL
    to_lane_end = (f % PPL) + cnt == PPL

    # link_in: the lane's first pixel continues the previous lane's last run; never into the wave's first lane, never
    # across a row's first pixel
    first_e, last_e = e[::PPL], e[PPL - 1::PPL]
    in_wave = np.arange(N) % LANES
    link_in = (in_wave > 0) & (first_e > 0) & (np.r_[0, last_e[:-1]] == first_e)
    if defect != "link_across_x0":
        link_in &= X[::PPL] != 0
    link_out = np.r_[link_in[1:], False] & (in_wave < LANES - 1)
    head = (f % PPL == 0) & link_in[lane]                                        # handed to the lane where the run begins
    whole = head & to_lane_end

    # R(lane) = the piece from the lane's first pixel to the run's end, by a suffix scan that stops where the run stops
    def lanes_of(values, fill):
        out = np.full(N, fill, np.uint64)
        out[lane[head]] = values[head]
        return out.reshape(steps, LANES)
    R = {"cnt": lanes_of(cnt.astype(np.uint64), 0)}
    for c in range(C):
        R[f"s{c}"], R[f"q{c}"] = lanes_of(acc["s"][c], 0), lanes_of(acc["q"][c], 0)
        R[f"mn{c}"], R[f"mx{c}"] = lanes_of(acc["mn"][c], BIG), lanes_of(acc["mx"][c], 0)
    go = np.zeros(N, bool)
    go[lane[whole]] = True
    go = (go & link_out).reshape(steps, LANES)
    merged, stopped = {}, {}
    dropped = {"drop_scan_d16": 16, "drop_scan_d32": 32}.get(defect)

    def merge(name, mine, other):
        if name.startswith("mn"):
            return np.minimum(mine, other)
        if name.startswith("mx"):
            return np.maximum(mine, other)
        return mine + other
    for d in SCAN_STEPS:
        if d == dropped:
            merged[d] = stopped[d] = 0
            continue
        god = _down(go, d, False)
        for name in R:
            fill = BIG if name.startswith("mn") else 0
            R[name] = np.where(go, merge(name, R[name], _down(R[name], d, fill)), R[name])
        merged[d], stopped[d] = int(go.sum()), int((go & ~god).sum())
        go = go & god
    Rn = {name: _down(a, 1, BIG if name.startswith("mn") else 0).reshape(-1) for name, a in R.items()}

    # what is added: every piece that is no head, the lane's last one together with the linked lanes after it
    keep = ~head
    takes = keep & to_lane_end & link_out[lane]
    run = {"cnt": np.where(takes, cnt.astype(np.uint64) + Rn["cnt"][lane], cnt.astype(np.uint64))[keep]}
    for c in range(C):
        for name, src in (("s", acc["s"]), ("q", acc["q"]), ("mn", acc["mn"]), ("mx", acc["mx"])):
            run[f"{name}{c}"] = np.where(takes, merge(name, src[c], Rn[f"{name}{c}"][lane]), src[c])[keep]
    fk = f[keep]
    ry, rx, rl = Y[fk].astype(np.uint64), X[fk].astype(np.uint64), run["cnt"]
    slot = off[fk // (chunks * CHUNK)] + e[fk] - 1
    out = {"shape": np.zeros((6, n), np.uint64), "bbox": np.zeros((n, 4), np.int32),
           "ch_sums": np.zeros((2, C, n), np.uint64), "ch_minmax": np.zeros((2, C, n), np.uint32),
           "bg_sums": np.zeros((3, T, C), np.uint64), "bg_minmax": np.zeros((2, T, C), np.uint32)}
    if fk.size:
        rb = rx + rl - np.uint64(1)
        sx = (rx + rb) * rl // np.uint64(2)
        order, first, s = _by_slot(slot, n)
        for j, v in enumerate((rl, ry * rl, sx, ry * ry * rl, _sum_xx(rx, rb, defect == "u64_sum_xx"), ry * sx)):
            out["shape"][j, s] = np.add.reduceat(v[order], first)
        out["bbox"][s, 0], out["bbox"][s, 1] = np.minimum.reduceat(ry[order], first), np.minimum.reduceat(rx[order], first)
        out["bbox"][s, 2] = np.maximum.reduceat(ry[order], first) + 1
        out["bbox"][s, 3] = np.maximum.reduceat((rx + rl)[order], first)
        for c in range(C):
            out["ch_sums"][0, c, s] = np.add.reduceat(run[f"s{c}"][order], first)
            out["ch_sums"][1, c, s] = np.add.reduceat(run[f"q{c}"][order], first)
            out["ch_minmax"][0, c, s] = np.minimum.reduceat(run[f"mn{c}"][order], first)
            out["ch_minmax"][1, c, s] = np.maximum.reduceat(run[f"mx{c}"][order], first)

    # background: a wave collects it over its steps and adds it when it moves on to another frame, and at its end
    it0 = np.arange(waves, dtype=np.int64) * per
    it1 = np.minimum(steps, it0 + per)
    crossing = np.zeros(waves, bool)
    if C:
        per_step = lambda a, op: op(a.reshape(steps, CHUNK), axis=1)
        b_cnt = per_step(is_bg.astype(np.uint64), np.sum)
        b_s = [per_step(np.where(is_bg, vals[c], 0).astype(np.uint64), np.sum) for c in range(C)]
        b_q = [per_step(np.where(is_bg, vals[c] * vals[c], 0).astype(np.uint64), np.sum) for c in range(C)]
        b_mn = [per_step(np.where(is_bg, vals[c], BIG), np.min) for c in range(C)]
        b_mx = [per_step(np.where(is_bg, vals[c], 0).astype(np.uint64), np.max) for c in range(C)]
        bg_mn, bg_mx = np.full((T, C), BIG, np.uint64), np.zeros((T, C), np.uint64)
        tcur = np.full(waves, -1, np.int64)
        w_cnt = np.zeros(waves, np.uint64)
        w_s, w_q = np.zeros((C, waves), np.uint64), np.zeros((C, waves), np.uint64)
        w_mn, w_mx = np.full((C, waves), BIG, np.uint64), np.zeros((C, waves), np.uint64)

        def add_to_frames(sel):
            sel = sel & (w_cnt > 0)
            t = tcur[sel]
            for c in range(C):
                np.add.at(out["bg_sums"][0, :, c], t, w_cnt[sel])
                np.add.at(out["bg_sums"][1, :, c], t, w_s[c, sel])
                np.add.at(out["bg_sums"][2, :, c], t, w_q[c, sel])
                np.minimum.at(bg_mn[:, c], t, w_mn[c, sel])
                np.maximum.at(bg_mx[:, c], t, w_mx[c, sel])
        for j in range(per):
            it = it0 + j
            act = it < it1
            t = np.where(act, it // chunks, -1)
            change = act & (t != tcur)
            moved = change & (tcur >= 0)
            crossing |= moved
            if defect != "no_bg_flush_on_frame_change":
                add_to_frames(moved)
                w_cnt[change] = 0
                w_s[:, change], w_q[:, change], w_mn[:, change], w_mx[:, change] = 0, 0, BIG, 0
            tcur[change] = t[change]
            i = it[act]
            w_cnt[act] += b_cnt[i]
            for c in range(C):
                w_s[c, act] += b_s[c][i]
                w_q[c, act] += b_q[c][i]
                w_mn[c, act] = np.minimum(w_mn[c, act], b_mn[c][i])
                w_mx[c, act] = np.maximum(w_mx[c, act], b_mx[c][i])
        add_to_frames(tcur >= 0)
        out["bg_minmax"][0], out["bg_minmax"][1] = np.where(out["bg_sums"][0] > 0, bg_mn, 0), bg_mx
    else:
        for j in range(1, per):
            it = it0 + j
            crossing |= (it < it1) & (it // chunks != it0 // chunks)
    info = dict(chunks=chunks, steps=steps, waves=waves, per=per, idle=int((it0 >= steps).sum()), crossing=int(crossing.sum()),
                merged=merged, stopped=stopped, full_wave_runs=int((rl == CHUNK).sum()),
                longest_run=int(rl.max(initial=0)), runs=(ry.astype(np.int64), rx.astype(np.int64), rl.astype(np.int64)))
    return out, info
