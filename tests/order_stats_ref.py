"""Plain numpy restatement of the per-cell order statistics (include/mseg_hip.h: mseg_cell_order_stats) and of the
percentile rule of the cell table, written from the header text: np.sort of the masked pixels, then plain indexing.
Imports nothing from the package."""
import math

import numpy as np


def order_stats(labels, off, img, bbox, ranks, bg_ranks):
    """labels [T, H, W]; off int64 [T + 1]; img [T, C, H, W] uint8 / uint16; bbox int [n, 4] (r0, c0, r1, c1, half-open,
    zeros = absent); ranks int [R, n]; bg_ranks int [R, T] -> (values uint32 [R, C, n], bg_values uint32 [R, T, C], status)"""
    T, H, W = labels.shape
    C = img.shape[1]
    n = int(off[-1])
    R = len(bg_ranks)
    values, bg_values, status = np.zeros((R, C, n), np.uint32), np.zeros((R, T, C), np.uint32), 0
    for t in range(T):
        for l in range(1, int(off[t + 1] - off[t]) + 1):
            s = int(off[t]) + l - 1
            r0, c0, r1, c1 = (int(v) for v in bbox[s])
            if (r0, c0, r1, c1) == (0, 0, 0, 0):
                continue                                       # absent: zeros, the ranks are not read
            inside = np.zeros((H, W), bool)
            inside[max(r0, 0):max(min(r1, H), 0), max(c0, 0):max(min(c1, W), 0)] = True
            m = (labels[t] == l) & inside
            for c in range(C):
                v = np.sort(img[t, c][m])
                for j in range(R):
                    r = int(ranks[j][s])
                    if 0 <= r < len(v):
                        values[j, c, s] = v[r]
                    else:
                        status = 1
        b = labels[t] == 0                                     # ids beyond the table and negative ids are not background
        if not b.any():
            continue
        for c in range(C):
            v = np.sort(img[t, c][b])
            for j in range(R):
                r = int(bg_ranks[j][t])
                if 0 <= r < len(v):
                    bg_values[j, t, c] = v[r]
                else:
                    status = 1
    return values, bg_values, status


def percentile_ranks(n, P):
    """the two 0-based ranks numpy's linear rule reads for percentile P of n >= 1 sorted values, and the weight of the upper"""
    h = (n - 1) * (P / 100)
    k = math.floor(h)
    return int(k), int(min(k + 1, n - 1)), h - k


def percentile_value(lo, hi, g):
    d = float(hi) - float(lo)
    return float(lo) + d * g if g < 0.5 else float(hi) - d * (1 - g)


def percentile(sorted_values, P):
    """percentile P of an ascending integer array through the two order statistics"""
    k, k1, g = percentile_ranks(len(sorted_values), P)
    return percentile_value(int(sorted_values[k]), int(sorted_values[k1]), g)


def percentile_columns(labels, img, channels, percentiles):
    """{column: [one float per cell in (frame, label) order]} for p{P}_ch{c} and bg_p{P}_ch{c}; NaN without background"""
    out = {f"{b}p{P}_ch{c}": [] for b in ("", "bg_") for c in channels for P in percentiles}
    for t in range(labels.shape[0]):
        for l in range(1, max(int(labels[t].max(initial=0)), 0) + 1):
            m = labels[t] == l
            if not m.any():
                continue
            for c in channels:
                v, b = np.sort(img[t, c][m]), np.sort(img[t, c][labels[t] == 0])
                for P in percentiles:
                    out[f"p{P}_ch{c}"].append(percentile(v, P))
                    out[f"bg_p{P}_ch{c}"].append(percentile(b, P) if len(b) else float("nan"))
    return out
