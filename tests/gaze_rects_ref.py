"""NumPy rasteriser of crfp_gaze_prep_f32's per-pixel definition (include/crfp_hip.h) and the explicit gaze trajectories the rectangle tests
share.  With R_e = entry e's rectangle intersected with the frame and G_e = the rectangle grown by `dilate` on all four sides intersected with the
frame (both empty for an entry that does not exist or has h < 1 or w < 1):
  fovea = p in R_0;  mk = bit1_0 and p in R_0;  outskirt = p in G_0 and not mk;
  past = OR over e = 1..3 of (p in G_e and not (bit1_e and p in R_e));  fg = p in box."""
import numpy as np

ROW_INTS = 24


def _rect(H, W, y, x, h, w, grow=0):
    m = np.zeros((H, W), dtype=bool)
    if h < 1 or w < 1:
        return m
    y0, y1, x0, x1 = (min(max(v, 0), lim) for v, lim in ((y - grow, H), (y + h + grow, H), (x - grow, W), (x + w + grow, W)))
    m[y0:y1, x0:x1] = True   # Python ints: no overflow whatever the row holds
    return m


def rasterise(row, H, W, dilate=10):
    """One row of the table -> dict of bool [H, W] planes mk, fovea, outskirt, past, fg."""
    row = [int(v) for v in row]
    assert len(row) == ROW_INTS
    R, G, counts = [], [], []
    for e in range(4):
        y, x, h, w, flags = row[4 + 5 * e:9 + 5 * e]
        on = bool(flags & 1)
        R.append(_rect(H, W, y, x, h, w) if on else np.zeros((H, W), dtype=bool))
        G.append(_rect(H, W, y, x, h, w, dilate) if on else np.zeros((H, W), dtype=bool))
        counts.append(bool(flags & 2))
    mk = R[0] if counts[0] else np.zeros((H, W), dtype=bool)
    past = np.zeros((H, W), dtype=bool)
    for e in (1, 2, 3):
        past |= G[e] & ~(R[e] if counts[e] else np.zeros((H, W), dtype=bool))
    y0, y1, x0, x1 = row[0:4]
    return {"mk": mk, "fovea": R[0], "outskirt": G[0] & ~mk, "past": past, "fg": _rect(H, W, y0, x0, y1 - y0, x1 - x0)}


# name -> H, W, fv_size, fv_start, regional-DCN box side (0 = off), [(cur_y, cur_x)]: a window in each of the four corners, a strictly interior
# one, two consecutive identical ones and more than four frames, so the three-frame history overflows
CASES = {
    "70x150": (70, 150, 16, 0, 0, [(0, 0), (0, 0), (0, 134), (27, 60), (54, 0), (54, 134), (30, 70), (5, 128)]),
    "23x45": (23, 45, 8, 2, 20, [(0, 0), (0, 0), (0, 37), (7, 18), (15, 0), (15, 37), (9, 20), (3, 33)]),
    "37x41": (37, 41, 8, 0, 12, [(0, 0), (0, 33), (0, 33), (14, 16), (29, 0), (29, 33), (10, 20), (25, 5)]),
    "64x256": (64, 256, 32, 1, 0, [(0, 0), (0, 224), (16, 100), (16, 100), (32, 0), (32, 224), (8, 180), (20, 36)]),
    "192x320": (192, 320, 32, 0, 96, [(0, 0), (0, 288), (80, 144), (160, 0), (160, 0), (160, 288), (40, 250), (100, 20)]),
}


def covers_the_edge_cases(H, W, fv, origins):
    """The conditions every list of CASES must hold."""
    corners = {(0, 0), (0, W - fv), (H - fv, 0), (H - fv, W - fv)}
    return (corners <= set(origins) and any(0 < y < H - fv and 0 < x < W - fv for y, x in origins) and
            any(a == b for a, b in zip(origins, origins[1:])) and len(origins) >= 5)
