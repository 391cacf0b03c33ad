"""Golden vectors under tests/golden/ that would be larger than a committed file may be are stored in parts.

A golden NAME is either one file NAME.npz or the parts NAME.part0.npz, NAME.part1.npz, ...  An array too large for one part is kept
as flat chunks KEY#0, KEY#1, ... plus its shape KEY#shape; load() puts it back together bit for bit.
"""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 640 << 10   # uncompressed bytes per part: a compressed part stays below 1 MiB whatever the data


def load(name, golden_dir=GOLDEN):
    """dict of the arrays of golden NAME (NAME.npz, or its parts)."""
    whole = os.path.join(golden_dir, name + ".npz")
    if os.path.exists(whole):
        return dict(np.load(whole))
    parts = sorted(glob.glob(os.path.join(golden_dir, glob.escape(name) + ".part*.npz")),
                   key=lambda p: int(p.rsplit(".part", 1)[1][:-4]))
    if not parts:
        raise FileNotFoundError(f"no golden {name!r} in {golden_dir}")
    raw = {}
    for p in parts:
        raw.update(np.load(p))
    out = {k: v for k, v in raw.items() if "#" not in k}
    for key in {k.split("#", 1)[0] for k in raw if k.endswith("#shape")}:
        n = sum(1 for k in raw if k.startswith(key + "#") and k != key + "#shape")
        out[key] = np.concatenate([raw[f"{key}#{i}"] for i in range(n)]).reshape(tuple(raw[key + "#shape"]))
    return out


def save(name, arrays, golden_dir=GOLDEN, part_bytes=PART_BYTES):
    """Write golden NAME: one compressed NAME.npz when the arrays fit one part, else NAME.part<k>.npz (stale files of NAME go first)."""
    for p in [os.path.join(golden_dir, name + ".npz")] + glob.glob(os.path.join(golden_dir, glob.escape(name) + ".part*.npz")):
        if os.path.exists(p):
            os.remove(p)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    assert not any("#" in k for k in arrays), "'#' is reserved for chunk keys"
    if sum(a.nbytes for a in arrays.values()) <= part_bytes:
        np.savez_compressed(os.path.join(golden_dir, name + ".npz"), **arrays)
        return
    pieces = []
    for k, a in arrays.items():
        if a.nbytes <= part_bytes:
            pieces.append((k, a))
            continue
        flat = np.ascontiguousarray(a).reshape(-1)
        step = max(1, part_bytes // a.itemsize)
        pieces += [(f"{k}#{i}", flat[o:o + step]) for i, o in enumerate(range(0, flat.size, step))]
        pieces.append((f"{k}#shape", np.array(a.shape, dtype=np.int64)))
    vols, cur, size = [], {}, 0
    for k, a in pieces:
        if cur and size + a.nbytes > part_bytes:
            vols.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    vols.append(cur)
    for i, v in enumerate(vols):
        np.savez_compressed(os.path.join(golden_dir, f"{name}.part{i}.npz"), **v)
