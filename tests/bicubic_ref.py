"""NumPy restatement of PIL's 8-bit bicubic resize (Image.resize(..., Image.BICUBIC) on an 8-bit image; include/crfp_hip.h, csrc/bicubic.hip):
tap tables in Python floats -- IEEE doubles, one rounding per operation -- and integer arithmetic on the pixels."""
import math

import numpy as np

BITS = 22

# h, w -> H, W: x8 (one pixel, tiny, odd, several tiles), ragged factors, one axis kept, the identity, shrinking, the rig's frame
PAIRS = [(1, 1, 8, 8), (3, 3, 24, 24), (5, 7, 40, 56), (17, 23, 136, 184), (2, 5, 16, 40), (9, 11, 10, 13), (7, 5, 24, 33), (24, 32, 24, 256),
         (8, 8, 8, 8), (64, 96, 8, 12), (45, 80, 17, 31), (134, 240, 1072, 1920)]


def cubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def ksize(in_size, out_size):
    return int(math.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1


def taps(in_size, out_size):
    """-> bounds [out, 2] int32 (xmin, cnt), taps [out, ksize] int32 (zero from cnt on)"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ks = ksize(in_size, out_size)
    bounds, k = np.zeros((out_size, 2), np.int32), np.zeros((out_size, ks), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)          # int(): truncation, as the C conversion
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w = [cubic((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, cnt)
        k[xx, :cnt] = [int(v * 4194304 + (-0.5 if v < 0 else 0.5)) for v in w]
    return bounds, k


def resample_axis(img, out_size, axis):
    """img uint8 [..]: one pass along `axis`, 32-bit accumulators, arithmetic shift, clamp"""
    bounds, k = taps(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], np.int32)
    for xx in range(out_size):
        xmin, cnt = bounds[xx]
        acc = np.full(src.shape[1:], 1 << (BITS - 1), np.int32)
        for x in range(cnt):
            acc = acc + src[xmin + x] * k[xx, x]
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize(img, H, W):
    """img uint8 [h,w,c] -> [H,W,c]: along x into an 8-bit image, then along y; an axis that keeps its size is skipped"""
    if W != img.shape[1]:
        img = resample_axis(img, W, 1)
    if H != img.shape[0]:
        img = resample_axis(img, H, 0)
    return np.ascontiguousarray(img)


def pil_resize(img, H, W):
    """the reference's call (test_video.py:241) on one uint8 [h,w,3] frame"""
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((W, H), Image.BICUBIC))


def contents(rs, shape):
    """the three kinds of content: uniform random; 0 and 255 only (overshoot into both clamps); a narrow band around 128"""
    return {"uniform": rs.randint(0, 256, shape).astype(np.uint8), "binary": (rs.randint(0, 2, shape) * 255).astype(np.uint8),
            "band": rs.randint(126, 131, shape).astype(np.uint8)}
