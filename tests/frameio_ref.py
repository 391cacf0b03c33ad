"""NumPy float32 restatement of crfp_frame_ingest_u8 / crfp_frame_export_u8 (include/crfp_hip.h): every operation is one float32 ufunc, so
every intermediate is rounded once, as in the kernels (built with -ffp-contract=off)."""
import numpy as np

F = np.float32
BGR, RECT_INTS, HAS_FOVEA = 1, 4, 1


def unit(u8):
    """astype(np.float32) / 255. (dataset/reds.py:306,409): IEEE division."""
    return u8.astype(np.float32) / F(255.0)


def ingest_lr(lr_u8, bgr=False):
    """[n,h,w,3] uint8 -> [n,3,h,w] float32"""
    x = lr_u8[..., ::-1] if bgr else lr_u8
    return np.ascontiguousarray(unit(x).transpose(0, 3, 1, 2))


def clip_rect(y, x, fh, fw, flags, H, W):
    """R = [y, y + fh) x [x, x + fw) intersected with the frame, in Python integers: (y0, y1, x0, x1), empty without the HAS_FOVEA bit."""
    if not int(flags) & HAS_FOVEA:
        return 0, 0, 0, 0
    y, x = int(y), int(x)
    c = lambda v, hi: max(min(v, hi), 0)   # noqa: E731
    return c(y, H), c(y + fh, H), c(x, W), c(x + fw, W)


def ingest_fovea(crop_u8, rects, H, W, bgr=False):
    """crop_u8 [n,fh,fw,3] uint8, rects [n,4] (y, x, flags, 0) -> fv [n,3,H,W] float32 (+0 outside R), mk [n,1,H,W] uint8"""
    n, fh, fw, _ = crop_u8.shape
    fv, mk = np.zeros((n, 3, H, W), np.float32), np.zeros((n, 1, H, W), np.uint8)
    src = crop_u8[..., ::-1] if bgr else crop_u8
    for i in range(n):
        y, x = int(rects[i][0]), int(rects[i][1])
        y0, y1, x0, x1 = clip_rect(y, x, fh, fw, rects[i][2], H, W)
        if y0 < y1 and x0 < x1:
            fv[i, :, y0:y1, x0:x1] = unit(src[i, y0 - y:y1 - y, x0 - x:x1 - x]).transpose(2, 0, 1)
            mk[i, 0, y0:y1, x0:x1] = 1
    return fv, mk


def quant(v):
    """(uint8)rintf(fminf(fmaxf(v * 255.0f, 0.0f), 255.0f)): NaN -> 0, ties to even"""
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.fmin(np.fmax(v * F(255.0), F(0.0)), F(255.0))
    return np.rint(t).astype(np.uint8)


def merge(y, chroma):
    """y [n,1,H,W], chroma [n,3,H,W] RGB -> RGB [n,3,H,W]: u, v of chroma under the luma y (test_video.py:100-127,401-402), this association"""
    assert y.dtype == np.float32 and chroma.dtype == np.float32
    y, r, g, b = y[:, 0], chroma[:, 0], chroma[:, 1], chroma[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((F(-0.147) * r) - (F(0.289) * g)) + (F(0.436) * b)
        v = ((F(0.615) * r) - (F(0.515) * g)) - (F(0.100) * b)
        return np.stack([y + (F(1.14) * v), (y + (F(-0.396) * u)) - (F(0.581) * v), y + (F(2.029) * u)], 1)


def export(sr, chroma=None, bgr=False):
    """sr [n,c,H,W] float32 (c = 3, or c = 1 with chroma [n,3,H,W]) -> [n,H,W,3] uint8"""
    assert (sr.shape[1] == 3 and chroma is None) or (sr.shape[1] == 1 and chroma is not None)
    rgb = sr if chroma is None else merge(sr, chroma)
    out = quant(np.ascontiguousarray(rgb)).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out[..., ::-1] if bgr else out)


def ties():
    """For k = 0..254 a float32 v with v * 255.0f == k + 0.5 exactly (one exists for every k), and the value it must round to (the even one)."""
    vs = []
    for k in range(255):
        c = F(k + 0.5) / F(255.0)
        cand = [v for v in (c, np.nextafter(c, F(0.0)), np.nextafter(c, F(1.0))) if v * F(255.0) == F(k + 0.5)]
        assert cand, k
        vs.append(cand[0])
    return np.array(vs, np.float32), np.array([k if k % 2 == 0 else k + 1 for k in range(255)], np.uint8)
