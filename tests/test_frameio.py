"""CPU: the NumPy restatement of the 8-bit frame I/O (tests/frameio_ref.py) against the formulas the reference uses, bit for bit -- evalrig.rgb2yuv /
yuv2rgb and `(x * 255.).clip(0., 255.).round()` in torch, `astype(np.float32) / 255.`, gaze.RegionMasks and `gt * mk`; the C-ABI's declaration,
binding and argument checks (none reaches a device); the Python surface without a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import frameio_ref as fref

T = torch.from_numpy


def torch_display(rgb):
    """test_video.py:403-406 on an RGB tensor: (sr * 255.).clip(0., 255.), round(), uint8, HWC"""
    return (rgb * 255.).clip(0., 255.).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()


def test_export_equals_the_torch_formulas_bit_for_bit():
    from crfp_amd import evalrig
    rs = np.random.RandomState(11)
    sr = rs.uniform(-0.2, 1.2, (2, 3, 19, 23)).astype(np.float32)
    want = torch_display(T(sr))
    assert 0.2 < float(((sr < 0) | (sr > 1)).mean()) < 0.5   # a good share of the values is clipped
    assert np.array_equal(fref.export(sr), want)
    assert np.array_equal(fref.export(sr, bgr=True), want[..., ::-1])
    # y_only (test_video.py:396-402): the chroma of an RGB frame under the predicted luma
    y = rs.uniform(-0.2, 1.2, (2, 1, 19, 23)).astype(np.float32)
    chroma = rs.uniform(-0.2, 1.2, (2, 3, 19, 23)).astype(np.float32)
    yuv = evalrig.rgb2yuv(T(chroma))
    yuv[:, 0] = T(y)[:, 0]
    rgb = evalrig.yuv2rgb(yuv)
    assert np.array_equal(fref.merge(y, chroma).view(np.int32), rgb.numpy().view(np.int32))
    assert np.array_equal(fref.export(y, chroma), torch_display(rgb))
    assert np.array_equal(fref.export(y, chroma, bgr=True), torch_display(rgb)[..., ::-1])


def test_ties_round_to_even_and_specials():
    v, want = fref.ties()
    assert np.array_equal(v * np.float32(255.0), np.arange(255, dtype=np.float32) + np.float32(0.5))
    assert np.array_equal(fref.quant(v), want)
    assert np.array_equal(T(v).mul(255.).clip(0., 255.).round().to(torch.uint8).numpy(), want)
    tiny = np.float32(1e-45)
    special = np.array([-0.0, 0.0, tiny, -tiny, np.inf, -np.inf, np.nan, 1.0, 2.0, -1.0], np.float32)
    assert fref.quant(special).tolist() == [0, 0, 0, 0, 255, 0, 0, 255, 255, 0]


def test_ingest_equals_astype_float32_over_255_on_all_codes():
    codes = np.arange(256, dtype=np.uint8)
    want = codes.astype(np.float32) / 255.
    assert want.dtype == np.float32 and np.array_equal(fref.unit(codes).view(np.int32), want.view(np.int32))
    assert np.array_equal(want, (T(codes).float() / 255.).numpy())
    recip = codes.astype(np.float32) * np.float32(1.0 / 255.0)
    assert int((recip != want).sum()) == 126          # why the kernel divides
    # export o ingest is the identity on every code
    frame = np.stack([codes, codes[::-1], np.roll(codes, 7)], -1).reshape(1, 16, 16, 3)
    for bgr in (False, True):
        assert np.array_equal(fref.export(fref.ingest_lr(frame, bgr), bgr=bgr), frame)
    assert np.array_equal(fref.ingest_lr(frame, True), fref.ingest_lr(frame)[:, ::-1])


@pytest.mark.parametrize("H,W,fv,origins", [(23, 45, 8, [(0, 0), (15, 37), (7, 13), (0, 37)]), (64, 96, 32, [(32, 64), (5, 9), (16, 0)])])
def test_scatter_equals_region_masks_and_gt_times_mk(H, W, fv, origins):
    from crfp_amd import gaze
    rs = np.random.RandomState(5)
    masks = gaze.RegionMasks(H, W, fv, "cpu")
    for n, (y, x) in enumerate(origins):
        frame = rs.randint(0, 256, (1, H, W, 3)).astype(np.uint8)
        gt = T(fref.ingest_lr(frame))
        mk = masks.frame(n, y, x)["mk"]
        rect = np.array([[y, x, fref.HAS_FOVEA, 0]], np.int32)
        got_fv, got_mk = fref.ingest_fovea(frame[:, y:y + fv, x:x + fv], rect, H, W)
        assert np.array_equal(got_mk.astype(bool), mk.numpy())
        assert np.array_equal(got_fv.view(np.int32), (gt * mk).numpy().view(np.int32))
        off = fref.ingest_fovea(frame[:, y:y + fv, x:x + fv], np.array([[y, x, 0, 0]], np.int32), H, W)
        assert not off[0].any() and not off[1].any()


def test_clip_rect_handles_every_origin():
    big = 2 ** 31 - 1
    assert fref.clip_rect(-3, 40, 8, 8, 1, 23, 45) == (0, 5, 40, 45)
    assert fref.clip_rect(-big - 1, big, 96, 96, 1, 23, 45) == (0, 0, 45, 45)
    assert fref.clip_rect(big, -big - 1, 96, 96, 1, 23, 45) == (23, 23, 0, 0)
    assert fref.clip_rect(3, 4, 8, 8, 2, 23, 45) == (0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_declares_and_ctypes_binds_the_symbols():
    from crfp_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crfp_hip.h")).read())
    assert ("int crfp_frame_ingest_u8(const uint8_t* lr_u8, const uint8_t* crop_u8, const int32_t* rects, float* lr, float* fv, uint8_t* mk, int n, "
            "int h, int w, int fh, int fw, int H, int W, int flags, void* stream);") in hdr
    assert "int crfp_frame_export_u8(const float* sr, const float* chroma, uint8_t* out_u8, int n, int c, int H, int W, int flags, void* stream);" in hdr
    for line in ("#define CRFP_IO_BGR 1", "#define CRFP_IO_RECT_INTS 4", "#define CRFP_IO_HAS_FOVEA 1"):
        assert line in hdr
    assert (_lib.IO_BGR, _lib.IO_RECT_INTS, _lib.IO_HAS_FOVEA) == (fref.BGR, fref.RECT_INTS, fref.HAS_FOVEA) == (1, 4, 1)
    assert _lib.SIGNATURES["crfp_frame_ingest_u8"] == (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 8 + [C.c_void_p])
    assert _lib.SIGNATURES["crfp_frame_export_u8"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p])


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


BADARG, UNSUPPORTED = -1, -3


def test_ingest_argument_errors_do_not_touch_the_gpu(lib):
    """Every refusal comes with its code and the error string set; this runs on a machine without a GPU, where any HIP call would fail with
    another code."""
    p = 16   # a non-null pointer value no check dereferences
    call = lambda *a: lib.crfp_frame_ingest_u8(*a, None)   # noqa: E731
    err = lib.crfp_last_error_string
    ok = [p, p, p, p, p, p, 2, 24, 32, 8, 8, 192, 256, 0]
    for hole in (0, 3):              # lr_u8 without lr, lr without lr_u8
        a = list(ok)
        a[hole] = None
        assert call(*a) == BADARG and b"lr_u8 and lr" in err(), hole
    for holes in ((1,), (2,), (4,), (5,), (1, 2), (4, 5), (1, 2, 4), (2, 4, 5)):   # a part of crop_u8 / rects / fv / mk
        a = list(ok)
        for k in holes:
            a[k] = None
        assert call(*a) == BADARG and b"go together" in err() and b"crop_u8" in err(), holes
    assert call(None, None, None, None, None, None, *ok[6:]) == BADARG and b"nothing to do" in err()
    for pos in range(6, 13):         # n, h, w, fh, fw, H, W
        for bad in (0, -1):
            a = list(ok)
            a[pos] = bad
            assert call(*a) == BADARG and b"bad argument" in err(), (pos, bad)
    for flags in (2, 4, 3, -1, 1 << 30):
        a = list(ok)
        a[13] = flags
        assert call(*a) == BADARG and b"unknown flags" in err() and b"BGR flag" in err(), flags
    for a in (ok, [None, p, p, None, p, p] + ok[6:], [p, None, None, p, None, None] + ok[6:]):   # both halves, the fovea alone, the LR frame alone
        a = list(a)
        a[6] = 65536
        assert call(*a) == UNSUPPORTED and b"65535" in err()


def test_export_argument_errors_do_not_touch_the_gpu(lib):
    p = 16
    call = lambda *a: lib.crfp_frame_export_u8(*a, None)   # noqa: E731
    err = lib.crfp_last_error_string
    ok3, ok1 = [p, None, p, 2, 3, 24, 32, 0], [p, p, p, 2, 1, 24, 32, 0]
    for ok in (ok3, ok1):
        for hole in (0, 2):          # sr, out_u8
            a = list(ok)
            a[hole] = None
            assert call(*a) == BADARG and b"null" in err(), hole
        for pos in (3, 5, 6):        # n, H, W
            for bad in (0, -1):
                a = list(ok)
                a[pos] = bad
                assert call(*a) == BADARG and b"bad argument" in err(), (pos, bad)
        for flags in (2, 3, -1):
            a = list(ok)
            a[7] = flags
            assert call(*a) == BADARG and b"unknown flags" in err(), flags
        a = list(ok)
        a[3] = 65536
        assert call(*a) == UNSUPPORTED and b"65535" in err()
    for c in (0, 2, 4, -1):
        assert call(p, p, p, 2, c, 24, 32, 0) == BADARG and b"c must be 1 or 3" in err(), c
    assert call(p, p, p, 2, 3, 24, 32, 0) == BADARG and b"chroma" in err()      # chroma with c = 3
    assert call(p, None, p, 2, 1, 24, 32, 0) == BADARG and b"chroma" in err()   # none with c = 1


def test_python_surface_without_a_device():
    from crfp_amd import frameio
    assert list(inspect.signature(frameio.ingest).parameters) == ["lr_u8", "crop_u8", "rects", "H", "W", "bgr"]
    assert list(inspect.signature(frameio.export).parameters) == ["sr", "chroma", "bgr", "out"]
    assert list(inspect.signature(frameio.HostStreamer.__init__).parameters)[:7] == ["self", "model", "h", "w", "fv_size", "depth", "bgr"]
    assert inspect.signature(frameio.HostStreamer.__init__).parameters["depth"].default == 2
    u8 = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        frameio.ingest(u8, u8, torch.zeros((1, 4), dtype=torch.int32), 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        frameio.export(torch.zeros((1, 3, 4, 4)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        frameio.HostStreamer(object(), 4, 4, 8, device="cpu")
    # 180 x 320, fv 96: the table of DESIGN.md section 3.7
    mb = frameio.pcie_bytes(180, 320, 96)
    assert mb == {"fp32": 691200 + 44236800 + 3686400 + 44236800, "u8": 172800 + 27648 + 16 + 11059200}
