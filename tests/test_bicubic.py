"""CPU: the NumPy restatement of PIL's 8-bit bicubic resize (tests/bicubic_ref.py) against PIL itself, byte for byte; crfp_bicubic_taps (the host
side of the function the device runs) against the restatement's tables, int for int; the C-ABI's declaration, binding and argument checks
(none reaches a device); the Python surface without a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import bicubic_ref as bref

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3


@pytest.mark.parametrize("h,w,H,W", bref.PAIRS)
def test_restatement_equals_pil_byte_for_byte(h, w, H, W):
    rs = np.random.RandomState(h * 1000 + W)
    for kind, img in bref.contents(rs, (h, w, 3)).items():
        want = bref.pil_resize(img, H, W)
        got = bref.resize(img, H, W)
        assert got.dtype == np.uint8 and got.shape == (H, W, 3) and np.array_equal(got, want), kind
        if kind == "binary" and H >= 8 * h and W >= 8 * w and h > 1 and w > 1:
            assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()


def test_an_axis_that_keeps_its_size_has_identity_taps():
    """PIL skips such an axis; the kernels run it: the same bytes"""
    for size in (1, 2, 8, 33):
        bounds, k = bref.taps(size, size)
        for xx in range(size):
            row = np.zeros(size, np.int64)
            row[bounds[xx, 0]:bounds[xx, 0] + bounds[xx, 1]] = k[xx, :bounds[xx, 1]]
            assert row[xx] == 1 << bref.BITS and not np.delete(row, xx).any()


def test_upscaling_needs_four_taps_of_five_and_a_patch_of_tile_plus_three():
    """what the fused kernel's LDS layout rests on"""
    for i, o in [(1, 8), (3, 24), (7, 56), (23, 184), (9, 10), (5, 33), (32, 256), (47, 376), (8, 8), (134, 1072), (240, 1920), (63, 64), (100, 101)]:
        bounds, k = bref.taps(i, o)
        assert k.shape[1] == 5 and bounds[:, 1].max() <= 4 and bounds[:, 1].min() >= 1
        ends = bounds.sum(1)
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(ends) >= 0).all() and ends.max() <= i
        for tile in (32, 64):
            for a in range(0, o, tile):
                b = min(a + tile, o) - 1
                assert ends[b] - bounds[a, 0] <= b - a + 1 + 3


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_declares_and_ctypes_binds_the_symbols():
    from crfp_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crfp_hip.h")).read())
    for decl in ("int crfp_bicubic_taps(int in_size, int out_size, int32_t* bounds, int32_t* taps, int taps_capacity);",
                 "size_t crfp_resize_bicubic_workspace_bytes(int n, int h, int w, int H, int W);",
                 "int crfp_resize_bicubic_u8(const uint8_t* src, void* dst, int n, int h, int w, int H, int W, int flags, void* workspace, "
                 "size_t workspace_bytes, void* stream);",
                 "int crfp_frame_export_y_bicubic_u8(const float* luma, const uint8_t* lr_u8, uint8_t* out_u8, int n, int h, int w, int H, int W, "
                 "int flags, void* workspace, size_t workspace_bytes, void* stream);",
                 "#define CRFP_IO_OUT_F32 2", "#define CRFP_IO_TWO_PASS 4"):
        assert decl in hdr, decl
    assert (_lib.IO_BGR, _lib.IO_OUT_F32, _lib.IO_TWO_PASS) == (1, 2, 4)
    assert _lib.SIGNATURES["crfp_bicubic_taps"] == (C.c_int, [C.c_int] * 2 + [C.POINTER(C.c_int32)] * 2 + [C.c_int])
    assert _lib.SIGNATURES["crfp_resize_bicubic_workspace_bytes"] == (C.c_size_t, [C.c_int] * 5)
    assert _lib.SIGNATURES["crfp_resize_bicubic_u8"] == (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p])
    assert _lib.SIGNATURES["crfp_frame_export_y_bicubic_u8"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p])


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


def host_taps(lib, i, o, slack=0):
    ks = bref.ksize(i, o)
    bounds, k = np.full((o, 2), -7, np.int32), np.full((o * ks + slack + 1,), -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    rc = lib.crfp_bicubic_taps(i, o, p(bounds), p(k), o * ks + slack)
    assert k[-1] == -7
    return rc, bounds, k[:o * ks].reshape(o, ks)


def test_host_taps_equal_the_restatement_on_every_axis(lib):
    axes = sorted({(h, H) for h, w, H, W in bref.PAIRS} | {(w, W) for h, w, H, W in bref.PAIRS} | {(33, 264), (47, 376), (180, 1440), (320, 2560)})
    for i, o in axes:
        want_b, want_k = bref.taps(i, o)
        rc, bounds, k = host_taps(lib, i, o, slack=3)
        assert rc == want_k.shape[1] == bref.ksize(i, o), (i, o)
        assert np.array_equal(bounds, want_b) and np.array_equal(k, want_k), (i, o)
    assert {bref.ksize(i, o) for i, o in axes} >= {5, 13, 33}   # upscaling, 45 -> 17, 64 -> 8


def test_taps_argument_errors(lib):
    err = lib.crfp_last_error_string
    i32 = C.POINTER(C.c_int32)
    b, k = (C.c_int32 * 16)(), (C.c_int32 * 40)()
    assert lib.crfp_bicubic_taps(1, 8, None, k, 40) == BADARG and b"null" in err()
    assert lib.crfp_bicubic_taps(1, 8, b, C.cast(None, i32), 40) == BADARG and b"null" in err()
    for i, o in ((0, 8), (-1, 8), (1, 0), (1, -3)):
        assert lib.crfp_bicubic_taps(i, o, b, k, 40) == BADARG and b"bad argument" in err(), (i, o)
    k[39] = 77
    assert lib.crfp_bicubic_taps(1, 8, b, k, 39) == WORKSPACE and b"39 ints" in err() and k[39] == 77   # one int short
    assert lib.crfp_bicubic_taps(1, 8, b, k, -1) == WORKSPACE
    assert lib.crfp_bicubic_taps(1, 8, b, k, 40) == 5
    assert lib.crfp_bicubic_taps(2 ** 31 - 1, 1, b, k, 40) == UNSUPPORTED and b"int" in err()
    assert lib.crfp_bicubic_taps(2 ** 31 - 1, 2 ** 31 - 1, b, k, 40) == UNSUPPORTED


def test_workspace_sizes(lib):
    size = lib.crfp_resize_bicubic_workspace_bytes
    tables = lambda h, w, H, W: 4 * ((2 + bref.ksize(w, W)) * W + (2 + bref.ksize(h, H)) * H)   # noqa: E731
    for n, h, w, H, W in ((1, 1, 1, 8, 8), (2, 17, 23, 136, 184), (1, 64, 96, 8, 12), (3, 45, 80, 17, 31), (1, 180, 320, 1440, 2560)):
        assert size(n, h, w, H, W) == (tables(h, w, H, W) + 15) // 16 * 16 + n * h * W * 3, (n, h, w, H, W)
    for bad in ((0, 8, 8, 8, 8), (1, 0, 8, 8, 8), (1, 8, -1, 8, 8), (1, 8, 8, 0, 8), (1, 8, 8, 8, 0), (65536, 8, 8, 8, 8), (1, 2 ** 31 - 1, 8, 1, 8)):
        assert size(*bad) == 0, bad


def test_resize_argument_errors_do_not_touch_the_gpu(lib):
    """Every refusal comes with its code and the error string set; this runs on a machine without a GPU, where any HIP call would fail with
    another code."""
    p = 16   # a non-null, 16-byte aligned pointer value no check dereferences
    err = lib.crfp_last_error_string
    need = lib.crfp_resize_bicubic_workspace_bytes(2, 3, 5, 24, 40)
    assert need > 0
    ok = [p, p, 2, 3, 5, 24, 40, 0, p, need]
    call = lambda *a: lib.crfp_resize_bicubic_u8(*a, None)   # noqa: E731
    for hole in (0, 1):
        a = list(ok)
        a[hole] = None
        assert call(*a) == BADARG and b"null" in err(), hole
    for pos in range(2, 7):          # n, h, w, H, W
        for bad in (0, -1):
            a = list(ok)
            a[pos] = bad
            assert call(*a) == BADARG and b"bad argument" in err(), (pos, bad)
    for flags in (8, 16, -1, 1 << 30):
        a = list(ok)
        a[7] = flags
        assert call(*a) == BADARG and b"unknown flags" in err(), flags
    for ws, nbytes in ((None, need), (p, need - 1), (p, 0)):
        a = list(ok)
        a[8], a[9] = ws, nbytes
        assert call(*a) == WORKSPACE and b"workspace too small" in err(), (ws, nbytes)
    a = list(ok)
    a[8] = 20
    assert call(*a) == BADARG and b"aligned" in err()
    a = list(ok)
    a[2], a[9] = 65536, 1 << 40
    assert call(*a) == UNSUPPORTED and b"65535" in err()


def test_export_y_bicubic_argument_errors_do_not_touch_the_gpu(lib):
    p = 16
    err = lib.crfp_last_error_string
    need = lib.crfp_resize_bicubic_workspace_bytes(2, 3, 5, 24, 40)
    ok = [p, p, p, 2, 3, 5, 24, 40, 0, p, need]
    call = lambda *a: lib.crfp_frame_export_y_bicubic_u8(*a, None)   # noqa: E731
    for hole in (0, 1, 2):
        a = list(ok)
        a[hole] = None
        assert call(*a) == BADARG and b"null" in err(), hole
    for pos in range(3, 8):
        for bad in (0, -1):
            a = list(ok)
            a[pos] = bad
            assert call(*a) == BADARG and b"bad argument" in err(), (pos, bad)
    for flags in (2, 4, 3, -1):      # the resize call's flags are not this call's
        a = list(ok)
        a[8] = flags
        assert call(*a) == BADARG and b"unknown flags" in err() and b"BGR flag" in err(), flags
    for ws, nbytes in ((None, need), (p, need - 1)):
        a = list(ok)
        a[9], a[10] = ws, nbytes
        assert call(*a) == WORKSPACE and b"workspace too small" in err(), (ws, nbytes)
    # a geometry the fused path does not take: refused before any launch
    for h, w, H, W in ((24, 5, 3, 40), (3, 40, 24, 5), (24, 40, 3, 5)):
        a = list(ok)
        a[4:8] = h, w, H, W
        a[10] = lib.crfp_resize_bicubic_workspace_bytes(2, h, w, H, W)
        assert call(*a) == UNSUPPORTED and b"fused path" in err(), (h, w, H, W)


def test_python_surface_without_a_device():
    from crfp_amd import frameio, gaze
    assert list(inspect.signature(frameio.resize_bicubic).parameters) == ["src_u8", "H", "W", "out", "bgr"]
    assert [p.default for p in inspect.signature(frameio.resize_bicubic).parameters.values()][3:] == ["u8", False]
    assert list(inspect.signature(frameio.export_y_bicubic).parameters) == ["luma", "lr_u8", "bgr", "out"]
    streamer = inspect.signature(frameio.HostStreamer.__init__).parameters
    assert list(streamer)[-1] == "chroma" and streamer["chroma"].default == "bilinear"
    u8 = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="'u8' or 'f32'"):
        frameio.resize_bicubic(u8, 32, 32, out="bf16")
    with pytest.raises(RuntimeError, match="no CPU path"):
        frameio.resize_bicubic(u8, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        frameio.export_y_bicubic(torch.zeros((1, 1, 32, 32)), u8)
    with pytest.raises(ValueError, match="'bilinear' or 'bicubic'"):
        frameio.HostStreamer(object(), 4, 4, 8, chroma="lanczos")
    assert "--baseline" in inspect.getsource(gaze.main)
