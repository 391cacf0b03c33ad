"""CPU: the rectangle form of the gaze rig's masks -- gaze.rect_table rasterised by the NumPy restatement of crfp_gaze_prep_f32's definition
(tests/gaze_rects_ref.py) against the composed gaze.RegionMasks on the same origins, bit for bit; the C-ABI's declaration, binding and
argument checks (none reaches a device); the Python defaults."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import gaze_rects_ref as gref


@pytest.mark.parametrize("name", sorted(gref.CASES))
def test_rasterised_rect_table_equals_region_masks(name):
    from crfp_amd import gaze
    H, W, fv, fv_start, rg, origins = gref.CASES[name]
    assert gref.covers_the_edge_cases(H, W, fv, origins), name
    assert all(gaze.window_origin(x + fv // 2, y + fv // 2, fv, H, W) == (y, x) for y, x in origins)   # values window_origin can return
    rows = gaze.rect_table(origins, H, W, fv, fv_start=fv_start, regional_dcn=rg > 0, rg_h=rg, rg_w=rg)
    assert rows.dtype == np.int32 and rows.shape == (len(origins), gref.ROW_INTS)
    masks = gaze.RegionMasks(H, W, fv, "cpu", fv_start, rg > 0, rg, rg)
    for n, (cur_y, cur_x) in enumerate(origins):
        ref, got = masks.frame(n, cur_y, cur_x), gref.rasterise(rows[n], H, W)
        for k in ("mk", "fovea", "outskirt", "fg"):
            assert np.array_equal(got[k], ref[k][0, 0].numpy()), (name, n, k)
        if n == 0:
            assert ref["past"] is None and not got["past"].any()
        else:
            assert np.array_equal(got["past"], ref["past"][0, 0].numpy()), (name, n, "past")
        assert got["mk"].any() == (n >= fv_start) and got["fovea"].sum() == fv * fv


def test_rect_table_layout():
    from crfp_amd import _lib, gaze
    origins = [(0, 0), (3, 5), (3, 5), (10, 20), (6, 7)]
    rows = gaze.rect_table(origins, 40, 64, 8, fv_start=2, regional_dcn=True, rg_h=12, rg_w=16)
    assert (_lib.GAZE_ROW_INTS, _lib.GAZE_EXISTS, _lib.GAZE_COUNTS) == (24, 1, 2)
    assert rows[4].tolist() == [4, 16, 3, 19,  6, 7, 8, 8, 3,  10, 20, 8, 8, 3,  3, 5, 8, 8, 3,  3, 5, 8, 8, 1]
    assert rows[0].tolist() == [0, 10, 0, 12,  0, 0, 8, 8, 1] + [0] * 15
    assert rows[1].tolist()[4:] == [3, 5, 8, 8, 1,  0, 0, 8, 8, 1] + [0] * 10
    assert gaze.rect_table(origins, 40, 64, 8)[3].tolist()[:9] == [0, 40, 0, 64,  10, 20, 8, 8, 3]   # no regional box: the whole frame
    assert gaze.rect_table([], 40, 64, 8).shape == (0, 24)


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_declares_and_ctypes_binds_the_symbol():
    import ctypes as C
    from crfp_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crfp_hip.h")).read())
    assert ("int crfp_gaze_prep_f32(const float* gt, const int32_t* rows, float* fv, uint8_t* mk, uint8_t* regions, uint8_t* fg, int n, int c, "
            "int h, int w, int dilate, void* stream);") in hdr
    assert "#define CRFP_GAZE_ROW_INTS 24" in hdr
    assert _lib.SIGNATURES["crfp_gaze_prep_f32"] == (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p])


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


def test_gaze_prep_argument_errors_do_not_touch_the_gpu(lib):
    """Every refusal is CRFP_E_BADARG with the error string set; this runs on a machine without a GPU, where any HIP call would fail with
    another code."""
    p = 16   # a non-null pointer value no check dereferences
    call = lambda *a: lib.crfp_gaze_prep_f32(*a, None)   # noqa: E731
    ok = [p, p, p, p, p, p, 2, 3, 24, 32, 10]
    for hole in (1, 3, 4, 5):   # rows, mk, regions, fg
        a = list(ok)
        a[hole] = None
        assert call(*a) == -1 and b"null" in lib.crfp_last_error_string(), hole
    for hole in (0, 2):         # gt without fv, fv without gt
        a = list(ok)
        a[hole] = None
        assert call(*a) == -1 and b"gt and fv" in lib.crfp_last_error_string(), hole
    for pos in (6, 7, 8, 9):    # n, c, h, w
        for bad in (0, -1):
            a = list(ok)
            a[pos] = bad
            assert call(*a) == -1 and b"bad argument" in lib.crfp_last_error_string(), (pos, bad)
    a = list(ok)
    a[10] = -1
    assert call(*a) == -1 and b"dilate" in lib.crfp_last_error_string()
    a = [None, p, None, p, p, p, 0, 3, 24, 32, 10]   # masks only is legal, n = 0 is not
    assert call(*a) == -1 and b"bad argument" in lib.crfp_last_error_string()


def test_python_defaults_and_surface_without_a_device():
    from crfp_amd import gaze
    assert inspect.signature(gaze.run_gaze_video).parameters["fused_masks"].default is False
    assert list(inspect.signature(gaze.rect_table).parameters) == ["origins", "H", "W", "fv_size", "fv_start", "regional_dcn", "rg_h", "rg_w"]
    ctor = list(inspect.signature(gaze.FusedRegionMasks.__init__).parameters)
    assert ctor[:-1] == list(inspect.signature(gaze.RegionMasks.__init__).parameters) and ctor[-1] == "origins"
    with pytest.raises(RuntimeError, match="no CPU path"):
        gaze.FusedRegionMasks(16, 32, 8, "cpu", origins=[(0, 0)])
