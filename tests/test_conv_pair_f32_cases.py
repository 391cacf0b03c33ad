"""CPU: the host side of the fp32 pair-kernel tests (tests/helpers/conv_pair_f32_cases.py, tests/test_gpu_conv_pair_f32.py): the probe's
mode 4 and its kernel id, what each build refuses, workspace sizing, and the exactness conditions of every case the GPU test holds to
float64."""
import ctypes
import dataclasses
import os
import subprocess

import pytest

from conftest import ROOT
from helpers import conv_pair_f32_cases as pc
from test_conv_cases import _desc, _kernels


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


def test_mode_and_kernel_id_are_appended():
    from crfp_amd import _lib
    assert _lib.PROBE_MODES == {"single": 0, "dual": 1, "pair": 2, "s3_chain": 3, "pair_f32": 4}
    assert _lib.CONV_KERNELS[-1] == "split_pair" and _lib.CONV_KERNELS.index("split_pair") == 12 and _lib.CONV_KERNELS[11] == "bf16_pair"


@pytest.mark.parametrize("shape", ["res", "block"])
def test_mode_4_reaches_the_pair_kernel(lib, shape):
    conv_a, conv_b = pc.SHAPES[shape]
    for h, w in pc.GEOMETRY:
        assert _kernels(lib, "f32", "pair_f32", _desc(conv_a), _desc(conv_b, False), pc.N, h, w) == ("split_pair", "split_pair"), (h, w)


def test_each_build_refuses_the_other_builds_pair_mode(lib):
    from crfp_amd import _lib
    a, b = _desc(pc.RES_A), _desc(pc.RES_B, False)
    k = (ctypes.c_int * 2)()
    assert lib.crfp_conv_probe_kernel_bf16(_lib.PROBE_MODES["pair_f32"], ctypes.byref(a), ctypes.byref(b), 2, 8, 62, k) == -3
    assert b"fp32 build only" in lib.crfp_last_error_string()
    assert lib.crfp_conv_probe_kernel(_lib.PROBE_MODES["pair"], ctypes.byref(a), ctypes.byref(b), 2, 8, 62, k) == -3
    assert b"bf16 build only" in lib.crfp_last_error_string()
    assert lib.crfp_conv_probe_kernel(5, ctypes.byref(a), ctypes.byref(b), 2, 8, 62, k) == -1 and b"unknown mode" in lib.crfp_last_error_string()


def test_workspace_sizing(lib):
    """Mode 4 lays out what the bf16 pair mode lays out (no tensor between the convs), in fp32 elements; conv a needs no destination, and a
    second conv is required."""
    from crfp_amd import _lib
    ws, ws16 = lib.crfp_conv_probe_workspace_bytes, lib.crfp_conv_probe_workspace_bytes_bf16
    m4, m2 = _lib.PROBE_MODES["pair_f32"], _lib.PROBE_MODES["pair"]
    for shape in ("res", "block"):
        conv_a, conv_b = pc.SHAPES[shape]
        a, b = _desc(conv_a), _desc(conv_b, False)
        small, big = ws(m4, ctypes.byref(a), ctypes.byref(b), 2, 8, 62), ws(m4, ctypes.byref(a), ctypes.byref(b), 2, 19, 130)
        assert 0 < small < big
        assert ws16(m4, ctypes.byref(a), ctypes.byref(b), 2, 8, 62) == 0
        assert ws16(m2, ctypes.byref(a), ctypes.byref(b), 2, 8, 62) < small   # bf16 activations are half the size
        # the two launches it replaces need conv a's output tensor on top: 2 x 32 channels x 8 x 62 floats
        a1 = _desc(dataclasses.replace(conv_a, dsts=None))
        assert ws(0, ctypes.byref(a1), None, 2, 8, 62) > 0
    a = _desc(pc.RES_A)
    assert ws(m4, ctypes.byref(a), None, 2, 8, 62) == 0 and b"null conv descriptor" in lib.crfp_last_error_string()


@pytest.mark.parametrize("which", pc.EXACT_KINDS)
@pytest.mark.parametrize("shape", ["res", "block_relu"])
def test_exact_cases_meet_their_conditions(shape, which):
    for h, w in pc.GEOMETRY:
        assert pc.exact_ok(shape, h, w, which), (shape, h, w, which)
    assert not pc.exact_ok("block", 8, 62, which)   # lrelu: never held to float64
