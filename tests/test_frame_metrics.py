"""CPU: the frame metrics table -- the float64 yardstick (tests/frame_metrics_ref.py) against the reference-generated values of
tests/golden/ops_small.npz (the fixture test_masked_psnr_ssim_golden_and_oracle reads) and against the fp32 oracle on the cases of
tests/test_gpu_frame_metrics.py; the C-ABI's declarations, bindings and argument checks (none reaches a device); the Python defaults."""
import inspect
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import frame_metrics_ref as fref

T = torch.from_numpy
PSNR_TOL, SSIM_TOL = 1e-4, 2e-6   # the project's metric tolerances (tests/test_gpu_parity.py: dB, SSIM)


@pytest.fixture(scope="module")
def orc():
    from oracle import crfp_oracle
    return crfp_oracle


def test_yardstick_against_the_reference_generated_golden(ops_golden):
    g = ops_golden
    sr, hr = T(g["metric_sr"]), T(g["metric_hr"])
    masks = torch.cat([T(g["metric_box"]), T(g["metric_ring"])], 1)
    t = fref.table(sr, hr, masks, luma_on=True)
    assert t.shape == (1, 3, 4) and t.dtype == torch.float64
    for row, tag in enumerate(("", "_box", "_ring")):
        assert abs(float(t[0, row, 0]) - float(g["metric_psnr" + tag])) < PSNR_TOL, tag
        assert abs(float(t[0, row, 1]) - float(g["metric_ssim" + tag])) < SSIM_TOL, tag
    assert abs(float(t[0, 0, 2]) - float(g["metric_psnr_y"])) < PSNR_TOL and abs(float(t[0, 0, 3]) - float(g["metric_ssim_y"])) < SSIM_TOL
    t255 = fref.table(sr * 255.0, hr * 255.0, masks[:, :1])      # the [0, 255] branch
    assert abs(float(t255[0, 1, 0]) - float(g["metric_psnr_box255"])) < PSNR_TOL
    assert abs(float(t255[0, 1, 1]) - float(g["metric_ssim_box255"])) < SSIM_TOL
    assert torch.isnan(t255[:, :, 2:]).all()                     # luma off


def test_the_ragged_case_takes_every_branch():
    sr, hr, masks = fref.ragged_case()
    assert sr.shape == (5, 3, 70, 150) and masks.shape == (5, 3, 70, 150) and masks.dtype == torch.bool
    span = [float(hr[i].max() - hr[i].min()) for i in range(5)]
    yspan = [float(fref.luma(hr[i:i + 1]).max() - fref.luma(hr[i:i + 1]).min()) for i in range(5)]
    assert span[0] <= 0.9 and span[1] >= 2.2 and 1.1 <= span[2] <= 1.8 and span[3] <= 0.9 and span[4] <= 0.9
    assert min(yspan[:3]) >= 2.2 and yspan[3] <= 0.9 and 1.1 <= yspan[4] <= 1.8
    assert abs(yspan[3] - 0.876) < 0.01 and abs(yspan[4] - 1.533) < 0.01
    dens = masks.float().mean((0, 2, 3))
    assert abs(float(dens[0]) - 0.6) < 0.02 and abs(float(dens[1]) - 0.1) < 0.02
    assert masks[0, 2, 9:41, 50:140].all() and int(masks[0, 2].sum()) == 32 * 90     # crosses tile rows 0..2 and columns 0..2


def test_yardstick_against_the_fp32_oracle_on_the_gpu_cases(orc):
    """The oracle is the same formulae in float32, so it differs from the yardstick by its own rounding.  PSNR: the project's 1e-4 dB.
    SSIM: the project's 2e-6 where the map is well conditioned; in general one unit roundoff (2^-24) of the filtered second moments
    amplified by kappa = mean((mu1^2 + mu2^2) / (sigma1^2 + sigma2^2 + C2)), the factor by which E[x^2] - mu^2 cancels.  kappa is about 5
    for noise in [0, 1], about 600 for the pairs confined to 0.5 +- 0.004 and 5e5 for their unconverted luma near 125, where the
    oracle's SSIM-Y is only good to a few 1e-3."""
    sr, hr, masks = fref.ragged_case()
    yard, ora = fref.table(sr, hr, masks, luma_on=True), fref.oracle_table(orc, sr, hr, masks, luma_on=True)
    kappa = fref.conditioning(sr, hr, luma_on=True)
    assert float(kappa[0, 0]) < 20 and float(kappa[3, 1]) > 1e5
    for i in range(5):
        for col in range(4):
            tol = PSNR_TOL if col % 2 == 0 else max(SSIM_TOL, 2.0 ** -24 * float(kappa[i, col // 2]))
            d = float((yard[i, :, col] - ora[i, :, col]).abs().max())
            print(f"frame {i} column {col}: |oracle - yardstick| {d:.3e}, bound {tol:.3e}")
            assert d < tol, (i, col, d, tol)
    for name, a, b in fref.small_cases():
        luma_on = a.shape[1] == 3
        yard, ora = fref.table(a, b, None, luma_on), fref.oracle_table(orc, a, b, None, luma_on)
        d = (yard - ora).abs()[0, 0]
        assert float(d[0]) < PSNR_TOL and float(d[1]) < SSIM_TOL, name
        assert (float(d[2]) < PSNR_TOL and float(d[3]) < SSIM_TOL) if luma_on else bool(torch.isnan(yard[0, 0, 2:]).all()), name
    # the formulae themselves, without fp32 noise: the oracle's code evaluated in float64
    a, b, mk = sr[3:4].double(), hr[3:4].double(), masks[3:4, 0:1].double()
    p, s = orc.calc_psnr_and_ssim(fref.luma(a), fref.luma(b), mk)
    assert abs(p - float(yard_row(sr, hr, masks, 3)[1, 2])) < 1e-9 and abs(s - float(yard_row(sr, hr, masks, 3)[1, 3])) < 1e-9


def yard_row(sr, hr, masks, i):
    return fref.table(sr[i:i + 1], hr[i:i + 1], masks[i:i + 1], luma_on=True)[0]


def test_yardstick_floor_value_and_empty_region():
    _, hr, masks = fref.ragged_case()
    masks = masks[:1].clone()
    masks[0, 1] = False
    t = fref.table(hr[:1], hr[:1], masks, luma_on=True)[0]
    import math
    assert t[0, 0] == -20 * math.log10(math.sqrt((1 / 255.0) ** 2 / (3 * 70 * 150))) and t[0, 2] == -20 * math.log10(math.sqrt((1 / 255.0) ** 2 / (70 * 150)))
    assert t[0, 1] == 1.0 and t[0, 3] == 1.0
    assert torch.isnan(t[2]).all() and not torch.isnan(t[[0, 1, 3]]).any()


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_declares_and_ctypes_binds_both_symbols():
    import ctypes as C
    from crfp_amd import _lib
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "crfp_hip.h")).read())
    assert "size_t crfp_frame_metrics_workspace_bytes(int n, int m, int h, int w);" in hdr
    assert ("int crfp_frame_metrics_f32(const float* sr, const float* hr, const uint8_t* masks, double* out, int n, int c, int m, int h, "
            "int w, int flags, void* workspace, size_t workspace_bytes, void* stream);") in hdr
    assert "#define CRFP_METRICS_LUMA 1" in hdr and _lib.METRICS_LUMA == 1
    assert _lib.SIGNATURES["crfp_frame_metrics_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)
    assert _lib.SIGNATURES["crfp_frame_metrics_f32"] == (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t, C.c_void_p])


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


def test_frame_metrics_sizing_and_argument_errors_do_not_touch_the_gpu(lib):
    p = 16   # a non-null pointer value no check dereferences
    size = lib.crfp_frame_metrics_workspace_bytes
    probe = 256 * 4 * 4
    assert size(1, 0, 16, 64) == probe + 1 * 1 * 5 * 8 and size(1, 0, 17, 65) == probe + 4 * 1 * 5 * 8
    assert size(5, 3, 70, 150) == 5 * (probe + 15 * 4 * 5 * 8) and size(1, 7, 1, 1) == probe + 8 * 5 * 8
    assert size(0, 0, 8, 8) == 0 and size(1, 8, 8, 8) == 0 and size(1, -1, 8, 8) == 0 and size(1, 0, 0, 8) == 0
    wsb = size(2, 3, 24, 31)
    call = lambda *a: lib.crfp_frame_metrics_f32(*a, None)   # noqa: E731
    for hole in (0, 1, 3):
        ptrs = [None if j == hole else p for j in range(4)]
        assert call(*ptrs, 2, 3, 3, 24, 31, 0, p, wsb) == -1
        assert b"null" in lib.crfp_last_error_string()
    assert call(p, p, None, p, 2, 3, 3, 24, 31, 0, p, wsb) == -1 and b"masks" in lib.crfp_last_error_string()
    for n, c, m in ((0, 3, 3), (-1, 3, 3), (2, 0, 3), (2, 5, 3), (2, 3, -1), (2, 3, 8)):
        assert call(p, p, p, p, n, c, m, 24, 31, 0, p, 1 << 30) == -1, (n, c, m)
    assert call(p, p, p, p, 2, 1, 3, 24, 31, 1, p, wsb) == -1 and b"LUMA" in lib.crfp_last_error_string()
    assert call(p, p, p, p, 2, 4, 3, 24, 31, 1, p, wsb) == -1
    assert call(p, p, p, p, 2, 3, 3, 24, 31, 1, p, wsb - 1) == -2 and b"workspace" in lib.crfp_last_error_string()   # CRFP_E_WORKSPACE
    assert call(p, p, p, p, 2, 3, 3, 24, 31, 1, None, wsb) == -2


def test_python_defaults_and_surface_without_a_device():
    from crfp_amd import evalrig, gaze, utils
    assert inspect.signature(evalrig.eval_clip).parameters["fused"].default is False
    assert inspect.signature(evalrig.eval_reds).parameters["fused_metrics"].default is False
    assert inspect.signature(gaze.run_gaze_video).parameters["fused_metrics"].default is False
    sig = inspect.signature(utils.frame_metrics_table).parameters
    assert list(sig) == ["sr", "hr", "masks", "luma"] and sig["masks"].default is None and sig["luma"].default is False
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.frame_metrics_table(torch.zeros(1, 3, 20, 20), torch.zeros(1, 3, 20, 20))
