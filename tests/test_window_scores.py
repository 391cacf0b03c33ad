"""CPU: the foveated score maps -- the restatement (tests/window_scores_ref.py) against the committed values of the reference's own
foveated_metric / utils.calc_psnr_and_ssim_cuda (tests/golden/fov_scores.npz, written by tests/golden/make_fovscore_golden.py), and the
argument checks of crfp_window_scores_f32, none of which reaches a device."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import window_scores_ref as wref

T = torch.from_numpy
PSNR_FLOOR, SSIM_FLOOR = 1e-4, 2e-6   # the project's metric tolerances (tests/test_gpu_parity.py: dB, SSIM)


@pytest.fixture(scope="module")
def fov():
    return dict(np.load(os.path.join(GOLDEN, "fov_scores.npz")))


def case(g, i):
    c = f"c{i}_"
    return T(g[c + "hr"]), T(g[c + "sr"]), int(g[c + "k"]), int(g[c + "s"])


def test_cases_are_the_ones_the_maps_were_specified_on(fov):
    assert int(fov["n_cases"]) == 9
    shapes = [(tuple(fov[f"c{i}_hr"].shape[1:]), int(fov[f"c{i}_k"]), int(fov[f"c{i}_s"])) for i in range(1, 10)]
    assert shapes == [((10, 10), 10, 5), ((24, 31), 10, 5), ((75, 130), 10, 5), ((29, 40), 7, 3), ((40, 48), 12, 12), ((20, 22), 16, 1)] + \
        [((24, 31), 10, 5)] * 3
    assert fov["c3_psnr64"].shape == (14, 25) and fov["c2_psnr64"].shape == (3, 5)
    spans = []
    for i in (7, 8, 9):   # the three range branches, decided by sr's covered pixels alone
        sr = fov[f"c{i}_sr"][:, :20, :30]
        spans.append(float(sr.max() - sr.min()))
    assert spans[0] > 2 and 1 < spans[1] <= 2 and spans[2] <= 1
    assert fov["c9_sr"].max() - fov["c9_sr"].min() > 2      # ... although the whole image of case 9 spans more
    for i in range(2, 10):
        assert fov[f"c{i}_equal"].sum() >= 2


@pytest.mark.parametrize("i", range(1, 10))
def test_float64_restatement_is_the_stored_yardstick(fov, i):
    hr, sr, k, s = case(fov, i)
    p, q = wref.window_scores(hr, sr, k, s, torch.float64)
    assert np.array_equal(p.numpy(), fov[f"c{i}_psnr64"]) and np.array_equal(q.numpy(), fov[f"c{i}_ssim64"])
    eq = fov[f"c{i}_equal"]
    assert np.all(p.numpy()[eq] == wref.floor_psnr(3, k)) and np.all(q.numpy()[eq] == 1.0)
    # the stored deviation of the reference's fp32 path from it
    assert float(fov[f"c{i}_ref_err_psnr"]) == np.abs(fov[f"c{i}_ref_psnr"] - p.numpy()).max() < 1e-4
    assert float(fov[f"c{i}_ref_err_ssim"]) == np.abs(fov[f"c{i}_ref_ssim"] - q.numpy()).max() < 2e-5


@pytest.mark.parametrize("i", range(1, 10))
def test_float32_restatement_reproduces_the_reference_maps(fov, i):
    """In float32 the gaussian filter is torch's grouped convolution over the unfolded windows (window_scores_unfold): the values the
    reference stored carry that operation's rounding.  Measured when the fixture was made: 0 on every case.  Another fp32 summation
    order (window_scores(dtype=float32): taps added one by one) is up to 1.0e-5 away from them in SSIM on the flat-region windows of
    cases 5 and 6, where E[x^2] - mu^2 cancels to a rounding error that is compared with C2 = 9e-4 -- as far as the reference itself is
    from exact arithmetic (ref_err_ssim 8.4e-6 on case 5); the test below holds that form to the bound the GPU kernel is held to."""
    hr, sr, k, s = case(fov, i)
    p, q = wref.window_scores_unfold(hr, sr, k, s)
    dp, dq = np.abs(p.numpy() - fov[f"c{i}_ref_psnr"]).max(), np.abs(q.numpy() - fov[f"c{i}_ref_ssim"]).max()
    print(f"case {i}: fp32 composition vs reference maps: {dp:.3e} dB, {dq:.3e} SSIM")
    assert dp <= PSNR_FLOOR and dq <= SSIM_FLOOR
    # the reference's return values are those maps transformed
    assert np.abs(p.numpy() / 100 - fov[f"c{i}_psnr_score"]).max() <= PSNR_FLOOR / 100
    assert np.abs((q.numpy().clip(0, 1) - 0.7) / 0.3 - fov[f"c{i}_ssim_score"]).max() <= SSIM_FLOOR / 0.3
    ext = np.array([p.min(), p.max(), q.min(), q.max()])
    assert np.all(np.abs(ext - fov[f"c{i}_extrema"]) <= [PSNR_FLOOR, PSNR_FLOOR, SSIM_FLOOR, SSIM_FLOOR])


@pytest.mark.parametrize("i", range(1, 10))
def test_separable_float32_meets_the_bound_set_for_the_kernel(fov, i):
    """rows-then-columns in fp32 (the kernel's form, here on the CPU) against the float64 yardstick within max(floor, 4 x ref_err)."""
    hr, sr, k, s = case(fov, i)
    p, q = wref.window_scores(hr, sr, k, s, torch.float32)
    assert np.abs(p.numpy() - fov[f"c{i}_psnr64"]).max() <= max(PSNR_FLOOR, 4 * float(fov[f"c{i}_ref_err_psnr"]))
    assert np.abs(q.numpy() - fov[f"c{i}_ssim64"]).max() <= max(SSIM_FLOOR, 4 * float(fov[f"c{i}_ref_err_ssim"]))


def test_truncation_and_isolation_of_a_window():
    """k > 11: positions more than 5 apart do not see each other; and nothing outside a window reaches its score."""
    rs = np.random.RandomState(3)
    hr, sr = (T(rs.rand(3, 12, 30).astype(np.float32)) for _ in range(2))
    p, q = wref.window_scores(hr, sr, 12, 9)
    hr2, sr2 = hr.clone(), sr.clone()
    hr2[:, :, 12:18] = 0.0   # the columns between / after windows 0 (0..11) and 1 (9..20): only window 1 and 2 change
    p2, q2 = wref.window_scores(hr2, sr2, 12, 9)
    assert p2[0, 0] == p[0, 0] and q2[0, 0] == q[0, 0] and p2[0, 1] != p[0, 1]
    pu, qu = wref.window_scores_unfold(hr.double(), sr.double(), 12, 9)
    assert float((pu - p).abs().max()) < 1e-9 and float((qu - q).abs().max()) < 1e-7   # 2-D fp32 weights vs g[i] g[j]: 1e-8


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


def test_window_scores_argument_errors_do_not_touch_the_gpu(lib):
    p = 16   # a non-null pointer value no check dereferences
    wsb = lib.crfp_window_scores_workspace_bytes(1)
    assert wsb > 0 and lib.crfp_window_scores_workspace_bytes(4) == 4 * wsb and lib.crfp_window_scores_workspace_bytes(0) == 0
    call = lambda *a: lib.crfp_window_scores_f32(*a, None)   # noqa: E731
    for hole in range(4):
        ptrs = [None if j == hole else p for j in range(4)]
        assert call(*ptrs, 1, 3, 24, 31, 10, 5, p, wsb) == -1
        assert b"null" in lib.crfp_last_error_string()
    assert call(p, p, p, p, 1, 3, 24, 31, 17, 5, p, wsb) == -3            # CRFP_E_UNSUPPORTED
    assert b"16" in lib.crfp_last_error_string()
    assert call(p, p, p, p, 1, 3, 9, 31, 10, 5, p, wsb) == -1             # h < k
    assert call(p, p, p, p, 1, 3, 24, 9, 10, 5, p, wsb) == -1             # w < k
    assert call(p, p, p, p, 1, 3, 24, 31, 10, 5, p, wsb - 1) == -1        # one byte short
    assert b"workspace" in lib.crfp_last_error_string()
    assert call(p, p, p, p, 1, 3, 24, 31, 10, 5, None, wsb) == -1
    for n, c, k, s in ((0, 3, 10, 5), (1, 0, 10, 5), (1, 3, 0, 5), (1, 3, 10, 0), (-1, 3, 10, 5)):
        assert call(p, p, p, p, n, c, 24, 31, k, s, p, wsb) == -1


def test_python_surface_without_a_device():
    from crfp_amd import gaze, utils
    import inspect
    assert list(inspect.signature(utils.foveated_metric).parameters) == ["LR", "LR_fv", "HR", "mn", "hw", "crop", "kernel_size", "stride_size",
                                                                         "eval_mode"]
    assert inspect.signature(utils.foveated_metric).parameters["eval_mode"].default is False
    sig = inspect.signature(utils.window_scores).parameters
    assert list(sig) == ["sr", "hr", "kernel_size", "stride"] and sig["kernel_size"].default == 10 and sig["stride"].default == 5
    g = inspect.signature(gaze.run_gaze_video).parameters
    assert g["score_maps"].default is False and g["baseline"].default is None
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.window_scores(torch.zeros(3, 20, 20), torch.zeros(3, 20, 20))
    with pytest.raises(NotImplementedError):   # out of scope, as before
        utils.psnr_cuda(None, None, None, batch_avg=True)
