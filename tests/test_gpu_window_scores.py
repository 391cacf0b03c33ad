"""GPU (-m gpu): the fused foveated score maps (crfp_window_scores_f32 through crfp_amd.utils.window_scores / foveated_metric and
crfp_amd.gaze.run_gaze_video) against tests/golden/fov_scores.npz and the restatement tests/window_scores_ref.py.

Parity is taken against the float64 evaluation of the formula (psnr64 / ssim64), per case within max(project floor, 4 x ref_err): the
floor is the project's metric tolerance (1e-4 dB, 2e-6), ref_err how far the reference's own fp32 path is from exact arithmetic on that
case, and the factor 4 covers the second rounding of the separable filter and the fused multiply-adds."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

import window_scores_ref as wref

pytestmark = pytest.mark.gpu

T = torch.from_numpy
PSNR_FLOOR, SSIM_FLOOR = 1e-4, 2e-6


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fov():
    return dict(np.load(os.path.join(GOLDEN, "fov_scores.npz")))


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


def case(g, i):
    c = f"c{i}_"
    return T(g[c + "hr"]), T(g[c + "sr"]), int(g[c + "k"]), int(g[c + "s"])


def tolerances(g, i):
    return max(PSNR_FLOOR, 4 * float(g[f"c{i}_ref_err_psnr"])), max(SSIM_FLOOR, 4 * float(g[f"c{i}_ref_err_ssim"]))


@pytest.mark.parametrize("i", range(1, 10))
def test_raw_maps_against_float64(fov, i):
    from crfp_amd import utils as U
    hr, sr, k, s = case(fov, i)
    p, q = U.window_scores(sr.to(dev()), hr.to(dev()), k, s)
    p, q = p.cpu().numpy(), q.cpu().numpy()
    assert p.dtype == np.float32 and p.shape == fov[f"c{i}_psnr64"].shape == q.shape
    tp, tq = tolerances(fov, i)
    dp, dq = np.abs(p - fov[f"c{i}_psnr64"]).max(), np.abs(q - fov[f"c{i}_ssim64"]).max()
    print(f"case {i}: |psnr - psnr64| = {dp:.3e} dB (tol {tp:.1e}), |ssim - ssim64| = {dq:.3e} (tol {tq:.1e})")
    assert dp <= tp and dq <= tq
    eq = fov[f"c{i}_equal"]
    assert np.all(p[eq] == np.float32(wref.floor_psnr(3, k))) and np.all(p[eq] == fov[f"c{i}_psnr64"][eq].astype(np.float32))
    assert np.all(q[eq] == 1.0)
    assert not np.any(p[~eq] == np.float32(wref.floor_psnr(3, k)))


@pytest.mark.parametrize("i", range(1, 10))
def test_foveated_metric_mirror(fov, i):
    from crfp_amd import utils as U
    hr, sr, k, s = case(fov, i)
    d_hr, d_sr = hr.to(dev()), sr.to(dev())
    ps, ss, (pmin, pmax), (smin, smax) = U.foveated_metric(None, d_sr, d_hr, (0, 0), tuple(hr.shape[1:]), (k, k), k, s, eval_mode=True)
    assert torch.equal(d_hr.cpu(), hr) and torch.equal(d_sr.cpu(), sr)     # eval mode draws nothing
    tp, tq = tolerances(fov, i)
    assert np.abs(ps.cpu().numpy() - fov[f"c{i}_psnr_score"]).max() <= tp / 100
    assert np.abs(ss.cpu().numpy() - fov[f"c{i}_ssim_score"]).max() <= tq / 0.3
    ext = np.array([float(pmin), float(pmax), float(smin), float(smax)])
    assert np.all(np.abs(ext - fov[f"c{i}_extrema"]) <= [tp, tp, tq, tq])


def test_foveated_metric_draws_the_rectangle_in_place(fov):
    from crfp_amd import utils as U
    hr, sr, k, s = case(fov, 2)
    d_hr, d_sr = hr.to(dev()), sr.to(dev())
    mn, crop = tuple(int(v) for v in fov["c2_mn"]), tuple(int(v) for v in fov["c2_crop"])
    ps, ss, _, _ = U.foveated_metric(None, d_sr, d_hr, mn, tuple(hr.shape[1:]), crop, k, s, eval_mode=False)
    assert torch.equal(d_hr.cpu(), T(fov["c2_hr_drawn"])) and torch.equal(d_sr.cpu(), T(fov["c2_sr_drawn"]))
    tp, tq = tolerances(fov, 2)   # scored before drawing
    assert np.abs(ps.cpu().numpy() - fov["c2_psnr_score"]).max() <= tp / 100
    assert np.abs(ss.cpu().numpy() - fov["c2_ssim_score"]).max() <= tq / 0.3
    with pytest.raises(ValueError):
        U.foveated_metric(None, d_sr[:1], d_hr[:1], mn, tuple(hr.shape[1:]), crop, k, s, eval_mode=True)


def pair(seed, n, c, h, w):
    rs = np.random.RandomState(seed)
    hr = rs.rand(n, c, h, w).astype(np.float32)
    sr = np.clip(hr + rs.normal(0, 0.05, hr.shape), 0, 1).astype(np.float32)
    sr[:, :, :12, :17] = hr[:, :, :12, :17]
    if n > 1:
        sr[1] *= 255.0; hr[1] *= 255.0        # every image of a batch picks its own range conversion
    if n > 2:
        sr[2, 0, 20, 5] = 1.7
    return T(hr), T(sr)


@pytest.mark.parametrize("h,w", [(33, 47), (75, 130)])
def test_batch_stream_and_dirty_buffers(h, w):
    """n = 3 in one call == three calls; a side stream gives the same bits; so do outputs and workspace full of NaN bytes."""
    from crfp_amd import _lib, utils as U
    hr, sr = pair(h, 3, 3, h, w)
    d_hr, d_sr = hr.to(dev()), sr.to(dev())
    P, Q = U.window_scores(d_sr, d_hr)
    assert P.shape == (3, (h - 10) // 5 + 1, (w - 10) // 5 + 1) and bool(torch.isfinite(P).all()) and bool(torch.isfinite(Q).all())
    for b in range(3):
        p, q = U.window_scores(d_sr[b], d_hr[b])
        assert torch.equal(p, P[b]) and torch.equal(q, Q[b]), b
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        P2, Q2 = U.window_scores(d_sr, d_hr)
    side.synchronize()
    assert torch.equal(P2, P) and torch.equal(Q2, Q)
    # straight through the C-ABI with every byte of the outputs and of the workspace set to 0xFF (NaN as floats)
    L = _lib.lib()
    wsb = L.crfp_window_scores_workspace_bytes(3)
    ws = torch.full((wsb,), 255, dtype=torch.uint8, device=dev())
    P3, Q3 = torch.empty_like(P), torch.empty_like(Q)
    P3.view(torch.uint8).fill_(255)
    Q3.view(torch.uint8).fill_(255)
    assert bool(torch.isnan(P3).all()) and bool(torch.isnan(Q3).all())
    rc = L.crfp_window_scores_f32(d_hr.data_ptr(), d_sr.data_ptr(), P3.data_ptr(), Q3.data_ptr(), 3, 3, h, w, 10, 5, ws.data_ptr(), wsb,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(P3, P) and torch.equal(Q3, Q)
    # textured images (no flat region, variances far above C2): fp32 rounding leaves ~4e-6 dB and ~3e-7, so the project floors hold
    p64, q64 = wref.window_scores(hr, sr, 10, 5)
    assert float((P.cpu() - p64).abs().max()) <= PSNR_FLOOR and float((Q.cpu() - q64).abs().max()) <= SSIM_FLOOR


@pytest.mark.parametrize("h,w", [(33, 47), (75, 130)])
def test_one_channel(h, w):
    """C = 1 (the y_only models' frames) against the restatement; the floor of an equal window follows C."""
    from crfp_amd import utils as U
    hr, sr = pair(h + 1, 1, 1, h, w)
    p, q = U.window_scores(sr[0].to(dev()), hr[0].to(dev()), 10, 5)
    p64, q64 = wref.window_scores(hr[0], sr[0], 10, 5)
    assert float((p.cpu() - p64).abs().max()) <= PSNR_FLOOR and float((q.cpu() - q64).abs().max()) <= SSIM_FLOOR   # textured: see above
    assert float(p[0, 0]) == np.float32(wref.floor_psnr(1, 10)) and float(q[0, 0]) == 1.0


def test_gaze_rig_score_maps():
    """run_gaze_video(score_maps=True, baseline=...) for 3 frames at 16 x 24 LR: frame by frame the maps are utils.foveated_metric of the
    frame the model returned, the extrema are the running ones of the baseline's maps, and the region metrics are those of a run
    without score maps."""
    from crfp_amd import gaze, synth, utils as U
    from crfp_amd.model import CRFP
    sd = synth.make_state_dict(7)
    h, w, N, fv = 16, 24, 3, 32
    lr = T(synth.make_clip(21, 1, N, h, w, fv_size=fv)[0][0]).to(dev())
    base = F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False)
    gt = torch.clamp(base + T(np.random.RandomState(4).normal(0, 0.02, (N, 3, 8 * h, 8 * w)).astype(np.float32)).to(dev()), 0, 1)
    m = CRFP.MRCF_simple_v18(device=dev(), mid_channels=32)
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev()).eval()

    class Recorder:
        def __init__(self):
            self.frames = []

        def clear_states(self):
            m.clear_states()

        def __call__(self, **kw):
            out = m(**kw)
            self.frames.append(out.reshape(3, 8 * h, 8 * w).clone())
            return out

    rec = Recorder()
    res = gaze.run_gaze_video(rec, lr, gt, sigma=6.0, fv_size=fv, seed=11, score_maps=True, baseline=base)
    plain = gaze.run_gaze_video(m, lr, gt, sigma=6.0, fv_size=fv, seed=11)
    Hr, Wr = wref.map_size(8 * h, 8 * w, 10, 5)
    assert res["psnr_score"].shape == (N, Hr, Wr) == res["ssim_score_baseline"].shape and res["psnr_score"].is_cuda
    ext = [1000.0, 0.0, 1000.0, 0.0]
    for n in range(N):
        ps, ss, _, _ = U.foveated_metric(None, rec.frames[n], gt[n], (0, 0), (8 * h, 8 * w), (fv, fv), 10, 5, eval_mode=True)
        assert torch.equal(res["psnr_score"][n], ps) and torch.equal(res["ssim_score"][n], ss)
        pb, sb, (p0, p1), (s0, s1) = U.foveated_metric(None, base[n], gt[n], (0, 0), (8 * h, 8 * w), (fv, fv), 10, 5, eval_mode=True)
        assert torch.equal(res["psnr_score_baseline"][n], pb) and torch.equal(res["ssim_score_baseline"][n], sb)
        ext = [min(ext[0], float(p0)), max(ext[1], float(p1)), min(ext[2], float(s0)), max(ext[3], float(s1))]
    assert [float(v) for v in res["score_extrema"].cpu()] == [float(np.float32(v)) for v in ext]
    assert "psnr_score" not in plain and set(plain) == set(res) - {"psnr_score", "ssim_score", "psnr_score_baseline", "ssim_score_baseline",
                                                                   "score_extrema"}
    assert plain["per_frame"] == res["per_frame"] and plain["trajectory"] == res["trajectory"]
    for r in ("whole", "fovea", "outskirt", "past"):
        assert plain[f"psnr_{r}"] == res[f"psnr_{r}"] and plain[f"ssim_{r}"] == res[f"ssim_{r}"]
