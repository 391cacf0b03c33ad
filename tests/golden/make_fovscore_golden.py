"""Generates tests/golden/fov_scores.npz by EXECUTING the reference's own foveated_metric (/root/reference/test_video.py:23-98) and
utils.calc_psnr_and_ssim_cuda (/root/reference/utils.py:242-254, batch_avg=True).  test_video.py is a script (importing it would start
the rig), so this reads the file where it lies, takes the statements of that one function and runs them against the reference's utils
module, imported from where it lies with ``cv2`` / ``visdom`` / ``imageio`` stubbed (not installed, not used by these functions).  Nothing
of the reference is copied into the repository: only the inputs and the results are stored.  Per case:
  hr, sr                      the two [3,H,W] float32 images (sr = the model output, the second argument `LR_fv`)
  k, s                        window side and stride
  psnr_score, ssim_score      the reference's first two return values for eval_mode=True (psnr/100, (ssim.clip(0,1)-0.7)/0.3)
  extrema                     its other two, (psnr.min, psnr.max, ssim.min, ssim.max) of the raw maps
  ref_psnr, ref_ssim          the raw maps of the reference's utils.calc_psnr_and_ssim_cuda on the unfolded windows (float32)
  psnr64, ssim64              the raw maps of tests/window_scores_ref.py in float64
  ref_err_psnr, ref_err_ssim  max |ref - 64|: how close the reference's own fp32 path is to exact arithmetic
and for case 2 the two images as eval_mode=False leaves them (the crop rectangle drawn in), with mn and crop.
Run in the build container (needs /root/reference): python tests/golden/make_fovscore_golden.py"""
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "fov_scores.npz")
sys.path.insert(0, os.path.dirname(HERE))
import window_scores_ref as wref  # noqa: E402


def reference_functions():
    for name in ("cv2", "visdom", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    import utils as ref_utils   # the reference's
    lines = open(os.path.join(REF, "test_video.py")).read().splitlines()
    i0 = next(i for i, l in enumerate(lines) if l.startswith("def foveated_metric("))
    i1 = next(i for i, l in enumerate(lines) if i > i0 and l.startswith("def "))
    env = dict(torch=torch, F=F, np=np, calc_psnr_and_ssim_cuda=ref_utils.calc_psnr_and_ssim_cuda)
    exec(textwrap.dedent("\n".join(lines[i0:i1])), env)
    return env["foveated_metric"], ref_utils.calc_psnr_and_ssim_cuda


def images(rs, H, W, k, s):
    """Smooth (bilinear-upsampled) noise + N(0, 0.05) noise per image, clipped to [0, 1]; a flat region hr = 0.5 / sr = 0.51 over the
    last windows (E[x^2] - mu^2 cancels against C2 there); sr == hr on a box at the top left (exactly equal windows)."""
    base = F.interpolate(torch.from_numpy(rs.rand(1, 3, H // 6 + 2, W // 6 + 2).astype(np.float32)), size=(H, W), mode="bilinear",
                         align_corners=False)[0].numpy()
    hr = np.clip(base + 0.05 * rs.standard_normal((3, H, W)), 0, 1).astype(np.float32)
    sr = np.clip(base + 0.05 * rs.standard_normal((3, H, W)), 0, 1).astype(np.float32)
    Hr, Wr = wref.map_size(H, W, k, s)
    if Hr * Wr > 1:
        y0, x0 = (Hr - 1) * s, max(Wr - 2, 0) * s
        hr[:, y0:, x0:] = 0.5
        sr[:, y0:, x0:] = 0.51
        sr[:, :k, :k + s] = hr[:, :k, :k + s]
    return hr, sr


def main():
    assert os.path.isdir(REF), "reference not mounted: run this in the build container"
    fov, calc = reference_functions()
    torch.set_grad_enabled(False)
    rs = np.random.RandomState(20240607)
    T = torch.from_numpy
    cases = []
    for H, W, k, s in ((10, 10, 10, 5), (24, 31, 10, 5), (75, 130, 10, 5), (29, 40, 7, 3), (40, 48, 12, 12), (20, 22, 16, 1)):
        cases.append((*images(rs, H, W, k, s), k, s))
    hr2, sr2 = cases[1][0], cases[1][1]
    cases.append((hr2 * 255.0, sr2 * 255.0, 10, 5))            # 7: the /255 branch
    sr8 = sr2.copy(); sr8[0, 12, 4] = 1.5; sr8[1, 17, 22] = 0.0  # 8: span (1, 2] inside the covered area -> (x+1)/2
    cases.append((hr2, sr8, 10, 5))
    sr9 = sr2.copy(); sr9[:, 20:, :] = 300.0; sr9[:, :, 30] = -5.0   # 9: out of range only where no window reaches -> no conversion
    cases.append((hr2, sr9, 10, 5))
    out = {"n_cases": np.asarray(len(cases))}
    for i, (hr, sr, k, s) in enumerate(cases, 1):
        H, W = hr.shape[1:]
        Hr, Wr = wref.map_size(H, W, k, s)
        ps, ss, (pmin, pmax), (smin, smax) = fov(None, T(sr.copy()), T(hr.copy()), (0, 0), (H, W), (k, k), k, s, eval_mode=True)
        fold = lambda x: F.unfold(T(x)[None], kernel_size=k, stride=s).permute(0, 2, 1).reshape(Hr * Wr, 3, k, k)   # noqa: E731
        rp, rss = calc(fold(hr), fold(sr), torch.ones(Hr * Wr, 1, k, k), is_tensor=False, batch_avg=True)
        rp, rss = rp.view(Hr, Wr).numpy(), rss.view(Hr, Wr).numpy()
        assert np.array_equal(rp / np.float32(100), ps.numpy()) and float(pmin) == rp.min() and float(smax) == rss.max()
        p64, s64 = (v.numpy() for v in wref.window_scores(T(hr), T(sr), k, s, torch.float64))
        equal = np.array([[np.array_equal(hr[:, y * s:y * s + k, x * s:x * s + k], sr[:, y * s:y * s + k, x * s:x * s + k])
                           for x in range(Wr)] for y in range(Hr)])
        assert Hr * Wr == 1 or equal.sum() >= 2, "no exactly equal windows"
        assert np.all(p64[equal] == wref.floor_psnr(3, k)) and np.all(s64[equal] == 1.0)
        c = f"c{i}_"
        out.update({c + "hr": hr, c + "sr": sr, c + "k": np.asarray(k), c + "s": np.asarray(s), c + "psnr_score": ps.numpy(),
                    c + "ssim_score": ss.numpy(), c + "extrema": np.asarray([float(pmin), float(pmax), float(smin), float(smax)], np.float32),
                    c + "ref_psnr": rp, c + "ref_ssim": rss, c + "psnr64": p64, c + "ssim64": s64, c + "equal": equal,
                    c + "ref_err_psnr": np.asarray(np.abs(rp - p64).max()), c + "ref_err_ssim": np.asarray(np.abs(rss - s64).max())})
        print(f"case {i}: {H}x{W} k={k} s={s} map {Hr}x{Wr} equal windows {int(equal.sum())} psnr {p64.min():.2f}..{p64.max():.2f} "
              f"ssim {s64.min():.4f}..{s64.max():.4f} ref_err {out[c + 'ref_err_psnr']:.2e} dB / {out[c + 'ref_err_ssim']:.2e}")
    # the in-place rectangle of eval_mode=False on case 2
    hr, sr, k, s = cases[1]
    mn, crop = (3, 4), (12, 14)
    th, ts = T(hr.copy()), T(sr.copy())
    fov(None, ts, th, mn, hr.shape[1:], crop, k, s, eval_mode=False)
    out.update({"c2_mn": np.asarray(mn), "c2_crop": np.asarray(crop), "c2_hr_drawn": th.numpy(), "c2_sr_drawn": ts.numpy()})
    assert not np.array_equal(th.numpy(), hr)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
