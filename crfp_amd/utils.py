"""Host-side mirror of the metric functions of the reference's ``utils`` module that sit on the eval path
(utils.py:166-185 psnr_cuda, :187-240 ssim, :242-254 calc_psnr_and_ssim_cuda, :328-330 bgr2ycbcr(y_only)),
computed by libcrfp_hip.so (crfp_psnr_ssim_partial_f32: one pass over the image pair gives both figures), and of the video rig's
foveated_metric (test_video.py:23-98; crfp_window_scores_f32: both score maps from one fused kernel, no unfold).
Same names, argument meaning and quirks; CUDA/HIP tensors only (no CPU path in the product)."""
from __future__ import annotations

import math

import torch

from . import _lib
from .ops import _dev, _stream


def _mask_bytes(mask, n, h, w, device):
    """[n,1,h,w] (or broadcastable) bool / float mask -> contiguous uint8, None for 'all ones'."""
    if mask is None:
        return None
    m = mask.to(device)
    if m.dtype != torch.bool:
        m = m != 0
    return m.expand(n, 1, h, w).contiguous().view(torch.uint8)


def psnr_ssim_sums(a, b, mask=None, mul=1.0, add=0.0):
    """float64 tensor (sum m*(a'-b')^2 over channels, sum m*SSIM_map over channels, sum m) with x' = x*mul + add."""
    a, b = _dev(a, "a"), _dev(b, "b")
    n, c, h, w = a.shape
    if tuple(b.shape) != (n, c, h, w):
        raise ValueError(f"shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    m8 = _mask_bytes(mask, n, h, w, a.device)
    acc = torch.zeros(3, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().crfp_psnr_ssim_partial_f32(a.data_ptr(), b.data_ptr(), None if m8 is None else m8.data_ptr(),
                                                         acc.data_ptr(), n, c, h, w, float(mul), float(add), _stream()),
                   "crfp_psnr_ssim_partial_f32")
    return acc


def _psnr_from(se, msum, shape):
    C = shape[1]
    mse = se / (msum * C)
    if mse == 0:   # utils.py:177-179
        return -20 * math.log10(math.sqrt((1 / 255.) ** 2 / float(torch.prod(torch.tensor(shape)))))
    return -20 * math.log10(math.sqrt(mse))


def psnr_cuda(img1, img2, mask, batch_avg=False):
    """utils.psnr_cuda, batch_avg=False branch.  Image range [0, 1]."""
    if batch_avg:
        raise NotImplementedError("batch_avg=True is a training-time branch of the reference (not on the eval path)")
    se, _, ms = (float(v) for v in psnr_ssim_sums(img1, img2, mask))
    return torch.tensor(_psnr_from(se, ms, tuple(img1.shape)))


def ssim_cuda(img1, img2, mask, batch_avg=False):
    """utils.ssim_cuda: masked mean of the 11x11-gaussian SSIM map.  Image range [0, 1]."""
    if batch_avg:
        raise NotImplementedError("batch_avg=True is a training-time branch of the reference (not on the eval path)")
    _, ss, ms = (float(v) for v in psnr_ssim_sums(img1, img2, mask))
    return torch.tensor(ss / (ms * img1.shape[1]))


def calc_psnr_and_ssim_cuda(sr, hr, mask, is_tensor=True, batch_avg=False):
    """utils.calc_psnr_and_ssim_cuda: range conversion chosen from hr's span (> 2: /255; > 1: (x+1)/2), then both."""
    if batch_avg:
        raise NotImplementedError("batch_avg=True is a training-time branch of the reference (not on the eval path)")
    sr, hr = _dev(sr, "sr"), _dev(hr, "hr")
    span = float(hr.max() - hr.min())
    mul, add = (1.0 / 255.0, 0.0) if span > 2 else ((0.5, 0.5) if span > 1 else (1.0, 0.0))
    se, ss, ms = (float(v) for v in psnr_ssim_sums(sr, hr, mask, mul, add))
    return torch.tensor(_psnr_from(se, ms, tuple(sr.shape))), torch.tensor(ss / (ms * sr.shape[1]))


def calc_psnr_and_ssim_regions(sr, hr, masks):
    """calc_psnr_and_ssim_cuda(sr, hr, m) for every mask m of one frame (the video rig's whole / fovea / outskirt / past
    regions, test_video.py:360-370) with ONE range probe and ONE host synchronisation instead of one per region; same
    kernel, same numbers.  Returns a list of (psnr, ssim) tensors."""
    sr, hr = _dev(sr, "sr"), _dev(hr, "hr")
    span = float(hr.max() - hr.min())
    mul, add = (1.0 / 255.0, 0.0) if span > 2 else ((0.5, 0.5) if span > 1 else (1.0, 0.0))
    sums = torch.stack([psnr_ssim_sums(sr, hr, m, mul, add).clone() for m in masks]).cpu()
    out = []
    for se, ss, ms in sums.tolist():
        out.append((torch.tensor(_psnr_from(se, ms, tuple(sr.shape))), torch.tensor(ss / (ms * sr.shape[1]))))
    return out


def frame_metrics_table(sr, hr, masks=None, luma=False):
    """float64 device tensor [n, 1+m, 4] = (PSNR, SSIM, PSNR-Y, SSIM-Y) of every frame of sr / hr [n,C,H,W] for the whole frame (row 0)
    and each of m <= 7 region masks (rows 1..m), from one fused pass over the batch (crfp_frame_metrics_f32): what
    calc_psnr_and_ssim_cuda(sr[i:i+1], hr[i:i+1], mask) gives per frame and region and, with luma (C == 3), the same on
    bgr2ycbcr(y_only=True) of both images, each with its own range conversion, both picked on the device.  masks: None, a list of m
    tensors broadcastable to [n,1,H,W], or one [n,m,H,W] tensor (bool, or non-zero = inside).  An empty region is NaN in its row (the
    per-region functions divide by zero there); without luma columns 2 and 3 are NaN.  The call does not synchronise."""
    sr, hr = _dev(sr, "sr"), _dev(hr, "hr")
    if sr.dim() != 4 or sr.shape != hr.shape:
        raise ValueError(f"sr / hr must be [n,C,H,W] of one shape, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    n, c, h, w = sr.shape
    if masks is None:
        m, m8 = 0, None
    else:
        if torch.is_tensor(masks):
            if masks.dim() != 4 or masks.shape[0] != n or tuple(masks.shape[2:]) != (h, w):
                raise ValueError(f"masks must be [n,m,H,W] = [{n},m,{h},{w}], got {tuple(masks.shape)}")
            mm = masks.to(sr.device)
        else:
            mm = [k.to(sr.device) for k in masks]
            mm = torch.cat([(k if k.dtype == torch.bool else k != 0).expand(n, 1, h, w) for k in mm], 1) if mm else None
        m = 0 if mm is None else mm.shape[1]
        m8 = None if m == 0 else (mm if mm.dtype == torch.bool else mm != 0).contiguous().view(torch.uint8)
    L = _lib.lib()
    out = torch.empty((n, 1 + m, 4), dtype=torch.float64, device=sr.device)
    ws_bytes = L.crfp_frame_metrics_workspace_bytes(n, m, h, w)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=sr.device)
    with torch.cuda.device(sr.device):
        _lib.check(L.crfp_frame_metrics_f32(sr.data_ptr(), hr.data_ptr(), None if m8 is None else m8.data_ptr(), out.data_ptr(), n, c, m, h, w,
                                            _lib.METRICS_LUMA if luma else 0, ws.data_ptr(), ws_bytes, _stream()), "crfp_frame_metrics_f32")
    return out


def window_scores(sr, hr, kernel_size=10, stride=5):
    """Raw per-window (psnr [dB], ssim) maps, [Hr,Wr] for [C,H,W] input and [n,Hr,Wr] for [n,C,H,W], of every kernel_size x
    kernel_size window at `stride`, each window scored as an image of its own (zero padding at the window's border).  The range
    conversion is picked on the device from sr's span over the covered pixels, per image; the call does not synchronise."""
    sr, hr = _dev(sr, "sr"), _dev(hr, "hr")
    if sr.dim() not in (3, 4) or sr.shape != hr.shape:
        raise ValueError(f"sr / hr must be [C,H,W] or [n,C,H,W] of one shape, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    n, (c, h, w) = (1 if sr.dim() == 3 else sr.shape[0]), sr.shape[-3:]
    k, s = int(kernel_size), int(stride)
    if k < 1 or s < 1 or k > h or k > w:
        raise ValueError(f"window {k} at stride {s} does not fit a {h} x {w} image")
    hr_, wr_ = (h - k) // s + 1, (w - k) // s + 1
    psnr = torch.empty((n, hr_, wr_), dtype=torch.float32, device=sr.device)
    ssim = torch.empty_like(psnr)
    L = _lib.lib()
    ws_bytes = L.crfp_window_scores_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=sr.device)
    with torch.cuda.device(sr.device):
        _lib.check(L.crfp_window_scores_f32(hr.data_ptr(), sr.data_ptr(), psnr.data_ptr(), ssim.data_ptr(), n, c, h, w, k, s,
                                            ws.data_ptr(), ws_bytes, _stream()), "crfp_window_scores_f32")
    return (psnr[0], ssim[0]) if sr.dim() == 3 else (psnr, ssim)


def foveated_metric(LR, LR_fv, HR, mn, hw, crop, kernel_size, stride_size, eval_mode=False):
    """test_video.foveated_metric: (psnr/100, (ssim.clip(0,1) - 0.7)/0.3, (psnr.min, psnr.max), (ssim.min, ssim.max)) of the per-window
    maps of LR_fv (the model output) against HR, both [3,H,W]; unless eval_mode, the crop rectangle at mn is then drawn into HR and
    LR_fv in place with the colour [0, 0, 255], as the reference does.  LR is unused there too.  Everything stays on the device."""
    if LR_fv.dim() != 3 or LR_fv.shape[0] != 3:
        raise ValueError(f"foveated_metric needs [3,H,W] images (the reference's .view(.., 3, k, k)), got {tuple(LR_fv.shape)}")
    psnr_score, ssim_score = window_scores(LR_fv, HR, kernel_size, stride_size)
    if not eval_mode:
        (m, n), (crop_h, crop_w) = mn, crop
        colour = torch.tensor([0., 0., 255.], device=HR.device).unsqueeze(1)
        for img in (HR, LR_fv):
            img[:, m:m + crop_h, n] = colour
            img[:, m:m + crop_h, n + crop_w - 1] = colour
            img[:, m, n:n + crop_w] = colour
            img[:, m + crop_h - 1, n:n + crop_w] = colour
    extrema = (psnr_score.min(), psnr_score.max()), (ssim_score.min(), ssim_score.max())
    return (psnr_score / 100, (ssim_score.clip(0, 1) - 0.7) / 0.3) + extrema


def bgr2ycbcr(img, y_only=False):
    """utils.bgr2ycbcr on an [N,H,W,3] tensor (BGR weights applied to whatever channel order arrives, as the
    reference does, trainer.py:362-363)."""
    if y_only:
        out = torch.matmul(img, torch.tensor([24.966, 128.553, 65.481], device=img.device)) + 16.0
        return out.unsqueeze(3).permute(0, 3, 1, 2)
    out = torch.matmul(img, torch.tensor([[24.966, 112.0, -18.214], [128.553, -74.203, -93.786], [65.481, -37.797, 112.0]],
                                         device=img.device)) + torch.tensor([16, 128, 128], device=img.device)
    return out.permute(0, 3, 1, 2)
