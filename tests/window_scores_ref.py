"""Restatement of the foveated score maps (the reference's video rig, test_video.py:23-63 foveated_metric -> the batch_avg=True
branches of utils.py:166-172,197-221,242-254), written from the formula and not from the reference's unfold + convolution code:

  window (i, j) of size k at stride s covers rows i*s .. i*s+k-1, columns j*s .. j*s+k-1 of every channel;
  range conversion from the span of `sr` over the covered pixels (> 2: x/255, > 1: (x+1)/2);
  mse = mean over the C*k*k elements of (a-b)^2;  psnr = -20 log10(sqrt(mse)), or -20 log10(sqrt((1/255)^2 / (C k k))) when mse == 0;
  each k x k patch filtered along both axes with the weight g[q-p+5] between positions p and q when |q-p| <= 5, else 0 (g: the 11-tap
  sigma-1.5 gaussian, float32 weights normalised by their float32 sum) -- a zero-padded patch, nothing from outside the window;
  ssim = mean over the C*k*k positions of ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), C1 = 0.01^2, C2 = 0.03^2.

`window_scores` evaluates it in the dtype asked for (float64 = the yardstick of the GPU tests).  `window_scores_unfold` is the
composition a PyTorch user would write (F.unfold of both images, five grouped 11 x 11 convolutions over the patches): the thing the
fused kernel is timed against, on whatever device its inputs live.  Test infrastructure only."""
import math

import torch
import torch.nn.functional as F


def gaussian11(dtype=torch.float64):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return (g / g.sum()).to(dtype)


def filter_axis(X, dim, dtype):
    """out[p] = sum_q g[q-p+5] X[q] over the q of the patch with |q-p| <= 5, along `dim`; taps added in the order d = -5 .. 5
    with elementwise operations only (no BLAS), so that the float64 result does not depend on the machine."""
    g = gaussian11(dtype)
    k = X.shape[dim]
    out = torch.zeros_like(X)
    for d in range(-5, 6):
        if abs(d) >= k:
            continue
        dst = out.narrow(dim, max(0, -d), k - abs(d))
        dst += g[d + 5] * X.narrow(dim, max(0, d), k - abs(d))
    return out


def ordered_mean(X):
    """[C, Hr, Wr, k, k] -> [Hr, Wr]: the C*k*k elements added one after the other (same reason)."""
    C, Hr, Wr, k, _ = X.shape
    flat = X.permute(0, 3, 4, 1, 2).reshape(C * k * k, Hr, Wr)
    acc = torch.zeros(Hr, Wr, dtype=X.dtype, device=X.device)
    for v in flat:
        acc = acc + v
    return acc / (C * k * k)


def map_size(h, w, k, s):
    return (h - k) // s + 1, (w - k) // s + 1


def convert_range(hr, sr, k, s):
    """The conversion the span of sr's covered pixels selects, applied to both [.., C, H, W] images of ONE frame."""
    Hr, Wr = map_size(hr.shape[-2], hr.shape[-1], k, s)
    cov = sr[..., :(Hr - 1) * s + k, :(Wr - 1) * s + k]
    span = cov.max() - cov.min()
    if span > 2:
        return hr / 255.0, sr / 255.0
    if span > 1:
        return (hr + 1.0) / 2.0, (sr + 1.0) / 2.0
    return hr, sr


def floor_psnr(c, k):
    return -20.0 * math.log10(math.sqrt((1 / 255.0) ** 2 / (c * k * k)))


def window_scores(hr, sr, k=10, s=5, dtype=torch.float64):
    """hr, sr: [C,H,W] (or [n,C,H,W], every frame on its own) -> raw (psnr [Hr,Wr] dB, ssim [Hr,Wr]) in `dtype`."""
    if hr.dim() == 4:
        both = [window_scores(a, b, k, s, dtype) for a, b in zip(hr, sr)]
        return torch.stack([p for p, _ in both]), torch.stack([q for _, q in both])
    a, b = convert_range(hr.to(dtype), sr.to(dtype), k, s)
    C = a.shape[0]
    A = a.unfold(1, k, s).unfold(2, k, s)   # [C, Hr, Wr, k, k] views of the windows
    B = b.unfold(1, k, s).unfold(2, k, s)
    mse = ordered_mean((A - B) ** 2)
    psnr = torch.where(mse == 0, torch.full_like(mse, floor_psnr(C, k)), -20.0 * torch.log10(torch.sqrt(mse)))
    filt = lambda X: filter_axis(filter_axis(X, 4, dtype), 3, dtype)   # noqa: E731  rows, then columns, of the zero-padded patch
    mu1, mu2 = filt(A), filt(B)
    s1, s2, s12 = filt(A * A) - mu1 * mu1, filt(B * B) - mu2 * mu2, filt(A * B) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return psnr, ordered_mean(smap)


def window_scores_unfold(hr, sr, k=10, s=5):
    """The unfused composition in the inputs' dtype on the inputs' device: unfold both [C,H,W] images into [Hr*Wr, C, k, k]
    patches, five grouped 11 x 11 convolutions (padding 5), the map, the two means."""
    a, b = convert_range(hr, sr, k, s)
    C, H, W = a.shape
    Hr, Wr = map_size(H, W, k, s)
    pa = F.unfold(a[None], kernel_size=k, stride=s).permute(0, 2, 1).reshape(Hr * Wr, C, k, k)
    pb = F.unfold(b[None], kernel_size=k, stride=s).permute(0, 2, 1).reshape(Hr * Wr, C, k, k)
    mse = ((pa - pb) ** 2).reshape(Hr * Wr, -1).mean(1)
    floor = torch.full_like(mse, floor_psnr(C, k))
    psnr = torch.where(mse == 0, floor, -20.0 * torch.log10(torch.sqrt(mse)))
    g = gaussian11(a.dtype).to(a.device)
    win = (g[:, None] * g[None, :]).expand(C, 1, 11, 11).contiguous()
    conv = lambda x: F.conv2d(x, win, padding=5, groups=C)   # noqa: E731
    mu1, mu2 = conv(pa), conv(pb)
    s1, s2, s12 = conv(pa * pa) - mu1 * mu1, conv(pb * pb) - mu2 * mu2, conv(pa * pb) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return psnr.view(Hr, Wr), smap.reshape(Hr * Wr, -1).mean(1).view(Hr, Wr)
