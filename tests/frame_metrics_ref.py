"""Float64 torch-CPU restatement of the frame metrics table (crfp_frame_metrics_f32 / crfp_amd.utils.frame_metrics_table): the yardstick
of tests/test_gpu_frame_metrics.py, itself pinned against the reference-generated values of tests/golden/ops_small.npz and the fp32
oracle by tests/test_frame_metrics.py.

Per frame, and per region (row 0 = the whole frame, rows 1..m = the masks, non-zero = inside):
  PSNR, SSIM      utils.calc_psnr_and_ssim_cuda(sr, hr, mask): conversion from hr's span (> 2: /255; > 1: (x+1)/2; else none, also for a
                  NaN span), mse = sum m (a-b)^2 / (sum m * C), PSNR = -20 log10 sqrt(mse) or, when mse == 0, the floor
                  -20 log10 sqrt((1/255)^2 / (C H W)); SSIM = sum m S / (sum m * C), S the map of the zero-padded 121-tap gaussian window
                  (the reference's float32 weights, C1 = 0.01^2, C2 = 0.03^2)
  PSNR-Y, SSIM-Y  the same on luma = 24.966 c0 + 128.553 c1 + 65.481 c2 + 16 (the reference's float32 weights) of both images, converted
                  by the span of luma(hr); NaN when luma is off
An empty region is NaN in all four columns (the reference divides by zero there)."""
import math

import torch
import torch.nn.functional as F

NAN = float("nan")


def window(dtype=torch.float64):
    """utils.gaussian / create_window: float32 taps normalised by their float32 sum, outer product in float32; [1,1,11,11]."""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().to(dtype)[None, None]


def luma(x):
    """[n,3,H,W] -> [n,1,H,W] in x's dtype, the reference's float32 weights."""
    w = torch.tensor([24.966, 128.553, 65.481]).to(x.dtype).view(1, 3, 1, 1)
    return (x * w).sum(1, keepdim=True) + 16.0


def convert(a, b):
    span = float(b.max() - b.min())
    if span > 2:
        return a / 255.0, b / 255.0
    if span > 1:
        return (a + 1.0) / 2.0, (b + 1.0) / 2.0
    return a, b


def ssim_map(a, b):
    """[1,C,H,W] -> the SSIM map, zero padding, per channel."""
    c = a.shape[1]
    w = window(a.dtype).expand(c, 1, 11, 11).contiguous()
    f = lambda x: F.conv2d(x, w, padding=5, groups=c)   # noqa: E731
    mu1, mu2 = f(a), f(b)
    s1, s2, s12 = f(a * a) - mu1 * mu1, f(b * b) - mu2 * mu2, f(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def _pair(a, b, regions):
    """(psnr, ssim) per region of one converted-or-not frame pair [1,C,H,W]."""
    a, b = convert(a, b)
    c, numel = a.shape[1], a.numel()
    se, S = ((a - b) ** 2).sum(1, keepdim=True), ssim_map(a, b).sum(1, keepdim=True)
    out = []
    for m in regions:
        msum = float(m.sum())
        if msum == 0:
            out.append((NAN, NAN))
            continue
        mse = float((se * m).sum()) / (msum * c)
        p = -20 * math.log10(math.sqrt((1 / 255.0) ** 2 / numel)) if mse == 0 else -20 * math.log10(math.sqrt(mse))
        out.append((p, float((S * m).sum()) / (msum * c)))
    return out


def table(sr, hr, masks=None, luma_on=False, dtype=torch.float64):
    """sr, hr [n,C,H,W]; masks None or [n,m,H,W]; -> float64 [n,1+m,4]."""
    n, c, h, w = sr.shape
    m = 0 if masks is None else masks.shape[1]
    out = torch.full((n, 1 + m, 4), NAN, dtype=torch.float64)
    for i in range(n):
        a, b = sr[i:i + 1].to(dtype), hr[i:i + 1].to(dtype)
        regions = [torch.ones(1, 1, h, w, dtype=dtype)] + [(masks[i:i + 1, k:k + 1] != 0).to(dtype) for k in range(m)]
        out[i, :, 0:2] = torch.tensor(_pair(a, b, regions), dtype=torch.float64)
        if luma_on:
            out[i, :, 2:4] = torch.tensor(_pair(luma(a), luma(b), regions), dtype=torch.float64)
    return out


# ---------------------------------------------------------------------------------------------------------------- shared cases
def ragged_case():
    """The GPU test's batch: n = 5 frames 3 x 70 x 150 (five tile rows, three tile columns, ragged both ways).  Frames 0-2: one uniform-
    noise pair (hr in [0.1, 0.85]: spans 0.75, 191 and 1.5, clear of the thresholds) scaled x1, x255, x2 - 1 (the three RGB
    branches).  Frames 3-4: hr confined to a width of 0.004 / 0.007, so that luma spans 0.88 / 1.53 (with frames 0-2, whose luma
    spans more than 160, the three luma branches).  m = 3: random masks of density 0.6 and
    0.1, and one rectangle crossing tile borders."""
    g = torch.Generator().manual_seed(77)
    h, w = 70, 150
    hr0 = 0.1 + 0.75 * torch.rand(3, h, w, generator=g)
    sr0 = (hr0 + 0.05 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    hr, sr = [hr0, hr0 * 255.0, hr0 * 2.0 - 1.0], [sr0, sr0 * 255.0, sr0 * 2.0 - 1.0]
    for width in (0.004, 0.007):
        b = 0.5 + width * torch.rand(3, h, w, generator=g)
        b[:, 0, 0], b[:, 0, 1] = 0.5, 0.5 + width          # the extremes are present in every channel: luma spans 219 x width
        hr.append(b)
        sr.append(b + 0.0005 * torch.randn(3, h, w, generator=g))
    masks = torch.zeros(5, 3, h, w, dtype=torch.bool)
    masks[:, 0] = torch.rand(5, h, w, generator=g) < 0.6
    masks[:, 1] = torch.rand(5, h, w, generator=g) < 0.1
    masks[:, 2, 9:41, 50:140] = True
    return torch.stack(sr).float().contiguous(), torch.stack(hr).float().contiguous(), masks


def small_cases():
    """(name, sr, hr) of the small and odd shapes: 1 x 7 x 9 (smaller than the filter), 3 x 16 x 64 (exactly one tile), 3 x 17 x 65."""
    g = torch.Generator().manual_seed(78)
    out = []
    for name, c, h, w in (("c1_7x9", 1, 7, 9), ("c3_16x64", 3, 16, 64), ("c3_17x65", 3, 17, 65)):
        hr = 0.1 + 0.75 * torch.rand(1, c, h, w, generator=g)   # span 0.75: clear of the conversion thresholds
        out.append((name, (hr + 0.03 * torch.randn(1, c, h, w, generator=g)).float(), hr.float()))
    return out


def oracle_table(orc, sr, hr, masks=None, luma_on=False):
    """The same table from the fp32 oracle (oracle.crfp_oracle: calc_psnr_and_ssim, to_y), frame by frame and region by region; an empty
    region stays NaN (the oracle divides by zero there)."""
    n, c, h, w = sr.shape
    m = 0 if masks is None else masks.shape[1]
    out = torch.full((n, 1 + m, 4), NAN, dtype=torch.float64)
    for i in range(n):
        a, b = sr[i:i + 1], hr[i:i + 1]
        if luma_on:
            ya, yb = orc.to_y(a.permute(0, 2, 3, 1)), orc.to_y(b.permute(0, 2, 3, 1))
        for k in range(1 + m):
            mk = torch.ones(1, 1, h, w) if k == 0 else (masks[i:i + 1, k - 1:k] != 0).float()
            if float(mk.sum()) == 0:
                continue
            out[i, k, 0:2] = torch.tensor(orc.calc_psnr_and_ssim(a, b, mk), dtype=torch.float64)
            if luma_on:
                out[i, k, 2:4] = torch.tensor(orc.calc_psnr_and_ssim(ya, yb, mk), dtype=torch.float64)
    return out


def bounds(yard, oracle):
    """The project's tolerance rule per figure: max(1e-4 dB or 2e-6 SSIM, 4 x |fp32 oracle - float64 yardstick|); [n,1+m,4]."""
    floor = torch.tensor([1e-4, 2e-6, 1e-4, 2e-6], dtype=torch.float64).expand_as(yard)
    return torch.maximum(floor, 4.0 * torch.nan_to_num((oracle - yard).abs(), nan=0.0))


def conditioning(sr, hr, luma_on=False):
    """kappa [n, 2] (RGB, luma): mean over pixels and channels of (mu1^2 + mu2^2) / (sigma1^2 + sigma2^2 + C2) on the converted pair --
    how much a relative rounding error of the filtered second moments is amplified in the SSIM map."""
    out = torch.zeros(sr.shape[0], 2, dtype=torch.float64)
    for i in range(sr.shape[0]):
        a, b = sr[i:i + 1].double(), hr[i:i + 1].double()
        for col, (x, y) in enumerate(((a, b), (luma(a), luma(b))) if luma_on else ((a, b),)):
            x, y = convert(x, y)
            c = x.shape[1]
            w = window().expand(c, 1, 11, 11).contiguous()
            f = lambda t: F.conv2d(t, w, padding=5, groups=c)   # noqa: E731
            mu1, mu2 = f(x), f(y)
            den = f(x * x) - mu1 * mu1 + f(y * y) - mu2 * mu2 + 0.03 ** 2
            out[i, col] = float(((mu1 * mu1 + mu2 * mu2) / den).mean())
    return out
