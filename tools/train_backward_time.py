#!/usr/bin/env python3
"""Device time of the training backward kernels (csrc/train_backward.hip) against ATen's autograd on the same device in the same run, at
the shapes of the headline configuration (180 x 320 -> 1440 x 2560, 7 frames): device events around one call, median / min / p90 of
`calls` calls after a warm-up.  Information, not a gate.  One JSON line.

Ours: the C-ABI with every output preallocated.  ATen: torch.autograd.grad through F.interpolate(bilinear, align_corners=False) (* mul),
F.avg_pool2d(2, 2) and the torch-composed Charbonnier loss, graph retained between calls.  The loss legs time forward + backward and
record the peak memory above the leaves (torch.cuda.max_memory_allocated).  Last: one CRFP_DSV.forward_train + loss + backward step."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crfp_amd import _lib, synth   # noqa: E402
from crfp_amd.loss import charbonnier_loss   # noqa: E402

calls, warm = 20, 3
dev = torch.device("cuda:0")
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream

RESIZE = (("flow_x8", 1, 2, 180, 320, 8, 8.0), ("flow_x2", 1, 2, 180, 320, 2, 2.0), ("fnet_decoder3_x2", 6, 64, 88, 160, 2, 1.0),
          ("fnet_tail_176_to_180", 6, 2, 176, 320, (180, 320), 1.0))
POOL = (("fnet_encoder1", 6, 32, 180, 320), ("fnet_encoder3", 6, 128, 45, 80))
LOSS = (("7x3x1440x2560", 7, 3, 1440, 2560, 0), ("7x3x1440x2560_mask", 7, 3, 1440, 2560, 1))


def stats(t):
    t = sorted(t)
    return dict(median_us=round(t[len(t) // 2], 1), min_us=round(t[0], 1), p90_us=round(t[int(0.9 * (len(t) - 1))], 1))


def timed(fn, check_rc=True, n=calls):
    for _ in range(warm):
        rc = fn()
        assert not check_rc or rc == 0, L.crfp_last_error_string()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        rc = fn()
        b.record()
        assert not check_rc or rc == 0, L.crfp_last_error_string()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) * 1e3 for a, b in ev])


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


res = {"calls": calls, "upsample_bilinear_backward": {}, "avgpool2_backward": {}, "charbonnier": {}}
for tag, n, c, h, w, to, mul in RESIZE:
    g = torch.Generator(device=dev).manual_seed(h + c)
    x = torch.randn(n, c, h, w, device=dev, generator=g).requires_grad_(True)
    if isinstance(to, tuple):
        (oh, ow), sh, sw = to, float(torch.tensor(float(h)) / torch.tensor(float(to[0]))), float(torch.tensor(float(w)) / torch.tensor(float(to[1])))
        y = F.interpolate(x, size=to, mode="bilinear", align_corners=False) * mul
    else:
        oh, ow, sh, sw = h * to, w * to, 1.0 / to, 1.0 / to
        y = F.interpolate(x, scale_factor=to, mode="bilinear", align_corners=False) * mul
    go = torch.randn(n, c, oh, ow, device=dev, generator=g)
    gx = torch.empty(n, c, h, w, device=dev)
    ours = lambda: L.crfp_upsample_bilinear_backward_f32(go.data_ptr(), gx.data_ptr(), n, c, h, w, oh, ow, sh, sw, mul, s)   # noqa: E731
    row = {"backward": timed(ours), "aten_backward": timed(lambda: torch.autograd.grad(y, x, go, retain_graph=True), False)}
    row["over_aten"] = round(row["backward"]["median_us"] / row["aten_backward"]["median_us"], 3)
    row["max_abs_diff_to_aten_over_max"] = rel(gx, torch.autograd.grad(y, x, go, retain_graph=True)[0])
    row["bytes_moved"] = 4 * n * c * (h * w + oh * ow)
    res["upsample_bilinear_backward"][f"{tag}_{n}x{c}x{h}x{w}->{oh}x{ow}"] = row
    del y

for tag, n, c, h, w in POOL:
    g = torch.Generator(device=dev).manual_seed(h + c)
    x = torch.randn(n, c, h, w, device=dev, generator=g).requires_grad_(True)
    y = F.avg_pool2d(x, 2, 2)
    go = torch.randn(y.shape, device=dev, generator=g)
    gx = torch.empty(n, c, h, w, device=dev)
    row = {"backward": timed(lambda: L.crfp_avgpool2_backward_f32(go.data_ptr(), gx.data_ptr(), n, c, h, w, s)),
           "aten_backward": timed(lambda: torch.autograd.grad(y, x, go, retain_graph=True), False)}
    row["over_aten"] = round(row["backward"]["median_us"] / row["aten_backward"]["median_us"], 3)
    row["max_abs_diff_to_aten_over_max"] = rel(gx, torch.autograd.grad(y, x, go, retain_graph=True)[0])
    res["avgpool2_backward"][f"{tag}_{n}x{c}x{h}x{w}"] = row
    del y


def composed(pred, target, weight):
    """loss/loss.py composed from torch elementwise ops (mean; masked mean with a weight)"""
    loss = torch.sqrt((pred - target) ** 2 + 1e-12)
    if weight is None:
        return loss.mean()
    loss = loss * weight
    return loss.sum() / (weight.expand_as(loss).sum() + 1e-12)


for tag, n, c, h, w, wc in LOSS:
    g = torch.Generator(device=dev).manual_seed(wc)
    pred = torch.rand(n, c, h, w, device=dev, generator=g).requires_grad_(True)
    target = torch.rand(n, c, h, w, device=dev, generator=g)
    weight = (torch.rand(n, 1, h, w, device=dev, generator=g) < 0.6).float() if wc else None
    row = {}
    for name, fn in (("fused", lambda: charbonnier_loss(pred, target, weight)), ("composed", lambda: composed(pred, target, weight))):
        def step():
            pred.grad = None
            fn().backward()
        row[f"{name}_forward_backward"] = timed(step, False)
        pred.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        row[f"{name}_peak_bytes_above_leaves"] = torch.cuda.max_memory_allocated() - base
        row[f"{name}_loss"] = float(fn().detach())
        row[f"{name}_grad"] = pred.grad.clone()
    row["fused_over_composed"] = round(row["fused_forward_backward"]["median_us"] / row["composed_forward_backward"]["median_us"], 3)
    row["grad_max_abs_diff_over_max"] = rel(row.pop("fused_grad"), row.pop("composed_grad"))
    row["tensor_bytes"] = 4 * n * c * h * w
    res["charbonnier"][tag] = row
    del pred, target, weight

# one training step of the model at the headline shape: forward_train + Charbonnier mean + backward (no optimizer)
from crfp_amd.model.CRFP import CRFP_DSV   # noqa: E402
model = CRFP_DSV(dev, mid_channels=32)
model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(0, 32).items()}, strict=True)
model.to(dev)
lrs, fvs, mks, hrs = (torch.from_numpy(a).to(dev) for a in synth.make_clip_hr(1, 1, 7, 180, 320))


def train_step():
    model.zero_grad(set_to_none=True)
    out = model.forward_train(lrs, fvs, mks)
    charbonnier_loss(out.view(-1, 3, 1440, 2560), hrs.view(-1, 3, 1440, 2560)).backward()


calls_step, warm = 5, 2
row = {"forward_train_loss_backward": timed(train_step, False, calls_step), "calls": calls_step}
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
train_step()
torch.cuda.synchronize()
row["peak_bytes_above_resident"] = torch.cuda.max_memory_allocated() - base
with torch.no_grad():
    row["forward_train_no_grad"] = timed(lambda: model.forward_train(lrs, fvs, mks) is None, False, calls_step)
    model.trainable = False
    row["engine_forward"] = timed(lambda: model(lrs, fvs, mks) is None, False, calls_step)
res["crfp_dsv_mid32_1x7x180x320"] = row
print(json.dumps(res))
