#!/usr/bin/env python3
"""Device time of the flow_warp forward / backward and of the shared-offset DCNv2 forward + backward: device events around one call,
median / min / p90 of `calls` calls after a warm-up.  Information, not a gate.  One JSON line.

flow_warp, at the reference's two call shapes (1, 32, 360, 640) and (1, 4, 1440, 2560), through the C-ABI with every output
preallocated.  The flow is a smooth field (amplitude `amp` px: a few pixels, and a large motion beyond the window's halo) plus noise of
sigma 2 px.  Legs: forward; backward with both gradients, grad_x alone, grad_flow alone; the backward with the LDS window of grad_x on
the undisplaced tile (crfp_flow_warp_backward_window_f32, window = 0) against the product's placement at the tile displaced by its
centre flow.  Next to them the reference's own route on the same device in the same run: the reference's flow_warp formula through
F.grid_sample and torch.autograd.grad (ATen's grid_sampler_2d_backward), and the bytes the scatter of grad_x adds (4 bytes per valid
corner and channel) per second against the chip-wide rate of global float atomic adds, ~1.3 TB/s.

dcnv2_shared at (1, 4 -> 4, 1440, 2560), forward + backward of all five gradients under autograd: ops.dcnv2_shared on the compact
offset [1,2,h,w] / mask [1,1,h,w] against the route to the same gradients before the shared backward existed, ops.dcnv2 on the
9x-tiled tensors including the `repeat` and its backward; time and torch.cuda.max_memory_allocated above the leaves for both."""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crfp_amd import _lib, ops   # noqa: E402

ATOMIC_RATE = 1.3e12   # bytes/s of float atomic adds, chip-wide
calls, warm = 20, 3
dev = torch.device("cuda:0")
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731


def stats(t):
    t = sorted(t)
    return dict(median_us=round(t[len(t) // 2], 1), min_us=round(t[0], 1), p90_us=round(t[int(0.9 * (len(t) - 1))], 1))


def timed(fn, check_rc=True):
    for _ in range(warm):
        rc = fn()
        assert not check_rc or rc == 0, L.crfp_last_error_string()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        rc = fn()
        b.record()
        assert not check_rc or rc == 0, L.crfp_last_error_string()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) * 1e3 for a, b in ev])


def reference_flow_warp(x, flow, padding_mode="zeros"):
    """the reference's flow_warp (model/CRFP.py:90-130)"""
    n, c, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(0, h, device=x.device), torch.arange(0, w, device=x.device), indexing="ij")
    g = torch.stack((gx, gy), 2).to(x.dtype) + flow
    nx = 2.0 * g[..., 0] / max(w - 1, 1) - 1.0
    ny = 2.0 * g[..., 1] / max(h - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((nx, ny), dim=3), mode="bilinear", padding_mode=padding_mode, align_corners=True)


def make_flow(n, h, w, amp, g):
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, h, 1) / h
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, w) / w
    fx = amp * torch.sin(2 * math.pi * (yy + 0.5 * xx))
    fy = amp * torch.cos(2 * math.pi * (xx - 0.25 * yy))
    return (torch.stack((fx.expand(n, h, w), fy.expand(n, h, w)), 3) + 2.0 * torch.randn(n, h, w, 2, device=dev, generator=g)).contiguous()


def warp_atomic_bytes(flow, c, h, w):
    """4 bytes per valid corner of every sample, times the channels"""
    ix = torch.arange(w, device=dev).view(1, 1, w) + flow[..., 0]
    iy = torch.arange(h, device=dev).view(1, h, 1) + flow[..., 1]
    x0, y0 = torch.floor(ix), torch.floor(iy)
    cols = ((x0 >= 0) & (x0 <= w - 1)).long() + ((x0 + 1 >= 0) & (x0 + 1 <= w - 1)).long()
    rows = ((y0 >= 0) & (y0 <= h - 1)).long() + ((y0 + 1 >= 0) & (y0 + 1 <= h - 1)).long()
    return int((rows * cols).sum()) * c * 4


res = {"atomic_rate_guide_TBps": ATOMIC_RATE / 1e12, "calls": calls, "flow_warp": {}, "dcnv2_shared": {}}
for n, c, h, w in ((1, 32, 360, 640), (1, 4, 1440, 2560)):
    for amp in (4.0, 24.0):
        g = torch.Generator(device=dev).manual_seed(c + int(amp))
        x = torch.randn(n, c, h, w, device=dev, generator=g)
        go = torch.randn(n, c, h, w, device=dev, generator=g)
        flow = make_flow(n, h, w, amp, g)
        out, gx, gflow = torch.empty_like(x), torch.empty_like(x), torch.empty_like(flow)
        fws = torch.empty(max(L.crfp_flow_warp_workspace_bytes(n, c, h, w), 256), dtype=torch.uint8, device=dev)
        bws = torch.empty(L.crfp_flow_warp_backward_workspace_bytes(n, c, h, w), dtype=torch.uint8, device=dev)

        def fwd():
            return L.crfp_flow_warp_f32(p(x), p(flow), p(out), n, c, h, w, 0, p(fws), fws.numel(), s)

        def bwd(ox, oflow, window=1):
            return lambda: L.crfp_flow_warp_backward_window_f32(p(x), p(flow), p(go), p(ox), p(oflow), n, c, h, w, 0, window, p(bws), bws.numel(), s)

        xr, fr = x.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        ref_out = reference_flow_warp(xr, fr)
        ab = warp_atomic_bytes(flow, c, h, w)
        row = {"forward": timed(fwd), "backward_both": timed(bwd(gx, gflow)), "backward_grad_x_only": timed(bwd(gx, None)),
               "backward_grad_flow_only": timed(bwd(None, gflow)),
               "backward_both_window_on_tile": timed(bwd(gx, gflow, 0)), "backward_grad_x_only_window_on_tile": timed(bwd(gx, None, 0)),
               "aten_forward": timed(lambda: reference_flow_warp(x, flow), False),
               "aten_backward_both": timed(lambda: torch.autograd.grad(ref_out, (xr, fr), go, retain_graph=True), False),
               "aten_backward_grad_x_only": timed(lambda: torch.autograd.grad(ref_out, (xr,), go, retain_graph=True), False),
               "atomic_bytes_per_call": ab, "atomic_floor_us_at_guide_rate": round(ab / ATOMIC_RATE * 1e6, 1)}
        ref_gx, ref_gflow = torch.autograd.grad(ref_out, (xr, fr), go, retain_graph=True)
        assert bwd(gx, gflow)() == 0
        torch.cuda.synchronize()
        row["max_abs_diff_to_aten"] = {"grad_x": float((gx - ref_gx).abs().max()), "grad_x_max": float(ref_gx.abs().max()),
                                       "grad_flow_median_abs_diff": float((gflow - ref_gflow).abs().median())}
        for leg in ("backward_both", "backward_grad_x_only", "backward_grad_x_only_window_on_tile"):
            row[leg]["atomic_TBps"] = round(ab / (row[leg]["median_us"] * 1e-6) / 1e12, 3)
        row["backward_over_aten"] = round(row["backward_both"]["median_us"] / row["aten_backward_both"]["median_us"], 3)
        row["displaced_over_on_tile"] = round(row["backward_both"]["median_us"] / row["backward_both_window_on_tile"]["median_us"], 3)
        res["flow_warp"][f"{n}x{c}_{h}x{w}_amp{int(amp)}"] = row
        del xr, fr, ref_out, ref_gx, ref_gflow

# ---- dcnv2_shared: the compact route against the tiled one, forward + backward of all five gradients under autograd
n, h, w = 1, 1440, 2560
g = torch.Generator(device=dev).manual_seed(4)
leaves = dict(x=torch.randn(n, 4, h, w, device=dev, generator=g), offset=torch.randn(n, 2, h, w, device=dev, generator=g) * 2.0,
              mask=torch.rand(n, 1, h, w, device=dev, generator=g), weight=torch.randn(4, 4, 3, 3, device=dev, generator=g) * 0.1,
              bias=torch.zeros(4, device=dev))
go = torch.randn(n, 4, h, w, device=dev, generator=g)
for t in leaves.values():
    t.requires_grad_(True)


def compact():
    out = ops.dcnv2_shared(*leaves.values())
    return torch.autograd.grad(out, list(leaves.values()), go)


def tiled():
    out = ops.dcnv2(leaves["x"], leaves["offset"].repeat(1, 9, 1, 1), leaves["mask"].repeat(1, 9, 1, 1), leaves["weight"], leaves["bias"], 3, 1, 1, 1)
    return torch.autograd.grad(out, list(leaves.values()), go)


row = {}
for name, fn in (("compact", compact), ("tiled", tiled)):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    grads = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    row[name] = timed(fn, False)
    row[name]["peak_bytes_above_leaves"] = peak
    row[name + "_grads"] = [t.clone() for t in grads]
    del grads
row["max_abs_diff_compact_to_tiled"] = {k: float((a - b).abs().max()) for k, a, b in zip(leaves, row.pop("compact_grads"), row.pop("tiled_grads"))}
row["compact_over_tiled_time"] = round(row["compact"]["median_us"] / row["tiled"]["median_us"], 3)
row["tiled_spread_us_p90_minus_min"] = round(row["tiled"]["p90_us"] - row["tiled"]["min_us"], 1)
row["compact_over_tiled_peak"] = round(row["compact"]["peak_bytes_above_leaves"] / row["tiled"]["peak_bytes_above_leaves"], 3)
row["tiled_operand_bytes"] = 27 * h * w * 4
res["dcnv2_shared"][f"{n}x4->4_{h}x{w}"] = row
print(json.dumps(res))
