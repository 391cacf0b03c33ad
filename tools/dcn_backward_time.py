#!/usr/bin/env python3
"""Device time of the DCNv2 forward and backward at the reference's two call shapes, (1, 32 -> 32, dg 8, 360 x 640) and
(1, 4 -> 4, dg 1, 1440 x 2560), through the C-ABI with every output preallocated: device events around one call, median / min / p90 of
`calls` calls after a warm-up.  Offsets are normal with sigma 2 px.  Next to the backward time: the bytes the scatter of grad_x adds
(4 bytes per valid corner of every (channel, tap, pixel) sample, counted from the offsets) per second, against the chip-wide rate of
global float atomic adds, ~1.3 TB/s of added bytes.  The kernel sums them per workgroup in an LDS window first, so what reaches memory
as global atomics is at most `window_flush_bytes_max` (the windows of all workgroups, zeros skipped) plus the corners beyond a window's
halo.  The backward legs: all five gradients, grad_x alone (weight
transpose + pixel kernel), grad_weight / grad_bias alone (slab pass + slab sum).  Information, not a gate.  One JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crfp_amd import _lib   # noqa: E402

ATOMIC_RATE = 1.3e12   # bytes/s of float atomic adds, chip-wide
calls, warm = 20, 3
dev = torch.device("cuda:0")
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731


def atomic_bytes(offset, cin, dg, h, w):
    """4 bytes per valid corner of every sample, times the channels of its group"""
    off = offset.reshape(1, dg, 9, 2, h, w)
    k = torch.arange(9, device=dev)
    py = torch.arange(h, device=dev).view(1, 1, 1, h, 1) + (k // 3 - 1).view(1, 1, 9, 1, 1) + off[:, :, :, 0]
    px = torch.arange(w, device=dev).view(1, 1, 1, 1, w) + (k % 3 - 1).view(1, 1, 9, 1, 1) + off[:, :, :, 1]
    inside = (py > -1) & (py < h) & (px > -1) & (px < w)
    y0, x0 = torch.floor(py), torch.floor(px)
    rows = ((y0 >= 0) & (y0 <= h - 1)).long() + ((y0 + 1 >= 0) & (y0 + 1 <= h - 1)).long()
    cols = ((x0 >= 0) & (x0 <= w - 1)).long() + ((x0 + 1 >= 0) & (x0 + 1 <= w - 1)).long()
    return int((rows * cols * inside).sum()) * (cin // dg) * 4


def timed(fn):
    for _ in range(warm):
        assert fn() == 0, L.crfp_last_error_string()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        rc = fn()
        b.record()
        assert rc == 0, L.crfp_last_error_string()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return dict(median_us=round(t[len(t) // 2], 1), min_us=round(t[0], 1), p90_us=round(t[int(0.9 * (len(t) - 1))], 1))


res = {"atomic_rate_guide_TBps": ATOMIC_RATE / 1e12, "calls": calls, "shapes": {}}
for n, cin, cout, dg, h, w in ((1, 32, 32, 8, 360, 640), (1, 4, 4, 1, 1440, 2560)):
    g = torch.Generator(device=dev).manual_seed(cin)
    x = torch.randn(n, cin, h, w, device=dev, generator=g)
    offset = torch.randn(n, 2 * dg * 9, h, w, device=dev, generator=g) * 2.0
    mask = torch.rand(n, dg * 9, h, w, device=dev, generator=g)
    weight = torch.randn(cout, cin, 3, 3, device=dev, generator=g) * 0.1
    bias = torch.zeros(cout, device=dev)
    go = torch.randn(n, cout, h, w, device=dev, generator=g)
    out = torch.empty_like(go)
    gx, goff, gm, gw, gb = (torch.empty_like(t) for t in (x, offset, mask, weight, bias))
    fws = torch.empty(max(L.crfp_dcnv2_workspace_bytes(n, cin, cout, h, w, 3, dg), 256), dtype=torch.uint8, device=dev)
    bws = torch.empty(L.crfp_dcnv2_backward_workspace_bytes(n, cin, cout, h, w, 3, dg), dtype=torch.uint8, device=dev)

    def fwd():
        return L.crfp_dcnv2_forward_f32(p(x), p(offset), p(mask), p(weight), p(bias), p(out), n, cin, cout, h, w, 3, 1, 1, dg, p(fws), fws.numel(), s)

    def bwd(*outs):
        return lambda: L.crfp_dcnv2_backward_f32(p(x), p(offset), p(mask), p(weight), p(go), *(p(o) for o in outs), n, cin, cout, h, w, 3, 1, 1, dg,
                                                 p(bws), bws.numel(), s)

    ab = atomic_bytes(offset, cin, dg, h, w)
    row = {"forward": timed(fwd), "backward_all": timed(bwd(gx, goff, gm, gw, gb)), "backward_grad_x_only": timed(bwd(gx, None, None, None, None)),
           "backward_offset_mask_only": timed(bwd(None, goff, gm, None, None)), "backward_weight_bias_only": timed(bwd(None, None, None, gw, gb)),
           "atomic_bytes_per_call": ab, "backward_workspace_bytes": bws.numel()}
    for leg in ("backward_all", "backward_grad_x_only"):
        row[leg]["atomic_TBps"] = round(ab / (row[leg]["median_us"] * 1e-6) / 1e12, 3)
        row[leg]["share_of_guide_rate"] = round(row[leg]["atomic_TBps"] / (ATOMIC_RATE / 1e12), 3)
    row["window_flush_bytes_max"] = n * cin * ((h + 3) // 4) * ((w + 63) // 64) * 20 * 80 * 4
    row["atomic_floor_us_at_guide_rate"] = round(ab / ATOMIC_RATE * 1e6, 1)
    res["shapes"][f"{n}x{cin}->{cout}_dg{dg}_{h}x{w}"] = row
print(json.dumps(res))
