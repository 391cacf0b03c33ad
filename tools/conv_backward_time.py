#!/usr/bin/env python3
"""Device time of the conv3x3 backward (crfp_conv3x3_ex_backward_f32) against ATen's autograd of F.conv2d on the same device in the same
run: device events around one call, median / min / p90 of `calls` calls after a warm-up.  Information, not a gate.  One JSON line.

Ours: the C-ABI with every output and the workspace preallocated -- all gradients, the input gradients alone, grad_weight + grad_bias
alone.  ATen: torch.autograd.grad through the graph the reference composes, cat -> F.conv2d(padding=1) -> activation -> * s -> + residual
-> F.pixel_shuffle, retained between calls, for the same leaves (so its time covers the activation, cat and shuffle steps).  Shapes:
(1, 32+34 -> 32, lrelu, 360 x 640), (1, 32 -> 144, 10 tanh, 360 x 640), (1, 4+4 -> 4, none + residual, 1440 x 2560),
(1, 32 -> 64, shuffle 4, 360 x 640)."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crfp_amd import _lib, ops   # noqa: E402

calls, warm = 20, 3
dev = torch.device("cuda:0")
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731

SHAPES = (dict(cin=32, cin2=34, cout=32, act="lrelu", s=1.0, h=360, w=640),
          dict(cin=32, cin2=0, cout=144, act="tanh", s=10.0, h=360, w=640),
          dict(cin=4, cin2=4, cout=4, act="none", s=1.0, resid=True, h=1440, w=2560),
          dict(cin=32, cin2=0, cout=64, act="none", s=1.0, shuffle=4, h=360, w=640))


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


res = {"calls": calls, "conv3x3_backward": {}}
for c in SHAPES:
    n, cin, cin2, cout, h, w, r = 1, c["cin"], c["cin2"], c["cout"], c["h"], c["w"], c.get("shuffle", 0)
    g = torch.Generator(device=dev).manual_seed(cin + cout)
    x = torch.randn(n, cin, h, w, device=dev, generator=g)
    x2 = torch.randn(n, cin2, h, w, device=dev, generator=g) if cin2 else None
    weight = torch.randn(cout, cin + cin2, 3, 3, device=dev, generator=g) / (3.0 * (cin + cin2) ** 0.5)
    bias = torch.randn(cout, device=dev, generator=g) * 0.1
    resid = torch.randn(n, cout, h, w, device=dev, generator=g) if c.get("resid") else None
    leaves = [t.requires_grad_(True) for t in (x, x2, weight, bias, resid) if t is not None]
    z = F.conv2d(x if x2 is None else torch.cat([x, x2], 1), weight, bias, padding=1)
    y = {"none": lambda t: t, "lrelu": lambda t: F.leaky_relu(t, 0.1), "tanh": torch.tanh}[c["act"]](z) * c["s"]
    if resid is not None:
        y = y + resid
    if r:
        y = F.pixel_shuffle(y, r)
    go = torch.randn(y.shape, device=dev, generator=g)
    out = y.detach().contiguous()
    gx, gx2, gw, gb = torch.empty_like(x), None if x2 is None else torch.empty_like(x2), torch.empty_like(weight), torch.empty_like(bias)
    nb = L.crfp_conv3x3_ex_backward_workspace_bytes(n, cin, cin2, cout, h, w, 0, r)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def bwd(ox, ox2, ow, ob):
        return lambda: L.crfp_conv3x3_ex_backward_f32(p(x), cin, p(x2), cin2, p(weight), p(out), p(go), p(ox), p(ox2), p(ow), p(ob), n, cout, h, w,
                                                      ops.ACT[c["act"]], c["s"], 0, r, p(ws), nb, s)

    inputs = [t for t in (x, x2) if t is not None]
    row = {"backward_all": timed(bwd(gx, gx2, gw, gb)), "backward_inputs_only": timed(bwd(gx, gx2, None, None)),
           "backward_weight_bias_only": timed(bwd(None, None, gw, gb)),
           "aten_backward_all": timed(lambda: torch.autograd.grad(y, leaves, go, retain_graph=True), False),
           "aten_backward_inputs_only": timed(lambda: torch.autograd.grad(y, inputs, go, retain_graph=True), False),
           "aten_backward_weight_bias_only": timed(lambda: torch.autograd.grad(y, (weight, bias), go, retain_graph=True), False),
           "workspace_bytes": nb}
    ref = dict(zip([k for k, t in zip(("x", "x2", "weight", "bias", "residual"), (x, x2, weight, bias, resid)) if t is not None],
                   torch.autograd.grad(y, leaves, go, retain_graph=True)))
    assert bwd(gx, gx2, gw, gb)() == 0
    torch.cuda.synchronize()
    row["max_abs_diff_to_aten_over_max"] = {k: float((t - ref[k]).abs().max() / ref[k].abs().max())
                                            for k, t in (("x", gx), ("x2", gx2), ("weight", gw), ("bias", gb)) if t is not None}
    for leg in ("all", "inputs_only", "weight_bias_only"):
        row[f"{leg}_over_aten"] = round(row[f"backward_{leg}"]["median_us"] / row[f"aten_backward_{leg}"]["median_us"], 3)
    tag = f"{n}x{cin}+{cin2}->{cout}_{c['act']}" + ("_resid" if c.get("resid") else "") + (f"_shuffle{r}" if r else "") + f"_{h}x{w}"
    res["conv3x3_backward"][tag] = row
    del z, y, ref, leaves
print(json.dumps(res))
