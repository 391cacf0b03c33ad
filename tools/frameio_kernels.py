#!/usr/bin/env python3
"""Device time of the 8-bit frame I/O calls at 1 x 3 x 1440 x 2560, fv 96, through the C-ABI with every output preallocated:
device events around one call (median / min / p90 of 200 calls after a warm-up) and one event pair around 200 calls back to back; each as a share
of the measured copy ceiling over the bytes the call cannot avoid.  crfp_gaze_prep_f32 runs beside them as the yardstick of the same kind of work
(profiles/r11_gaze_prep.txt).  One JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crfp_amd import _lib, gaze   # noqa: E402

COPY_CEILING = 6.29e12   # bytes/s, the measured device copy rate
h, w, fv, calls = 180, 320, 96, 200
H, W = 8 * h, 8 * w
dev = torch.device("cuda:0")
L = _lib.lib()
rs = np.random.RandomState(0)
lr_u8 = torch.from_numpy(rs.randint(0, 256, (1, h, w, 3)).astype(np.uint8)).to(dev)
crop = torch.from_numpy(rs.randint(0, 256, (1, fv, fv, 3)).astype(np.uint8)).to(dev)
rect = torch.tensor([[700, 1200, _lib.IO_HAS_FOVEA, 0]], dtype=torch.int32, device=dev)
rows = torch.from_numpy(gaze.rect_table([(700, 1200)], H, W, fv)).to(dev)
sr3 = torch.rand((1, 3, H, W), device=dev) * 1.2 - 0.1
sr1 = sr3[:, :1].contiguous()
lr = torch.empty((1, 3, h, w), device=dev)
fvt = torch.empty((1, 3, H, W), device=dev)
mk, fg = (torch.empty((1, 1, H, W), dtype=torch.uint8, device=dev) for _ in range(2))
regions = torch.empty((1, 3, H, W), dtype=torch.uint8, device=dev)
out = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
s = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()   # noqa: E731

# name -> (call, compulsory bytes)
legs = {
    "ingest": (lambda: L.crfp_frame_ingest_u8(p(lr_u8), p(crop), p(rect), p(lr), p(fvt), p(mk), 1, h, w, fv, fv, H, W, 0, s),
               12 * H * W + H * W + 12 * h * w + 3 * h * w + 3 * fv * fv + 16),
    "ingest_fovea_only": (lambda: L.crfp_frame_ingest_u8(None, p(crop), p(rect), None, p(fvt), p(mk), 1, h, w, fv, fv, H, W, 0, s),
                          12 * H * W + H * W + 3 * fv * fv + 16),
    "export_c3": (lambda: L.crfp_frame_export_u8(p(sr3), None, p(out), 1, 3, H, W, 0, s), 12 * H * W + 3 * H * W),
    "export_c1": (lambda: L.crfp_frame_export_u8(p(sr1), p(sr3), p(out), 1, 1, H, W, 0, s), 16 * H * W + 3 * H * W),
    "gaze_prep": (lambda: L.crfp_gaze_prep_f32(p(sr3), p(rows), p(fvt), p(mk), p(regions), p(fg), 1, 3, H, W, 10, s),
                  12 * H * W + 5 * H * W + 12 * fv * fv),
}
res = {}
for name, (fn, nbytes) in legs.items():
    for _ in range(20):
        assert fn() == 0, L.crfp_last_error_string()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    b2b = a.elapsed_time(b) * 1e3 / calls
    med = float(np.median(us))
    res[name] = {"median_us": round(med, 2), "min_us": round(float(us.min()), 2), "p90_us": round(float(np.percentile(us, 90)), 2),
                 "back_to_back_us": round(b2b, 2), "compulsory_MB": round(nbytes / 1e6, 2),
                 "share_of_copy_ceiling": round(nbytes / COPY_CEILING / (med * 1e-6), 3),
                 "share_back_to_back": round(nbytes / COPY_CEILING / (b2b * 1e-6), 3)}
print(json.dumps({"shape": f"1x3x{H}x{W}, fv {fv}", "calls": calls, "copy_ceiling_TBps": COPY_CEILING / 1e12, **res}))
