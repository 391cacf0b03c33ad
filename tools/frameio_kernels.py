#!/usr/bin/env python3
"""Device time of the 8-bit frame I/O calls at 1 x 3 x 1440 x 2560, fv 96, through the C-ABI with every output preallocated:
device events around one call (median / min / p90 of 200 calls after a warm-up) and one event pair around 200 calls back to back; each as a share
of the measured copy ceiling over the bytes the call cannot avoid.  crfp_gaze_prep_f32 runs beside them as the yardstick of the same kind of work
(profiles/r11_gaze_prep.txt).  The legs run in three rounds, alternating, in one process: the figures pool the rounds and `round_medians_us`
shows their spread.  The y_only display path both ways: `y_only_bilinear` = crfp_upsample_bilinear_f32 of the LR frame and crfp_frame_export_u8
with c = 1 (two calls, an fp32 chroma frame written and read back), `export_y_bicubic` = crfp_frame_export_y_bicubic_u8 on the 8-bit LR frame
(table kernel + one fused launch).  One JSON line."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crfp_amd import _lib, gaze   # noqa: E402

COPY_CEILING = 6.29e12   # bytes/s, the measured device copy rate
h, w, fv, calls, rounds = 180, 320, 96, 200, 3
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
chroma = torch.empty((1, 3, H, W), device=dev)
lr_f = lr_u8.permute(0, 3, 1, 2).float().div(255.0).contiguous()
ws = torch.empty((L.crfp_resize_bicubic_workspace_bytes(1, h, w, H, W),), dtype=torch.uint8, device=dev)
s = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()   # noqa: E731


def y_only_bilinear():
    return (L.crfp_upsample_bilinear_f32(p(lr_f), p(chroma), 1, 3, h, w, H, W, 0.125, 0.125, 1.0, s) or
            L.crfp_frame_export_u8(p(sr1), p(chroma), p(out), 1, 1, H, W, 0, s))


def bicubic(dst, flags):
    return lambda: L.crfp_resize_bicubic_u8(p(lr_u8), p(dst), 1, h, w, H, W, flags, p(ws), ws.numel(), s)


# name -> (call, compulsory bytes)
legs = {
    "ingest": (lambda: L.crfp_frame_ingest_u8(p(lr_u8), p(crop), p(rect), p(lr), p(fvt), p(mk), 1, h, w, fv, fv, H, W, 0, s),
               12 * H * W + H * W + 12 * h * w + 3 * h * w + 3 * fv * fv + 16),
    "ingest_fovea_only": (lambda: L.crfp_frame_ingest_u8(None, p(crop), p(rect), None, p(fvt), p(mk), 1, h, w, fv, fv, H, W, 0, s),
                          12 * H * W + H * W + 3 * fv * fv + 16),
    "export_c3": (lambda: L.crfp_frame_export_u8(p(sr3), None, p(out), 1, 3, H, W, 0, s), 12 * H * W + 3 * H * W),
    "export_c1": (lambda: L.crfp_frame_export_u8(p(sr1), p(sr3), p(out), 1, 1, H, W, 0, s), 16 * H * W + 3 * H * W),
    "upsample_bilinear": (lambda: L.crfp_upsample_bilinear_f32(p(lr_f), p(chroma), 1, 3, h, w, H, W, 0.125, 0.125, 1.0, s), 12 * H * W + 12 * h * w),
    "y_only_bilinear": (y_only_bilinear, 4 * H * W + 3 * H * W + 12 * h * w),
    "export_y_bicubic": (lambda: L.crfp_frame_export_y_bicubic_u8(p(sr1), p(lr_u8), p(out), 1, h, w, H, W, 0, p(ws), ws.numel(), s),
                         4 * H * W + 3 * H * W + 3 * h * w),
    "resize_bicubic_u8": (bicubic(out, 0), 3 * H * W + 3 * h * w),
    "resize_bicubic_f32": (bicubic(chroma, _lib.IO_OUT_F32), 12 * H * W + 3 * h * w),
    "resize_bicubic_u8_two_pass": (bicubic(out, _lib.IO_TWO_PASS), 3 * H * W + 3 * h * w),
    "gaze_prep": (lambda: L.crfp_gaze_prep_f32(p(sr3), p(rows), p(fvt), p(mk), p(regions), p(fg), 1, 3, H, W, 10, s),
                  12 * H * W + 5 * H * W + 12 * fv * fv),
}
samples = {k: [] for k in legs}
b2bs = {k: [] for k in legs}
for name, (fn, nbytes) in legs.items():
    for _ in range(20):
        assert fn() == 0, L.crfp_last_error_string()
torch.cuda.synchronize()
for _ in range(rounds):
    for name, (fn, nbytes) in legs.items():
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        samples[name].append(np.array([a.elapsed_time(b) for a, b in ev]) * 1e3)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        b2bs[name].append(a.elapsed_time(b) * 1e3 / calls)
res = {}
for name, (fn, nbytes) in legs.items():
    us = np.concatenate(samples[name])
    med, b2b = float(np.median(us)), float(np.median(b2bs[name]))
    res[name] = {"median_us": round(med, 2), "min_us": round(float(us.min()), 2), "p90_us": round(float(np.percentile(us, 90)), 2),
                 "round_medians_us": [round(float(np.median(r)), 2) for r in samples[name]],
                 "back_to_back_us": round(b2b, 2), "back_to_back_rounds_us": [round(v, 2) for v in b2bs[name]],
                 "compulsory_MB": round(nbytes / 1e6, 2),
                 "share_of_copy_ceiling": round(nbytes / COPY_CEILING / (med * 1e-6), 3),
                 "share_back_to_back": round(nbytes / COPY_CEILING / (b2b * 1e-6), 3)}
print(json.dumps({"shape": f"1x3x{H}x{W}, fv {fv}", "calls": calls, "rounds": rounds, "copy_ceiling_TBps": COPY_CEILING / 1e12, **res}))
