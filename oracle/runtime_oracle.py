"""ORACLE -- TEST INFRASTRUCTURE ONLY.  CPU fp32 restatement of the reference's benchmark-only wiring
``model/CRFP_runtime.py::MRCF_simple_v18.forward(lrs, fvs, warp_size)`` (:8469-8664) with
``ResidualBlocksWithInputConv_v2`` (:511-556) and that file's ``DCN_module`` (:135-219, same arithmetic as
model/CRFP.py:324-352).  Functional over a flat ``{key: tensor}`` state dict; building blocks come from
``oracle.crfp_oracle``.

Pinning: ``tests/golden/runtime_small.npz`` holds the output of the REFERENCE class itself, run on the CPU in the build
container (``tests/golden/make_runtime_golden.py``: the module's import-time ``.to('cuda:0')`` of its pixel grid, its
``torch.cuda`` timers and the absent ``memory_profiler`` / ``dcn_v2`` packages are neutralised there); DCNv2 inside it is
the oracle's own, so the golden pins the wiring, like every other golden that passes through DCNv2."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from . import crfp_oracle as o

Tensor = torch.Tensor


def rb_v2(P: Dict[str, Tensor], pre: str, feat1: Tensor, feat2: Tensor = None) -> Tensor:
    """ResidualBlocksWithInputConv_v2.forward (:541-556): conv1(feat1) pasted over conv2(feat2), LeakyReLU, one residual block."""
    if feat2 is not None:
        H, W = feat1.shape[-2:]
        feat = o.conv(P, pre + "conv2", feat2).clone()
        feat[:, :, :H, :W] = o.conv(P, pre + "conv1", feat1)
    else:
        feat = o.conv(P, pre + "conv1", feat1)
    x = o.lrelu(feat)
    return x + o.conv(P, pre + "main.1.0.conv2", F.relu(o.conv(P, pre + "main.1.0.conv1", x)))


def runtime_forward(P: Dict[str, Tensor], lrs: Tensor, fvs: Tensor, warp_size: Tuple[int, int], y_only: bool = False,
                    flows: Optional[Tensor] = None, taps: Optional[dict] = None) -> Tensor:
    """MRCF_simple_v18.forward (:8469-8664), split_ratio 3, offset_prop True.  Runs in the dtype of P / lrs / fvs (float64 as well).
    flows: [n, t-1, 2, WP_h/8, WP_w/8] used in place of FNet's (an engine's own flow, so that a comparison measures the gathers and not
    two evaluations of tanh * 256).  taps: a dict that receives the intermediates under the names of the engine's workspace buffers
    (crfp_rt_debug_fetch): flow_lr, x_lr, x_hr over the clip, everything else of the last frame; flow2 / flow8 as [n,H,W,2]."""
    WP_h, WP_w = warp_size
    n, t, c, h, w = lrs.shape
    if flows is None:
        flows = o.compute_flow(P, lrs[:, :, :, :WP_h // 8, :WP_w // 8]) if t > 1 else None      # :8487
    elif t < 2 or tuple(flows.shape) != (n, t - 1, 2, WP_h // 8, WP_w // 8):
        raise ValueError(f"flows {tuple(flows.shape)}: expected {(n, t - 1, 2, WP_h // 8, WP_w // 8)}")
    else:
        flows = flows.to(lrs.dtype)
    tp = {} if taps is None else taps
    inner = {}                                   # dcn_module's own taps ("dcn_k.aligned", "dcn_3.pre_offset")
    lr2 = lrs.reshape(n * t, c, h, w)
    x_lr = o.lrelu(o.conv(P, "encoder_lr.slice1.2", o.lrelu(o.conv(P, "encoder_lr.slice1.0", lr2)))).view(n, t, -1, h, w)
    Hf, Wf = fvs.shape[-2:]
    fv2 = fvs.reshape(n * t, 3, Hf, Wf)
    x_hr = torch.cat((fv2, fv2), 1)                                                             # :8507
    x_hr = o.lrelu(o.conv(P, "encoder_hr.slice1.2", o.lrelu(o.conv(P, "encoder_hr.slice1.0", x_hr)))).view(n, t, -1, Hf, Wf)
    outs = []
    state = feat_lv = None
    for i in range(t):
        prop0 = o.pixel_shuffle_pack(P, "upsample.", x_lr[:, i], 2)                             # :8524
        if i > 0:
            flow = flows[:, i - 1]
            flow_lv3 = o.up_bilinear(flow, 2) * 2.0                                             # :8531
            flow_lv0 = o.up_bilinear(flow, 8) * 8.0
            state_w = o.flow_warp(state, flow_lv0.permute(0, 2, 3, 1))                          # :8534-8535
            prev2_w = o.pixel_unshuffle_pack_v2(P, "downsample.", state_w, 4)                   # :8536
            prev2 = o.pixel_unshuffle_pack_v2(P, "downsample.", state, 4)                       # :8537
            mix = torch.chunk(o.flow_warp(torch.cat(feat_lv, 1), flow_lv3.permute(0, 2, 3, 1)), 3, dim=1)   # :8538-8547
            feat_lv = list(mix)
            win = prop0[:, :, :WP_h // 4, :WP_w // 4]
            tp.update(flow2=flow_lv3.permute(0, 2, 3, 1), flow8=flow_lv0.permute(0, 2, 3, 1), state_w=state_w, prev2w=prev2_w, prev2=prev2,
                      carryw=torch.cat(feat_lv, 1), win=win)
            off = None
            with o.tapping(inner):
                for k in range(3):                                                              # :8549-8599
                    feat_temp = torch.cat((win, feat_lv[k]), 1)
                    aligned, off = o.dcn_module(P, f"dcn_{k}.", feat_temp, prev2, prev2_w, flow_lv3, off,
                                                dg=8, repeat=False, interpolate="none")
                    tp[f"offfeat{k}"], tp[f"aligned{k}"] = off, aligned
                    y = rb_v2(P, f"forward_resblocks_{k}.", torch.cat([feat_temp, aligned], 1), feat_temp)
                    feat_lv[k] = y[:, 24:][:, :, :WP_h // 4, :WP_w // 4]
                up = o.lrelu(o.pixel_shuffle_pack(P, "upsample_post.", prop0, 4))               # :8602
                upw = up[:, :, :WP_h, :WP_w]
                aligned, _ = o.dcn_module(P, "dcn_3.", upw, state, state_w, flow_lv0, off,
                                          dg=1, repeat=True, interpolate="pixelshuffle")        # :8603-8606
            tp.update(upw=upw, al3=aligned, poff=inner["dcn_3.pre_offset"])
            feat = rb_v2(P, "forward_resblocks_3.", torch.cat([upw, aligned], 1), up)          # :8607-8609
        else:
            feat_lv = []
            for k in range(3):                                                                  # :8617-8633
                y = rb_v2(P, f"forward_resblocks_{k}_.", prop0)            # same two-input class, feat2 = None (:464-509)
                feat_lv.append(y[:, 24:][:, :, :WP_h // 4, :WP_w // 4])
                prop0 = y[:, :24]
            up = o.lrelu(o.pixel_shuffle_pack(P, "upsample_post.", prop0, 4))                   # :8636
            feat = rb_v2(P, "forward_resblocks_3_.", up)                                        # :8637
        fused = o.conv(P, "conv_tttf", torch.cat([feat[:, :, :Hf, :Wf], x_hr[:, i]], 1))        # :8645-8647
        feat_pre = o.lrelu(feat)
        feat = feat.clone()
        feat[:, :, :Hf, :Wf] = fused
        feat = o.lrelu(feat)                                                                    # :8648
        base = o.up_bilinear(o.rgb_to_y(lrs[:, i]), 8) if y_only else o.up_bilinear(lrs[:, i], 8)
        outs.append(o.conv(P, "conv_last", feat) + base)                                        # :8652-8654
        state = feat[:, :, :WP_h, :WP_w]                                                        # :8650
    # (x_lr, x_hr, flow_lr: the frames of the last clip, as the engine's workspace holds them.  Two taps no buffer has: `tttf`, the activated
    # conv_tttf crop that is pasted in, and `feat_pre`, the LeakyReLU branch it replaces there)
    tp.update(x_lr=x_lr[-1], x_hr=x_hr[-1], feat2=feat, state=state, carry=torch.cat(feat_lv, 1), tttf=o.lrelu(fused), feat_pre=feat_pre)
    if t > 1:
        tp["flow_lr"] = flows[-1]
    return torch.stack(outs, 1)
