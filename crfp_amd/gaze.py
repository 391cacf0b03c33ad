"""Gaze-trajectory driver and region metrics for the streaming model: counterpart of the per-frame loop of the
reference's video rig (test_video.py:303-379; BASELINE config 3 = 100 streamed frames, sigma^T = 50).

Per frame n (one model call, state kept on the device between calls):
  * gaze centre (x, y) ~ N(frame centre, sigma^2), drawn up front as ``sigma*randn(N) + W/2`` then ``sigma*randn(N) + H/2``
    (test_video.py:310-311: x first, then y, from one NumPy stream); fovea window origin = int(centre) - fv_size//2
    (:335-336).  The reference does not clip it; a window that would leave the frame is clipped here (no-op otherwise).
  * fv = GT inside the window, 0 elsewhere; mk = 1 inside (:340-342), only from frame ``fv_start`` on;
    mk_fv = mk with the window forced to 1 (:344-345);
    mk_out = (10 x [3x3 ones conv, clamp]) dilation of mk_fv minus mk = the ring around the fovea (:346-349);
    mk_past = union of the last three mk_out, as it was BEFORE this frame's ring is pushed (:371-375);
    fg = the regional-DCN box of rg x rg pixels around the window centre, or all ones (:351-358).
  * metrics = utils.calc_psnr_and_ssim_cuda(sr, gt, mask) for whole / fovea / outskirt / past (:360-370), arithmetic mean.
  * rect_table / FusedRegionMasks (opt-in, ``fused_masks``): every mask above is a function of this frame's window, the three previous ones and
    the regional box, so one crfp_gaze_prep_f32 call per frame writes mk, fovea / outskirt / past (already stacked for the metrics table), fg
    and fv = gt inside mk from a rectangle table uploaded once per trajectory.
  * score maps (optional) = utils.foveated_metric(.., kernel_size=10, stride_size=5) of the model output and of a baseline frame
    against the ground truth (:381-384), and the running extrema the rig keeps from the baseline's call (:385-392).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F


def gaze_trajectory(n_frames: int, H: int, W: int, sigma: float, rng: np.random.RandomState) -> Tuple[np.ndarray, np.ndarray]:
    """test_video.py:310-311 (the reference draws from the global NumPy stream; pass a seeded RandomState)."""
    x_array = sigma * rng.randn(n_frames) + (W / 2)
    y_array = sigma * rng.randn(n_frames) + (H / 2)
    return x_array, y_array


def window_origin(x: float, y: float, fv_size: int, H: int, W: int) -> Tuple[int, int]:
    """(cur_y, cur_x) of test_video.py:335-336, clipped so that the fv_size window stays inside the frame."""
    cur_y = int(y) - fv_size // 2
    cur_x = int(x) - fv_size // 2
    return min(max(cur_y, 0), H - fv_size), min(max(cur_x, 0), W - fv_size)


def dilate10(mask: torch.Tensor, iterations: int = 10) -> torch.Tensor:
    """`iterations` x (3x3 ones convolution, clamp to [0,1]) on a {0,1} mask [*,1,H,W] (test_video.py:347-348) = one
    (2*iterations+1)^2 max filter."""
    k = 2 * iterations + 1
    return F.max_pool2d(mask.float(), kernel_size=k, stride=1, padding=iterations)


def regional_box(cur_y: int, cur_x: int, fv_size: int, rg_h: int, rg_w: int, H: int, W: int) -> Tuple[int, int, int, int]:
    """(y0, y1, x0, x1) of the regional-DCN box (test_video.py:351-354; the reference hard-codes 1920 x 1080 as W x H)."""
    x0 = max(cur_x + (fv_size // 2) - (rg_w // 2), 0)
    x1 = min(cur_x + (fv_size // 2) + (rg_w // 2), W)
    y0 = max(cur_y + (fv_size // 2) - (rg_h // 2), 0)
    y1 = min(cur_y + (fv_size // 2) + (rg_h // 2), H)
    return y0, y1, x0, x1


class RegionMasks:
    """The per-frame masks of the rig; keeps the three-frame history that mk_past needs."""

    def __init__(self, H: int, W: int, fv_size: int, device, fv_start: int = 0, regional_dcn: bool = False,
                 rg_h: int = 0, rg_w: int = 0):
        self.H, self.W, self.fv, self.dev = H, W, fv_size, device
        self.fv_start, self.regional, self.rg_h, self.rg_w = fv_start, regional_dcn, rg_h, rg_w
        self.history: List[torch.Tensor] = []
        self.past: Optional[torch.Tensor] = None

    def frame(self, n: int, cur_y: int, cur_x: int) -> Dict[str, torch.Tensor]:
        H, W, fv = self.H, self.W, self.fv
        mk = torch.zeros((1, 1, H, W), device=self.dev)
        if n >= self.fv_start:
            mk[:, :, cur_y:cur_y + fv, cur_x:cur_x + fv] = 1
        mk_fv = mk.clone()
        mk_fv[:, :, cur_y:cur_y + fv, cur_x:cur_x + fv] = 1
        mk_out = torch.logical_and(torch.logical_not(mk.bool()), dilate10(mk_fv).bool())
        if self.regional:
            y0, y1, x0, x1 = regional_box(cur_y, cur_x, fv, self.rg_h, self.rg_w, H, W)
            fg = torch.zeros((1, 1, H, W), device=self.dev)
            fg[:, :, y0:y1, x0:x1] = 1
        else:
            fg = torch.ones((1, 1, H, W), device=self.dev)
        out = {"mk": mk.bool(), "fovea": mk_fv.bool(), "outskirt": mk_out, "past": self.past, "fg": fg.bool()}
        # history update happens after the frame's metrics (test_video.py:371-375)
        self.history.append(mk_out)
        if len(self.history) > 3:
            self.history.pop(0)
        self.past = torch.stack(self.history, 0).any(0)
        return out


def rect_table(origins: Sequence[Tuple[int, int]], H: int, W: int, fv_size: int, fv_start: int = 0, regional_dcn: bool = False,
               rg_h: int = 0, rg_w: int = 0) -> np.ndarray:
    """The rows crfp_gaze_prep_f32 reads, int32 [N, 24], for the whole trajectory `origins` = [(cur_y, cur_x)] (window_origin's values): ints 0..3
    the regional box y0, y1, x0, x1 (regional_box; the whole frame without regional DCN), then four entries y, x, h, w, flags -- frame n's window,
    then those of frames n - 1, n - 2, n - 3; flags bit 0: the entry exists, bit 1: its window counts as mk (frame index >= fv_start)."""
    from ._lib import GAZE_COUNTS, GAZE_EXISTS, GAZE_ROW_INTS
    rows = np.zeros((len(origins), GAZE_ROW_INTS), dtype=np.int32)
    for n, (cur_y, cur_x) in enumerate(origins):
        rows[n, 0:4] = regional_box(cur_y, cur_x, fv_size, rg_h, rg_w, H, W) if regional_dcn else (0, H, 0, W)
        for e in range(min(n, 3) + 1):
            y, x = origins[n - e]
            rows[n, 4 + 5 * e:9 + 5 * e] = (y, x, fv_size, fv_size, GAZE_EXISTS | (GAZE_COUNTS if n - e >= fv_start else 0))
    return rows


class FusedRegionMasks:
    """RegionMasks from rectangles: the trajectory's rect_table is uploaded once and frame n is ONE crfp_gaze_prep_f32 call on row n (a device
    pointer offset: nothing is uploaded or synchronised per frame).  `origins` = [(cur_y, cur_x)] of every frame."""

    DILATE = 10   # dilate10's iterations

    def __init__(self, H: int, W: int, fv_size: int, device, fv_start: int = 0, regional_dcn: bool = False,
                 rg_h: int = 0, rg_w: int = 0, origins: Sequence[Tuple[int, int]] = ()):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("crfp_amd: FusedRegionMasks needs a CUDA/HIP device (this build has no CPU path)")
        self.H, self.W, self.dev = H, W, device
        self.rows_host = rect_table(origins, H, W, fv_size, fv_start, regional_dcn, rg_h, rg_w)
        self.rows = torch.from_numpy(self.rows_host).to(device)

    def frame(self, n: int, gt: Optional[torch.Tensor] = None) -> Dict[str, Optional[torch.Tensor]]:
        """RegionMasks.frame's dict for frame n (bool views of the byte planes; "past" is None on frame 0) plus "regions" = the uint8
        [1,3,H,W] stack fovea / outskirt / past that utils.frame_metrics_table takes and "fv" = gt [1,C,H,W] inside mk, 0 elsewhere (None
        without gt).  Fresh tensors every call: the engine may still be reading the previous frame's."""
        from . import _lib
        from .ops import _dev, _stream
        H, W = self.H, self.W
        if not 0 <= n < self.rows.shape[0]:
            raise IndexError(f"frame {n} is outside the trajectory of {self.rows.shape[0]} frames")
        c, fv = 1, None
        if gt is not None:
            gt = _dev(gt, "gt")
            if gt.dim() != 4 or gt.shape[0] != 1 or tuple(gt.shape[2:]) != (H, W) or gt.device != self.dev:
                raise ValueError(f"gt must be [1,C,{H},{W}] on {self.dev}, got {tuple(gt.shape)} on {gt.device}")
            c, fv = gt.shape[1], torch.empty_like(gt)
        mk = torch.empty((1, 1, H, W), dtype=torch.uint8, device=self.dev)
        fg = torch.empty((1, 1, H, W), dtype=torch.uint8, device=self.dev)
        regions = torch.empty((1, 3, H, W), dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().crfp_gaze_prep_f32(None if gt is None else gt.data_ptr(), self.rows[n].data_ptr(),
                                                     None if fv is None else fv.data_ptr(), mk.data_ptr(), regions.data_ptr(), fg.data_ptr(),
                                                     1, c, H, W, self.DILATE, _stream()), "crfp_gaze_prep_f32")
        rb = regions.view(torch.bool)
        return {"mk": mk.view(torch.bool), "fovea": rb[:, 0:1], "outskirt": rb[:, 1:2], "past": rb[:, 2:3] if n > 0 else None,
                "fg": fg.view(torch.bool), "fv": fv, "regions": regions}


def run_gaze_video(model, lr: torch.Tensor, gt: torch.Tensor, sigma: float, fv_size: int = 96, seed: int = 1234,
                   fv_start: int = 0, regional_dcn: bool = False, rg: int = 0, metric_fn=None, score_maps: bool = False,
                   baseline: Optional[torch.Tensor] = None, fused_metrics: bool = False, fused_masks: bool = False) -> Dict[str, object]:
    """Stream `lr [N,3,h,w]` / `gt [N,3,8h,8w]` (device tensors, range [0,1]) through `model` (MRCF_simple_v18 interface:
    ``model(lrs=, fvs=, mks=, fgs=)`` one frame per call, ``clear_states()``) along a gaussian gaze trajectory and collect
    the rig's region metrics.  Returns per-region mean PSNR / SSIM, the trajectory and the outputs' checksum.
    score_maps: also score every frame's output per 10 x 10 window at stride 5 (utils.foveated_metric, eval mode: nothing is
    drawn) -> "psnr_score" / "ssim_score" [N,Hr,Wr] on the device; with `baseline` [N,3,H,W] (the rig's bicubic frames) those
    too ("psnr_score_baseline" / "ssim_score_baseline") and "score_extrema" = the rig's running (psnr_min, psnr_max, ssim_min,
    ssim_max) from the baseline's calls, started at (1000, 0, 1000, 0) as the rig starts them (from the output's calls when
    there is no baseline).  All of it stays on the device: no host synchronisation is added to the loop.
    fused_metrics: the four regions of a frame come from ONE utils.frame_metrics_table call (masks fovea / outskirt / past; frame 0
    passes an all-zero past whose row is dropped), the rows stay on the device and are fetched once after the loop: the loop
    itself no longer synchronises.  Same dict.
    fused_masks: the masks and fv of a frame come from ONE crfp_gaze_prep_f32 call (FusedRegionMasks) instead of the composed RegionMasks and
    `gt * mk`; with fused_metrics its regions stack goes to the table as it is.  Same dict, same values."""
    regions_fn = None
    if fused_metrics:
        if metric_fn is not None:
            raise ValueError("fused_metrics scores with the library's own table: it cannot be combined with metric_fn")
        from . import utils as U
    elif metric_fn is None:
        from . import utils as U
        metric_fn, regions_fn = U.calc_psnr_and_ssim_cuda, U.calc_psnr_and_ssim_regions
    N, _, H, W = gt.shape
    xs, ys = gaze_trajectory(N, H, W, sigma, np.random.RandomState(seed))
    origins = [window_origin(xs[n], ys[n], fv_size, H, W) for n in range(N)]
    if fused_masks:
        masks = FusedRegionMasks(H, W, fv_size, gt.device, fv_start, regional_dcn, rg, rg, origins=origins)
    else:
        masks = RegionMasks(H, W, fv_size, gt.device, fv_start, regional_dcn, rg, rg)
    regions = ("whole", "fovea", "outskirt", "past")
    acc = {r: [] for r in regions}
    traj = []
    ones = torch.ones((1, 1, H, W), device=gt.device, dtype=torch.bool)
    maps = {k: [] for k in ("psnr_score", "ssim_score", "psnr_score_baseline", "ssim_score_baseline")}
    extrema = None
    rows = []          # fused_metrics: one [4, 4] device row block per frame
    no_past = torch.zeros((1, 1, H, W), device=gt.device, dtype=torch.bool)
    if score_maps:
        from . import utils as U
        extrema = torch.tensor([1000.0, 0.0, 1000.0, 0.0], device=gt.device)   # psnr_min, psnr_max, ssim_min, ssim_max
    model.clear_states()
    with torch.no_grad():
        for n in range(N):
            cur_y, cur_x = origins[n]
            traj.append((cur_y, cur_x))
            g = gt[n:n + 1]
            if fused_masks:
                m = masks.frame(n, g)
                fv = m["fv"]
            else:
                m = masks.frame(n, cur_y, cur_x)
                fv = g * m["mk"]
            sr = model(lrs=lr[n:n + 1].unsqueeze(0), fvs=fv.unsqueeze(0), mks=m["mk"].unsqueeze(0), fgs=m["fg"].unsqueeze(0))
            sr = sr.reshape(1, -1, H, W)
            todo = [(r, mask) for r, mask in (("whole", ones), ("fovea", m["fovea"]), ("outskirt", m["outskirt"]),
                                              ("past", m["past"])) if mask is not None]   # frame 0 has no past ring
            if fused_metrics:   # one call for the four regions, nothing fetched inside the loop
                if fused_masks:   # frame 0's past plane is all zero, as no_past is
                    stack = m["regions"]
                else:
                    stack = torch.cat((m["fovea"], m["outskirt"], m["past"] if m["past"] is not None else no_past), 1)
                rows.append(U.frame_metrics_table(sr, g, stack)[0])
            elif regions_fn is not None:   # one range probe and one host sync per frame
                for (r, _), (p, s) in zip(todo, regions_fn(sr, g, [mask for _, mask in todo])):
                    acc[r].append((float(p), float(s)))
            else:
                for r, mask in todo:
                    p, s = metric_fn(sr, g, mask)
                    acc[r].append((float(p), float(s)))
            if score_maps:
                hw, fv2 = (H, W), (fv_size, fv_size)
                ps, ss, pe, se = U.foveated_metric(None, sr[0], g[0], (cur_y, cur_x), hw, fv2, 10, 5, eval_mode=True)
                maps["psnr_score"].append(ps); maps["ssim_score"].append(ss)
                if baseline is not None:
                    ps, ss, pe, se = U.foveated_metric(None, baseline[n], g[0], (cur_y, cur_x), hw, fv2, 10, 5, eval_mode=True)
                    maps["psnr_score_baseline"].append(ps); maps["ssim_score_baseline"].append(ss)
                lo, hi = torch.stack([pe[0], se[0]]), torch.stack([pe[1], se[1]])
                extrema[0::2] = torch.minimum(extrema[0::2], lo)
                extrema[1::2] = torch.maximum(extrema[1::2], hi)
    if rows:
        table = torch.stack(rows).cpu()   # [N, 4, 4]: the one fetch
        for n in range(N):
            for k, r in enumerate(regions):
                if r != "past" or n > 0:   # frame 0 has no past ring
                    acc[r].append((float(table[n, k, 0]), float(table[n, k, 1])))
    out: Dict[str, object] = {"trajectory": traj, "frames": N}
    if score_maps:
        out.update({k: torch.stack(v) for k, v in maps.items() if v})
        out["score_extrema"] = extrema
    for r in regions:
        if acc[r]:
            out[f"psnr_{r}"] = float(np.mean([v[0] for v in acc[r]]))
            out[f"ssim_{r}"] = float(np.mean([v[1] for v in acc[r]]))
    out["per_frame"] = acc
    return out


def main(argv=None):
    """BASELINE config 3 shape: N streamed frames at h x w -> 8h x 8w, gaussian gaze (sigma^T), synthetic data and
    weights (no REDS / checkpoints on the box); prints one JSON line with frames/s and the region metrics."""
    import argparse
    import json
    import time

    from . import synth
    from .model import CRFP

    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--lr-h", type=int, default=180)
    ap.add_argument("--lr-w", type=int, default=320)
    ap.add_argument("--sigma", type=float, default=50.0)
    ap.add_argument("--fv-size", type=int, default=96)
    ap.add_argument("--regional-dcn", type=int, default=0, help="side of the regional-DCN box in HR pixels (0 = whole frame)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--model-code", type=int, default=18, choices=(13, 15, 18),
                    help="the streaming model test_video.py builds for this code: 13 MRCF_simple_v13, 15 MRCF_simple_v15, 18 MRCF_simple_v18")
    ap.add_argument("--cra", action="store_true",
                    help="with --model-code 18: MRCF_simple_v18_cra, the streaming form of the cross-resolution wiring CRFP_DSV_CRA")
    ap.add_argument("--score-maps", action="store_true",
                    help="also time the stream with the per-window score maps of the output and of the x8 baseline (--baseline)")
    ap.add_argument("--baseline", choices=("bilinear", "bicubic"), default="bilinear",
                    help="the baseline frame of --score-maps: the bilinear x8 frame, or the rig's own (PIL's 8-bit bicubic resize of the 8-bit LR "
                         "frame, / 255: frameio.resize_bicubic)")
    ap.add_argument("--fused-metrics", action="store_true",
                    help="also time the stream with the four regions of a frame scored by one fused call and fetched once at the end")
    ap.add_argument("--fused-masks", action="store_true",
                    help="also time the stream with the masks and the fovea frame of a frame from one fused call, and the fused region metrics")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if a.cra and a.model_code != 18:
        ap.error("--cra selects MRCF_simple_v18_cra: it goes with --model-code 18")
    if a.cra:   # its own parameter table: weights seeded from it, as for the ablation wirings
        m = CRFP.MRCF_simple_v18_cra(device=dev, mid_channels=32, y_only=False, hr_dcn=True, offset_prop=True)
        sd = synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, 7)
    elif a.model_code == 18:
        sd = synth.make_state_dict(7)
        m = CRFP.MRCF_simple_v18(device=dev, mid_channels=32)
    else:   # the ablation wirings have other shapes under the same keys: weights seeded from the model's own table
        m = getattr(CRFP, f"MRCF_simple_v{a.model_code}")(device=dev, mid_channels=32, y_only=False, hr_dcn=True, offset_prop=True)
        sd = synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, 7)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    chunk = 10   # synthetic frames are generated in chunks of correlated frames and the state carried across
    lrs = np.concatenate([synth.make_clip(a.seed + i, 1, min(chunk, a.frames - i), a.lr_h, a.lr_w, fv_size=a.fv_size)[0][0]
                          for i in range(0, a.frames, chunk)], 0)
    lr = torch.from_numpy(lrs).to(dev)
    gt = torch.clamp(F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False), 0, 1)   # stand-in ground truth
    run = lambda: run_gaze_video(m, lr, gt, a.sigma, a.fv_size, a.seed, regional_dcn=a.regional_dcn > 0, rg=a.regional_dcn)
    run_gaze_video(m, lr[:3], gt[:3], a.sigma, a.fv_size, a.seed)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the same stream without the metric kernels and their host syncs
    ones = torch.ones((1, 1, 1, gt.shape[2], gt.shape[3]), device=dev, dtype=torch.bool)
    m.clear_states()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for n in range(a.frames):
            m(lrs=lr[n:n + 1].unsqueeze(0), fvs=gt[n:n + 1].unsqueeze(0), mks=ones, fgs=ones)
    torch.cuda.synchronize()
    dt_model = time.perf_counter() - t0
    res.pop("per_frame"); res.pop("trajectory")
    extra = {}
    if a.score_maps:   # the same stream once more with both score maps per frame; the baseline is the bilinear x8 frame, unclamped, or ...
        if a.baseline == "bicubic":   # ... test_video.py:241 on the device: the 8-bit LR frames through PIL's bicubic, as fractions of 255
            from . import frameio
            lr_u8 = torch.from_numpy(np.ascontiguousarray(np.rint(lrs * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))).to(dev)
            base = frameio.resize_bicubic(lr_u8, 8 * a.lr_h, 8 * a.lr_w, out="f32")
        else:
            base = F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False)
        run_gaze_video(m, lr[:3], gt[:3], a.sigma, a.fv_size, a.seed, score_maps=True, baseline=base[:3])   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sm = run_gaze_video(m, lr, gt, a.sigma, a.fv_size, a.seed, regional_dcn=a.regional_dcn > 0, rg=a.regional_dcn,
                            score_maps=True, baseline=base)
        torch.cuda.synchronize()
        extra["frames_per_sec_with_score_maps"] = a.frames / (time.perf_counter() - t0)
        extra["score_extrema"] = [float(v) for v in sm["score_extrema"].cpu()]
        extra["baseline"] = a.baseline
    if a.fused_metrics:
        run_gaze_video(m, lr[:3], gt[:3], a.sigma, a.fv_size, a.seed, fused_metrics=True)   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_gaze_video(m, lr, gt, a.sigma, a.fv_size, a.seed, regional_dcn=a.regional_dcn > 0, rg=a.regional_dcn, fused_metrics=True)
        torch.cuda.synchronize()
        extra["frames_per_sec_with_fused_region_metrics"] = a.frames / (time.perf_counter() - t0)
    if a.fused_masks:
        run_gaze_video(m, lr[:3], gt[:3], a.sigma, a.fv_size, a.seed, fused_metrics=True, fused_masks=True)   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_gaze_video(m, lr, gt, a.sigma, a.fv_size, a.seed, regional_dcn=a.regional_dcn > 0, rg=a.regional_dcn, fused_metrics=True,
                       fused_masks=True)
        torch.cuda.synchronize()
        extra["frames_per_sec_with_fused_masks_and_metrics"] = a.frames / (time.perf_counter() - t0)
    model = "" if a.model_code == 18 and not a.cra else f", {type(m).__name__}"
    print(json.dumps({"workload": f"BASELINE config 3 shape: {a.frames} streamed frames {a.lr_h}x{a.lr_w} -> x8, sigma_T={a.sigma}, fp32, synthetic{model}",
                      "frames_per_sec_with_region_metrics": a.frames / dt, "frames_per_sec_model_only": a.frames / dt_model, **extra, **res}))


if __name__ == "__main__":
    main()
