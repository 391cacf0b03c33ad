"""8-bit frame I/O around the engines' fp32 tensors (crfp_frame_ingest_u8 / crfp_frame_export_u8, csrc/frameio.hip) and a pipelined host path
on top of them.

A host holds, and a display consumes, 8-bit frames; the engines take ``lr`` [3,h,w], a full 8h x 8w ``fv`` that is zero outside the fovea
window and a full-frame ``mk``, all fp32 / byte planes, and return fp32 NCHW.  The reference converts on the host in NumPy (dataset/reds.py:306,409
``astype(np.float32) / 255.``; :196-203 ``Ref`` = HR inside the window, 0 outside; test_video.py:396-410 chroma merge of a y_only model,
``(sr * 255.).clip(0., 255.)``, ``round()``, uint8, HWC, RGB -> BGR).  Here

  * ``ingest`` turns an 8-bit LR frame, an 8-bit fovea crop and one rectangle into ``(lr, fv, mk)`` on the device,
  * ``export`` turns the model's output into the 8-bit HWC frame on the device,
  * ``resize_bicubic`` is PIL's 8-bit ``Image.resize(..., BICUBIC)`` on the device, byte for byte (csrc/bicubic.hip): the reference's baseline
    frames (test_video.py:241), and ``export_y_bicubic`` puts that frame's chroma under a y_only model's luma in the same launch,
  * ``HostStreamer`` moves only those 8-bit tensors over PCIe and downloads frame i - 1 on a stream of its own while frame i computes,

so that a 180 x 320 frame costs 11.3 MB of transfers instead of 92.8 MB (``pcie_bytes``).  ``python -m crfp_amd.frameio`` times the four ways
to run a stream (fp32 tensors through pinned memory, 8-bit on one stream, HostStreamer, resident inputs) in one process."""
from __future__ import annotations

import collections
from typing import Tuple

import numpy as np
import torch

from . import _lib
from .ops import _on, _stream, upsample_bilinear


def _dev_as(t, name: str, dtype, shape_tail=None) -> torch.Tensor:
    """`t` as a contiguous device tensor of `dtype`; no conversion of the dtype: an 8-bit tensor that arrives as fp32 is a caller's mistake."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"crfp_amd: `{name}` must be a CUDA/HIP tensor (this build has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"crfp_amd.frameio: `{name}` must be {dtype}, got {t.dtype}")
    if shape_tail is not None and (t.dim() != 1 + len(shape_tail) or any(b is not None and a != b for a, b in zip(t.shape[1:], shape_tail))):
        raise ValueError(f"crfp_amd.frameio: `{name}` must be [n,{','.join('*' if b is None else str(b) for b in shape_tail)}], got {tuple(t.shape)}")
    return t.contiguous()


def ingest(lr_u8, crop_u8, rects, H: int, W: int, bgr: bool = False):
    """lr_u8 [n,h,w,3] uint8, crop_u8 [n,fh,fw,3] uint8, rects [n,4] int32 (y, x, flags, 0; flags bit 0 = the frame has a fovea), all on the
    device -> (lr [n,3,h,w] fp32, fv [n,3,H,W] fp32, mk [n,1,H,W] bool): lr = lr_u8 / 255; inside the crop's rectangle clipped to the frame
    fv = crop / 255 and mk = True, elsewhere fv = +0 and mk = False.  (y, x) is where the crop's pixel (0, 0) lies in the frame; the crop may
    hang over any edge or lie outside.  bgr: the 8-bit tensors are B,G,R per pixel.  lr_u8 = None skips lr (returned as None); crop_u8 = rects =
    None skips fv and mk.  One call on the current stream, nothing synchronised."""
    have_lr, have_fv = lr_u8 is not None, crop_u8 is not None or rects is not None
    if not (have_lr or have_fv):
        raise ValueError("crfp_amd.frameio.ingest: nothing to do (lr_u8, crop_u8 and rects are all None)")
    if (crop_u8 is None) != (rects is None):
        raise ValueError("crfp_amd.frameio.ingest: crop_u8 and rects go together")
    lr = fv = mk = None
    n = h = w = fh = fw = 1
    if have_lr:
        lr_u8 = _dev_as(lr_u8, "lr_u8", torch.uint8, (None, None, 3))
        n, h, w = lr_u8.shape[:3]
        lr = torch.empty((n, 3, h, w), dtype=torch.float32, device=lr_u8.device)
    if have_fv:
        crop_u8 = _dev_as(crop_u8, "crop_u8", torch.uint8, (None, None, 3))
        rects = _dev_as(rects, "rects", torch.int32, (_lib.IO_RECT_INTS,))
        if have_lr and crop_u8.shape[0] != n or rects.shape[0] != crop_u8.shape[0]:
            raise ValueError(f"crfp_amd.frameio.ingest: frame counts differ: lr_u8 {n if have_lr else None}, crop_u8 {crop_u8.shape[0]}, rects {rects.shape[0]}")
        n, fh, fw = crop_u8.shape[:3]
        fv = torch.empty((n, 3, H, W), dtype=torch.float32, device=crop_u8.device)
        mk = torch.empty((n, 1, H, W), dtype=torch.uint8, device=crop_u8.device)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    with _on(*(t for t in (lr_u8, crop_u8, rects) if t is not None)):
        _lib.check(_lib.lib().crfp_frame_ingest_u8(ptr(lr_u8) if have_lr else None, ptr(crop_u8) if have_fv else None, ptr(rects) if have_fv else None,
                                                   ptr(lr), ptr(fv), ptr(mk), n, h, w, fh, fw, H, W, _lib.IO_BGR if bgr else 0, _stream()),
                   "crfp_frame_ingest_u8")
    return lr, fv, None if mk is None else mk.view(torch.bool)


def export(sr, chroma=None, bgr: bool = False, out=None):
    """sr [n,c,H,W] fp32 on the device -> uint8 [n,H,W,3]: round-half-even(clip(sr * 255, 0, 255)), NaN -> 0.  c = 3 takes no chroma; c = 1 (a
    y_only model's luma) needs chroma [n,3,H,W] fp32 RGB, whose u and v go under sr's luma (test_video.py:396-410).  bgr: the bytes of a pixel
    are B,G,R.  out: a contiguous uint8 [n,H,W,3] device tensor to fill.  One call on the current stream, nothing synchronised."""
    sr = _dev_as(sr, "sr", torch.float32, (None, None, None))
    n, c, H, W = sr.shape
    if chroma is not None:
        chroma = _dev_as(chroma, "chroma", torch.float32, (3, H, W))
        if chroma.shape[0] != n:
            raise ValueError(f"crfp_amd.frameio.export: chroma holds {chroma.shape[0]} frames, sr {n}")
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=sr.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, H, W, 3) and out.is_contiguous()):
        raise ValueError(f"crfp_amd.frameio.export: `out` must be a contiguous uint8 device tensor [{n},{H},{W},3]")
    with _on(*(t for t in (sr, chroma, out) if t is not None)):
        _lib.check(_lib.lib().crfp_frame_export_u8(sr.data_ptr(), None if chroma is None else chroma.data_ptr(), out.data_ptr(), n, c, H, W,
                                                   _lib.IO_BGR if bgr else 0, _stream()), "crfp_frame_export_u8")
    return out


def _workspace(n: int, h: int, w: int, H: int, W: int, device, what: str) -> torch.Tensor:
    nbytes = _lib.lib().crfp_resize_bicubic_workspace_bytes(n, h, w, H, W)
    if nbytes == 0:
        raise ValueError(f"crfp_amd.frameio.{what}: {n} frames {h}x{w} -> {H}x{W} are outside what the bicubic kernels take")
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def resize_bicubic(src_u8, H: int, W: int, out: str = "u8", bgr: bool = False):
    """src_u8 [n,h,w,3] uint8 on the device -> PIL's ``Image.resize((W, H), Image.BICUBIC)`` of every frame, byte for byte: uint8 [n,H,W,3]
    (out="u8"), or those bytes / 255 as fp32 [n,3,H,W] RGB planes (out="f32"; bgr: src_u8 is B,G,R per pixel, and so is a uint8 result).  Any
    sizes >= 1, shrinking included.  One call on the current stream, nothing synchronised, no host copy: it can be captured in a graph."""
    if out not in ("u8", "f32"):
        raise ValueError(f"crfp_amd.frameio.resize_bicubic: out must be 'u8' or 'f32', got {out!r}")
    src_u8 = _dev_as(src_u8, "src_u8", torch.uint8, (None, None, 3))
    n, h, w = src_u8.shape[:3]
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"crfp_amd.frameio.resize_bicubic: H and W must be >= 1, got {H}, {W}")
    with _on(src_u8):
        ws = _workspace(n, h, w, H, W, src_u8.device, "resize_bicubic")
        dst = (torch.empty((n, H, W, 3), dtype=torch.uint8, device=src_u8.device) if out == "u8" else
               torch.empty((n, 3, H, W), dtype=torch.float32, device=src_u8.device))
        flags = (_lib.IO_BGR if bgr else 0) | (_lib.IO_OUT_F32 if out == "f32" else 0)
        _lib.check(_lib.lib().crfp_resize_bicubic_u8(src_u8.data_ptr(), dst.data_ptr(), n, h, w, H, W, flags, ws.data_ptr(), ws.numel(), _stream()),
                   "crfp_resize_bicubic_u8")
    return dst


def export_y_bicubic(luma, lr_u8, bgr: bool = False, out=None):
    """A y_only model's display frame as the reference makes it (test_video.py:396-410): luma [n,1,H,W] fp32 and the 8-bit LR frame lr_u8
    [n,h,w,3], both on the device -> uint8 [n,H,W,3] = ``export(luma, chroma=resize_bicubic(lr_u8, H, W, "f32"))`` in one launch that never
    writes the chroma frame.  H >= h and W >= w.  bgr: lr_u8 and the result are B,G,R per pixel.  out: a contiguous uint8 [n,H,W,3] device
    tensor to fill.  (``export`` keeps its four arguments; this is its c = 1 form on an 8-bit LR frame.)"""
    luma = _dev_as(luma, "luma", torch.float32, (1, None, None))
    n, _, H, W = luma.shape
    lr_u8 = _dev_as(lr_u8, "lr_u8", torch.uint8, (None, None, 3))
    if lr_u8.shape[0] != n:
        raise ValueError(f"crfp_amd.frameio.export_y_bicubic: lr_u8 holds {lr_u8.shape[0]} frames, luma {n}")
    h, w = lr_u8.shape[1:3]
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=luma.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, H, W, 3) and out.is_contiguous()):
        raise ValueError(f"crfp_amd.frameio.export_y_bicubic: `out` must be a contiguous uint8 device tensor [{n},{H},{W},3]")
    with _on(luma, lr_u8, out):
        ws = _workspace(n, h, w, H, W, luma.device, "export_y_bicubic")
        _lib.check(_lib.lib().crfp_frame_export_y_bicubic_u8(luma.data_ptr(), lr_u8.data_ptr(), out.data_ptr(), n, h, w, H, W,
                                                            _lib.IO_BGR if bgr else 0, ws.data_ptr(), ws.numel(), _stream()),
                   "crfp_frame_export_y_bicubic_u8")
    return out


def pcie_bytes(h: int, w: int, fv_size: int, out_channels: int = 3) -> dict:
    """Bytes over PCIe per streamed frame, from shapes: the fp32 API tensors (lr, fv, mk up; the output down) against the 8-bit ones (LR frame,
    fovea crop, rectangle up; the HWC frame down)."""
    H, W = 8 * h, 8 * w
    return {"fp32": 4 * 3 * h * w + 4 * 3 * H * W + H * W + 4 * out_channels * H * W,
            "u8": 3 * h * w + 3 * fv_size * fv_size + 4 * _lib.IO_RECT_INTS + 3 * H * W}


def _model_frame(model, lr, fv, mk, bgr: bool, y_only: bool, lr_u8=None):
    """One frame through a one-frame-per-call model and the export kernel: lr [1,3,h,w], fv [1,3,H,W], mk [1,1,H,W] -> uint8 [1,H,W,3].  A
    y_only model's chroma: the bicubic frame of lr_u8 [1,h,w,3] when that is given, else the bilinear x8 frame of lr."""
    sr = model(lrs=lr.unsqueeze(0), fvs=fv.unsqueeze(0), mks=mk.unsqueeze(0), fgs=None)
    sr = sr.reshape(1, -1, fv.shape[2], fv.shape[3])
    if y_only and lr_u8 is not None:
        return export_y_bicubic(sr, lr_u8, bgr=bgr)
    return export(sr, upsample_bilinear(lr, scale_factor=8) if y_only else None, bgr=bgr)


class HostStreamer:
    """A one-frame-per-call model (MRCF_simple_v18 interface: ``model(lrs=, fvs=, mks=, fgs=)``, ``clear_states()``) fed from and drained to host
    memory in 8-bit frames.  ``submit`` queues a frame and returns at once; ``fetch`` returns the oldest queued frame's output.

    Per frame one upload (LR frame, fovea crop and rectangle packed in one pinned slot, 0.2 MB at 180 x 320), one ingest call, the model, one
    export call and one download into a pinned slot (11 MB).  Upload and compute share the compute stream; the download runs on a stream of its
    own behind an event, so frame i - 1 downloads while frame i computes.  An upload stream of its own was measured and lost (DESIGN.md
    section 3.7): the process then holds five streams -- the default one, three here and the library's side stream -- on four hardware queues,
    the download and the side stream share one, and every frame's side work waits behind an 11 MB copy.  `depth` staging slots per direction:
    at most `depth` frames may be queued and not yet fetched.  The output handed to the download stream gets ``record_stream``.  A y_only
    model's chroma is the bilinear x8 LR frame (``ops.upsample_bilinear``), or with chroma="bicubic" the reference's: PIL's bicubic resize of
    the staged 8-bit LR frame, merged in the export launch (``export_y_bicubic``).  The model's ``inputs_resident`` must stay off: the ingest kernel
    that writes its inputs runs on the compute stream right in front of it, which is what that promise excludes."""

    def __init__(self, model, h: int, w: int, fv_size: int, depth: int = 2, bgr: bool = False, device=None, chroma: str = "bilinear"):
        if chroma not in ("bilinear", "bicubic"):
            raise ValueError(f"crfp_amd.frameio.HostStreamer: chroma must be 'bilinear' or 'bicubic', got {chroma!r}")
        if depth < 1:
            raise ValueError("crfp_amd.frameio.HostStreamer: depth must be >= 1")
        if getattr(model, "inputs_resident", False):
            raise ValueError("crfp_amd.frameio.HostStreamer: the model's inputs_resident must be off (its inputs are written on the compute stream)")
        device = torch.device("cuda:0" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError("crfp_amd: HostStreamer needs a CUDA/HIP device (this build has no CPU path)")
        self.model, self.h, self.w, self.fv, self.depth, self.bgr, self.dev = model, h, w, fv_size, depth, bool(bgr), device
        self.H, self.W = 8 * h, 8 * w
        self.y_only = bool(getattr(model, "y_only", False))
        self.chroma = chroma
        # one upload per frame: the rectangle, then the LR frame, then the crop (each 4-byte aligned)
        self._o_lr = 4 * _lib.IO_RECT_INTS
        self._o_crop = self._o_lr + (3 * h * w + 3) // 4 * 4
        self._in_bytes = self._o_crop + 3 * fv_size * fv_size
        self._in_pin = torch.empty((depth, self._in_bytes), dtype=torch.uint8).pin_memory()
        self._out_pin = torch.empty((depth, self.H, self.W, 3), dtype=torch.uint8).pin_memory()
        self._in_np, self._out_np = self._in_pin.numpy(), self._out_pin.numpy()   # the same memory
        with torch.cuda.device(device):
            self._comp, self._down = torch.cuda.Stream(), torch.cuda.Stream()
            self._uploaded = [torch.cuda.Event() for _ in range(depth)]
            self._computed = [torch.cuda.Event() for _ in range(depth)]
            self._downloaded = [torch.cuda.Event() for _ in range(depth)]
        self._used = [False] * depth          # the slot's upload event has been recorded
        self._queue = collections.deque()     # slots submitted and not fetched, oldest first
        self._count = 0

    def clear_states(self):
        """The next submitted frame starts a new sequence.  Frames already queued are not affected."""
        self.model.clear_states()

    def submit(self, lr_u8, crop_u8, origin: Tuple[int, int], has_fovea: bool = True):
        """lr_u8 [h,w,3], crop_u8 [fv,fv,3]: host uint8 arrays (NumPy or CPU tensors); origin (y, x): where the crop's pixel (0, 0) lies in the
        8h x 8w frame.  Copies both into a pinned slot, so the caller may reuse its arrays at once."""
        if len(self._queue) == self.depth:
            raise RuntimeError(f"crfp_amd.frameio.HostStreamer: {self.depth} frames are queued; fetch() one before the next submit()")
        for name, t in (("lr_u8", lr_u8), ("crop_u8", crop_u8)):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                raise ValueError(f"crfp_amd.frameio.HostStreamer.submit: `{name}` must be a host array (device tensors go through ingest)")
        lr_u8, crop_u8 = np.asarray(lr_u8), np.asarray(crop_u8)
        for name, t, shape in (("lr_u8", lr_u8, (self.h, self.w, 3)), ("crop_u8", crop_u8, (self.fv, self.fv, 3))):
            if t.dtype != np.uint8 or t.shape != shape:
                raise ValueError(f"crfp_amd.frameio.HostStreamer.submit: `{name}` must be a host uint8 array {shape}, got {t.dtype} {t.shape}")
        slot = self._count % self.depth
        self._count += 1
        if self._used[slot]:
            self._uploaded[slot].synchronize()   # the slot's previous upload has left the pinned buffer (`depth` frames ago: long done)
        pin, row = self._in_pin[slot], self._in_np[slot]
        row[:self._o_lr].view(np.int32)[:] = (int(origin[0]), int(origin[1]), _lib.IO_HAS_FOVEA if has_fovea else 0, 0)
        row[self._o_lr:self._o_lr + 3 * self.h * self.w].reshape(self.h, self.w, 3)[...] = lr_u8
        row[self._o_crop:].reshape(self.fv, self.fv, 3)[...] = crop_u8
        with torch.cuda.device(self.dev), torch.no_grad():
            with torch.cuda.stream(self._comp):
                staged = pin.to(self.dev, non_blocking=True)
                self._uploaded[slot].record(self._comp)
                self._used[slot] = True
                lr_u8 = staged[self._o_lr:self._o_lr + 3 * self.h * self.w].view(1, self.h, self.w, 3)
                lr, fv, mk = ingest(lr_u8,
                                    staged[self._o_crop:].view(1, self.fv, self.fv, 3), staged[:self._o_lr].view(torch.int32).view(1, -1),
                                    self.H, self.W, bgr=self.bgr)
                out = _model_frame(self.model, lr, fv, mk, self.bgr, self.y_only, lr_u8 if self.chroma == "bicubic" else None)
                self._computed[slot].record(self._comp)
            out.record_stream(self._down)
            with torch.cuda.stream(self._down):
                self._down.wait_event(self._computed[slot])
                self._out_pin[slot].copy_(out[0], non_blocking=True)
                self._downloaded[slot].record(self._down)
        self._queue.append(slot)

    def fetch(self, copy: bool = True) -> np.ndarray:
        """The oldest queued frame as a host uint8 array [8h,8w,3]; waits for its download.  copy=False returns a view of the pinned slot, valid
        until `depth` more frames have been submitted."""
        if not self._queue:
            raise RuntimeError("crfp_amd.frameio.HostStreamer: fetch() without a queued frame")
        slot = self._queue.popleft()
        self._downloaded[slot].synchronize()
        frame = self._out_np[slot]
        return frame.copy() if copy else frame

    def pending(self) -> int:
        return len(self._queue)


# ---------------------------------------------------------------------------------------------------------------- the four legs
def _spread(rates):
    return {"median": float(np.median(rates)), "min": float(min(rates)), "max": float(max(rates))}


def main(argv=None):
    """Frames/s of one streamed sequence, inputs starting and outputs ending in host memory, four ways in one process (alternating, three rounds
    each; median, minimum and maximum): (a) the fp32 API tensors through pinned memory on one stream, (b) 8-bit I/O on one stream, (c)
    HostStreamer, (d) the model alone on resident inputs.  One JSON line, with the bytes over PCIe per frame of each leg."""
    import argparse
    import json
    import time

    from . import synth
    from .model import CRFP

    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--storage", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--lr-h", type=int, default=180)
    ap.add_argument("--lr-w", type=int, default=320)
    ap.add_argument("--fv-size", type=int, default=96)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="", help="comma-separated subset of the legs to run (a profiler run of one leg); default: all four")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    h, w, fvs, N = a.lr_h, a.lr_w, a.fv_size, a.frames
    H, W = 8 * h, 8 * w
    m = CRFP.MRCF_simple_v18(device=dev, mid_channels=32)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state_dict(7).items()}, strict=True)
    m.storage = a.storage
    m = m.to(dev).eval()

    # host data: a few distinct 8-bit frames, cycled (what is moved does not depend on the content); the crop follows a gaze walk
    K = min(N, 8)
    lrs = synth.make_clip(1234, 1, K, h, w, fv_size=fvs)[0][0]
    lr_u8 = np.ascontiguousarray(np.rint(lrs * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))            # [K,h,w,3]
    rs = np.random.RandomState(1234)
    crops = rs.randint(0, 256, (K, fvs, fvs, 3)).astype(np.uint8)
    origins = [(int(np.clip(rs.normal(H / 2, 50) - fvs // 2, 0, H - fvs)), int(np.clip(rs.normal(W / 2, 50) - fvs // 2, 0, W - fvs))) for _ in range(N)]
    # (a): the same frames as the fp32 API tensors, built once on the device and kept in pinned memory
    rects = torch.tensor([[y, x, _lib.IO_HAS_FOVEA, 0] for y, x in origins[:K]], dtype=torch.int32)
    with torch.no_grad():
        f_lr, f_fv, f_mk = ingest(torch.from_numpy(lr_u8).to(dev), torch.from_numpy(crops).to(dev), rects.to(dev), H, W)
    p_lr, p_fv, p_mk = (t.cpu().pin_memory() for t in (f_lr, f_fv, f_mk))
    p_out = torch.empty((1, 3, H, W), dtype=torch.float32).pin_memory()
    # (b): pinned 8-bit staging, one slot
    q_lr, q_crop = torch.from_numpy(lr_u8).pin_memory(), torch.from_numpy(crops).pin_memory()
    q_rect = torch.tensor([[y, x, _lib.IO_HAS_FOVEA, 0] for y, x in origins], dtype=torch.int32).pin_memory()
    q_out = torch.empty((1, H, W, 3), dtype=torch.uint8).pin_memory()
    streamer = HostStreamer(m, h, w, fvs, depth=a.depth)

    def leg_fp32():
        for i in range(N):
            k = i % K
            lr, fv, mk = (t[k:k + 1].to(dev, non_blocking=True) for t in (p_lr, p_fv, p_mk))
            sr = m(lrs=lr.unsqueeze(0), fvs=fv.unsqueeze(0), mks=mk.unsqueeze(0), fgs=None)
            p_out.copy_(sr.reshape(1, 3, H, W), non_blocking=True)   # one staging frame, rewritten every frame as in tools/pcie_inclusive.py

    def leg_u8():
        for i in range(N):
            k = i % K
            lr, fv, mk = ingest(q_lr[k:k + 1].to(dev, non_blocking=True), q_crop[k:k + 1].to(dev, non_blocking=True),
                                q_rect[i:i + 1].to(dev, non_blocking=True), H, W)
            q_out.copy_(_model_frame(m, lr, fv, mk, False, False), non_blocking=True)

    def leg_streamer():
        for i in range(N):
            if streamer.pending() == a.depth:
                streamer.fetch(copy=False)
            streamer.submit(lr_u8[i % K], crops[i % K], origins[i])
        while streamer.pending():
            streamer.fetch(copy=False)

    def leg_resident():
        for i in range(N):
            k = i % K
            m(lrs=f_lr[k:k + 1].unsqueeze(0), fvs=f_fv[k:k + 1].unsqueeze(0), mks=f_mk[k:k + 1].unsqueeze(0), fgs=None)

    legs = {"fp32_pinned_one_stream": leg_fp32, "u8_one_stream": leg_u8, "host_streamer": leg_streamer, "model_resident": leg_resident}
    if a.legs:
        legs = {k: legs[k] for k in a.legs.split(",")}
    rates = {k: [] for k in legs}
    with torch.no_grad():
        for r in range(a.rounds + 1):          # round 0 warms every leg up
            for name, leg in legs.items():
                m.clear_states()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg()
                torch.cuda.synchronize()
                if r:
                    rates[name].append(N / (time.perf_counter() - t0))
    mb = pcie_bytes(h, w, fvs)
    per_frame = {"fp32_pinned_one_stream": mb["fp32"], "u8_one_stream": mb["u8"], "host_streamer": mb["u8"], "model_resident": 0}
    per_frame = {k: per_frame[k] for k in legs}
    print(json.dumps({"workload": f"{N} streamed frames {h}x{w} -> x8, fv {fvs}, storage {a.storage}, MRCF_simple_v18, synthetic; host memory to host memory",
                      "rounds": a.rounds, "frames_per_sec": {k: _spread(v) for k, v in rates.items()}, "pcie_bytes_per_frame": per_frame}))


if __name__ == "__main__":
    main()
