"""Operator-level wrappers over the C-ABI (device tensors in, device tensors out).

Every function requires float32 CUDA(=HIP) tensors; CPU tensors raise -- the CPU restatement of
the path lives in ``oracle/`` and is test infrastructure, never a fallback.
"""
from __future__ import annotations

import torch

from . import _lib

ACT = {"none": 0, "relu": 1, "lrelu": 2, "tanh": 3, "sigmoid": 4}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"crfp_amd: `{name}` must be a CUDA/HIP tensor (this build has no CPU path)")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _on(*tensors):
    """Context that makes the operands' device current (the C-ABI enqueues on a stream of the CURRENT device, so the
    stream handle must be taken inside this block); all operands must live on one device."""
    devs = {t.device for t in tensors if isinstance(t, torch.Tensor)}
    if len(devs) != 1:
        raise RuntimeError(f"crfp_amd: operands on different devices: {sorted(map(str, devs))}")
    return torch.cuda.device(devs.pop())


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# Weights of the per-operator entry points are repacked on EVERY call, on the caller's stream, right in front of the kernel that
# reads them (one ~3 us pack launch).  Round 2 cached the packed image on the weight tensor keyed by ``Tensor._version``; writes
# through ``.data`` (which the reference uses: ``m.weight.data *= scale``, conv_identify at model/CRFP.py:359-370) do not bump
# that counter, so the cache could serve stale weights, and an image packed on one stream could be read half-written from
# another.  Callers that own the immutability of their weights hoist the repack themselves: ``pack_conv3x3`` /
# ``conv3x3_packed`` and ``pack_dcnv2_g8`` / ``dcnv2_g8_packed`` (the C-ABI's *_pack_f32 / *_packed_f32 forms); the engine
# (crfp_amd/engine.py) packs once per ``DSVEngine`` and is rebuilt by ``CRFP_DSV.engine()`` / ``invalidate_packed()``.


def _pack_buf(nbytes, device):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("crfp_amd.ops: per-call weight repacking allocates; inside CUDA-graph capture use the *_packed forms "
                           "with an image packed before the capture")
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def pack_conv3x3(weight, bias=None):
    """Packed image of a [cout, cin, 3, 3] weight (+ bias) for ``conv3x3_packed``; valid until the caller changes the weights.
    Produced on the current stream: use it on that stream, or order the consumer behind it."""
    weight = _dev(weight, "weight")
    cout, cin = weight.shape[:2]
    assert tuple(weight.shape) == (cout, cin, 3, 3), "conv3x3: weight must be [cout, cin, 3, 3]"
    bias = torch.zeros(cout, dtype=torch.float32, device=weight.device) if bias is None else _dev(bias, "bias")
    L = _lib.lib()
    with _on(weight, bias):
        pk = _pack_buf(L.crfp_conv3x3_packed_bytes(cin, cout), weight.device)
        _lib.check(L.crfp_conv3x3_pack_f32(weight.data_ptr(), bias.data_ptr(), cin, cout, pk.data_ptr(), pk.numel(), _stream()),
                   "crfp_conv3x3_pack_f32")
    pk._crfp_shape = (cin, cout)
    return pk


def conv3x3_packed(x, packed, act="none", post_scale=1.0):
    """conv3x3 with an image from ``pack_conv3x3``."""
    x = _dev(x, "x")
    cin, cout = packed._crfp_shape
    n, c, h, w = x.shape
    assert c == cin, f"conv3x3_packed: input has {c} channels, the packed weight {cin}"
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    with _on(x, packed):
        _lib.check(_lib.lib().crfp_conv3x3_packed_f32(x.data_ptr(), packed.data_ptr(), out.data_ptr(), n, cin, cout, h, w, ACT[act],
                                                      float(post_scale), _stream()), "crfp_conv3x3_packed_f32")
    return out


def pack_dcnv2_g8(weight):
    """Packed image of a DCNv2(32 -> 32, 3x3, 8 groups) weight for ``dcnv2_g8_packed``."""
    weight = _dev(weight, "weight")
    assert tuple(weight.shape) == (32, 32, 3, 3)
    L = _lib.lib()
    with _on(weight):
        pk = _pack_buf(L.crfp_dcnv2_g8_packed_bytes(), weight.device)
        _lib.check(L.crfp_dcnv2_g8_pack_f32(weight.data_ptr(), pk.data_ptr(), pk.numel(), _stream()), "crfp_dcnv2_g8_pack_f32")
    return pk


def dcnv2_g8_packed(x, offset, mask, packed, bias):
    """DCNv2(32 -> 32, 3x3, pad 1, 8 groups) with an image from ``pack_dcnv2_g8``."""
    x, offset, mask, bias = _dev(x, "input"), _dev(offset, "offset"), _dev(mask, "mask"), _dev(bias, "bias")
    n, cin, h, w = x.shape
    assert cin == 32 and tuple(offset.shape) == (n, 144, h, w) and tuple(mask.shape) == (n, 72, h, w)
    L = _lib.lib()
    out = torch.empty((n, 32, h, w), dtype=torch.float32, device=x.device)
    with _on(x, offset, mask, packed, bias):
        ws = _ws(L.crfp_dcnv2_workspace_bytes(n, 32, 32, h, w, 3, 8), x.device)
        _lib.check(L.crfp_dcnv2_g8_packed_f32(x.data_ptr(), offset.data_ptr(), mask.data_ptr(), packed.data_ptr(), bias.data_ptr(),
                                              out.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), _stream()), "crfp_dcnv2_g8_packed_f32")
    return out


def flow_warp(x, flow, interpolation="bilinear", padding_mode="zeros", align_corners=True):
    """Drop-in for the reference's ``flow_warp`` (model/CRFP.py:90-130): x[n,c,h,w], flow[n,h,w,2], forward and backward.  With grad mode
    on and ``x`` or ``flow`` requiring grad the result carries a ``grad_fn`` whose backward is crfp_flow_warp_backward_f32 (fp32, first
    order only; the gradient of ``x`` is an unordered float atomic sum, that of ``flow`` is bitwise reproducible); otherwise this is the
    plain forward call."""
    if tuple(x.shape[-2:]) != tuple(flow.shape[1:3]):
        raise ValueError(f"The spatial sizes of input ({tuple(x.shape[-2:])}) and flow "
                         f"({tuple(flow.shape[1:3])}) are not the same.")
    if interpolation != "bilinear" or not align_corners:
        raise NotImplementedError("flow_warp: only bilinear / align_corners=True (all reference call sites)")
    if padding_mode not in ("zeros", "border"):
        raise NotImplementedError(f"flow_warp: padding_mode {padding_mode!r}")
    x, flow = _dev(x, "x"), _dev(flow, "flow")
    border = 1 if padding_mode == "border" else 0
    if torch.is_grad_enabled() and (x.requires_grad or flow.requires_grad):
        return _FlowWarpFunction.apply(x, flow, border)
    return _flow_warp_forward(x, flow, border)


def _flow_warp_forward(x, flow, border):
    """crfp_flow_warp_f32 on float32, contiguous device tensors."""
    n, c, h, w = x.shape
    L = _lib.lib()
    out = torch.empty_like(x)
    nb = L.crfp_flow_warp_workspace_bytes(n, c, h, w)
    ws = _ws(nb, x.device)
    with _on(x, flow):
        _lib.check(L.crfp_flow_warp_f32(x.data_ptr(), flow.data_ptr(), out.data_ptr(), n, c, h, w,
                                        border, ws.data_ptr(), ws.numel(), _stream()),
                   "crfp_flow_warp_f32")
    return out


class _FlowWarpFunction(torch.autograd.Function):
    """``flow_warp`` under autograd: forward = ``_flow_warp_forward``, backward = crfp_flow_warp_backward_f32 with a NULL pointer for
    every gradient ``ctx.needs_input_grad`` does not ask for (and for ``x``, which only the gradient of the flow reads)."""

    @staticmethod
    def forward(ctx, x, flow, border):
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, flow)
        ctx.border = border
        ctx.shape = tuple(x.shape)
        return _flow_warp_forward(x, flow, border)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, flow = ctx.saved_tensors
        grad_out = _dev(grad_out, "grad_out")
        n, c, h, w = ctx.shape
        L = _lib.lib()
        with _on(flow, grad_out):
            gx = torch.empty_like(grad_out) if ctx.needs_input_grad[0] else None
            gflow = torch.empty_like(flow) if ctx.needs_input_grad[1] else None
            ws = _ws(L.crfp_flow_warp_backward_workspace_bytes(n, c, h, w), flow.device)
            _lib.check(L.crfp_flow_warp_backward_f32(x.data_ptr() if x is not None else None, flow.data_ptr(), grad_out.data_ptr(),
                                                     gx.data_ptr() if gx is not None else None,
                                                     gflow.data_ptr() if gflow is not None else None,
                                                     n, c, h, w, ctx.border, ws.data_ptr(), ws.numel(), _stream()),
                       "crfp_flow_warp_backward_f32")
        return gx, gflow, None


def dcnv2(x, offset, mask, weight, bias, kernel_size=3, padding=1, dilation=1, deformable_groups=1):
    """Drop-in for ``dcn_v2.DCNv2.forward`` (reference model/CRFP.py:350), forward and backward.  With grad mode on and at least one of
    the five tensors requiring grad the result carries a ``grad_fn`` whose backward is crfp_dcnv2_backward_f32 (fp32, first order only;
    grad_input is an unordered float atomic sum, the other four gradients are bitwise reproducible); otherwise this is the plain
    forward call.  ``dcnv2_shared``, ``flow_warp``, ``conv3x3``, ``conv3x3_ex``, ``upsample_bilinear``, ``avgpool2`` and ``charbonnier``
    have a backward of their own in the same mould; the other wrappers of this module (``dcnv2_g8_packed``, the ``*_packed`` /
    ``*_unpacked`` convs, ``convkxk``, ``fovea_head``, ``upsample_bilinear_ac``) are forward-only."""
    x, offset, mask = _dev(x, "input"), _dev(offset, "offset"), _dev(mask, "mask")
    weight, bias = _dev(weight, "weight"), _dev(bias, "bias")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, offset, mask, weight, bias)):
        return _DCNv2Function.apply(x, offset, mask, weight, bias, kernel_size, padding, dilation, deformable_groups)
    return _dcnv2_forward(x, offset, mask, weight, bias, kernel_size, padding, dilation, deformable_groups)


def _dcnv2_forward(x, offset, mask, weight, bias, kernel_size, padding, dilation, deformable_groups):
    """crfp_dcnv2_forward_f32 on float32, contiguous device tensors."""
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    K = kernel_size * kernel_size
    assert offset.shape[1] == 2 * deformable_groups * K, "offset channels != 2*deformable_groups*k*k"
    assert mask.shape[1] == deformable_groups * K, "mask channels != deformable_groups*k*k"
    assert weight.shape[1] == cin and tuple(offset.shape[-2:]) == (h, w) and tuple(mask.shape[-2:]) == (h, w)
    L = _lib.lib()
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    ws = _ws(L.crfp_dcnv2_workspace_bytes(n, cin, cout, h, w, kernel_size, deformable_groups), x.device)
    if (cin, cout, deformable_groups, kernel_size, padding, dilation) == (32, 32, 8, 3, 1, 1):   # MFMA fast path
        return dcnv2_g8_packed(x, offset, mask, pack_dcnv2_g8(weight), bias)
    with _on(x, offset, mask, weight, bias):
        _lib.check(L.crfp_dcnv2_forward_f32(x.data_ptr(), offset.data_ptr(), mask.data_ptr(), weight.data_ptr(),
                                            bias.data_ptr(), out.data_ptr(), n, cin, cout, h, w, kernel_size, padding,
                                            dilation, deformable_groups, ws.data_ptr(), ws.numel(), _stream()),
                   "crfp_dcnv2_forward_f32")
    return out


class _DCNv2Function(torch.autograd.Function):
    """``dcnv2`` under autograd: forward = ``_dcnv2_forward``, backward = crfp_dcnv2_backward_f32 with a NULL pointer for every gradient
    ``ctx.needs_input_grad`` does not ask for."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, kernel_size, padding, dilation, deformable_groups):
        ctx.save_for_backward(x, offset, mask, weight)
        ctx.cfg = (kernel_size, padding, dilation, deformable_groups)
        return _dcnv2_forward(x, offset, mask, weight, bias, kernel_size, padding, dilation, deformable_groups)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, offset, mask, weight = ctx.saved_tensors
        k, pad, dil, dg = ctx.cfg
        grad_out = _dev(grad_out, "grad_out")
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        L = _lib.lib()
        with _on(x, offset, mask, weight, grad_out):
            like = (x, offset, mask, weight)
            grads = [torch.empty_like(t) if need else None for t, need in zip(like, ctx.needs_input_grad[:4])]
            grads.append(torch.empty(cout, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[4] else None)
            nb = L.crfp_dcnv2_backward_workspace_bytes(n, cin, cout, h, w, k, dg)
            ws = _ws(nb, x.device)
            _lib.check(L.crfp_dcnv2_backward_f32(x.data_ptr(), offset.data_ptr(), mask.data_ptr(), weight.data_ptr(), grad_out.data_ptr(),
                                                 *(g.data_ptr() if g is not None else None for g in grads),
                                                 n, cin, cout, h, w, k, pad, dil, dg, ws.data_ptr(), ws.numel(), _stream()),
                       "crfp_dcnv2_backward_f32")
        return (*grads, None, None, None, None)


def dcnv2_shared(x, offset, mask, weight, bias):
    """DCNv2 (4 -> 4 channels, one group) with one (dy, dx) [n,2,h,w] and one mask [n,1,h,w] per pixel shared by the 9 taps: equal to
    ``dcnv2(x, offset.repeat(1, 9, 1, 1), mask.repeat(1, 9, 1, 1), ...)`` (reference model/CRFP.py:341-350) without the tiled tensors,
    forward and backward.  With grad mode on and at least one of the five tensors requiring grad the result carries a ``grad_fn`` whose
    backward is crfp_dcnv2_shared_backward_f32: the gradients of the compact offset and mask are the sums over the 9 taps, formed in
    registers (fp32, first order only; grad_input is an unordered float atomic sum, the other four are bitwise reproducible)."""
    x, offset, mask, weight, bias = _dev(x, "input"), _dev(offset, "offset"), _dev(mask, "mask"), _dev(weight, "weight"), _dev(bias, "bias")
    n, cin, h, w = x.shape
    assert tuple(offset.shape) == (n, 2, h, w) and tuple(mask.shape) == (n, 1, h, w), "dcnv2_shared: offset [n,2,h,w], mask [n,1,h,w]"
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, offset, mask, weight, bias)):
        return _DCNv2SharedFunction.apply(x, offset, mask, weight, bias)
    return _dcnv2_shared_forward(x, offset, mask, weight, bias)


def _dcnv2_shared_forward(x, offset, mask, weight, bias):
    """crfp_dcnv2_shared_f32 on float32, contiguous device tensors."""
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    L = _lib.lib()
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    with _on(x, offset, mask, weight, bias):
        nb = L.crfp_dcnv2_shared_workspace_bytes(n, cin, h, w)
        ws = _ws(max(nb, 256), x.device)
        _lib.check(L.crfp_dcnv2_shared_f32(x.data_ptr(), offset.data_ptr(), mask.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                           n, cin, cout, h, w, ws.data_ptr(), ws.numel(), _stream()), "crfp_dcnv2_shared_f32")
    return out


class _DCNv2SharedFunction(torch.autograd.Function):
    """``dcnv2_shared`` under autograd: forward = ``_dcnv2_shared_forward``, backward = crfp_dcnv2_shared_backward_f32 with a NULL pointer
    for every gradient ``ctx.needs_input_grad`` does not ask for."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias):
        ctx.save_for_backward(x, offset, mask, weight)
        return _dcnv2_shared_forward(x, offset, mask, weight, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, offset, mask, weight = ctx.saved_tensors
        grad_out = _dev(grad_out, "grad_out")
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        L = _lib.lib()
        with _on(x, offset, mask, weight, grad_out):
            like = (x, offset, mask, weight)
            grads = [torch.empty_like(t) if need else None for t, need in zip(like, ctx.needs_input_grad[:4])]
            grads.append(torch.empty(cout, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[4] else None)
            ws = _ws(L.crfp_dcnv2_shared_backward_workspace_bytes(n, cin, h, w), x.device)
            _lib.check(L.crfp_dcnv2_shared_backward_f32(x.data_ptr(), offset.data_ptr(), mask.data_ptr(), weight.data_ptr(), grad_out.data_ptr(),
                                                        *(g.data_ptr() if g is not None else None for g in grads),
                                                        n, cin, cout, h, w, ws.data_ptr(), ws.numel(), _stream()),
                       "crfp_dcnv2_shared_backward_f32")
        return tuple(grads)


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def conv3x3(x, weight, bias=None, act="none", post_scale=1.0):
    """3x3 stride-1 pad-1 convolution + bias + activation on the fp32 MFMA path (weights repacked by this call), forward and backward.
    With grad mode on and ``x``, ``weight`` or ``bias`` requiring grad the result carries a ``grad_fn`` whose backward is
    crfp_conv3x3_ex_backward_f32 (see ``conv3x3_ex``); otherwise this is the plain forward call."""
    x, weight = _dev(x, "x"), _dev(weight, "weight")
    if tuple(weight.shape) != (weight.shape[0], x.shape[1], 3, 3):   # nn.Conv2d's own error class and wording (the reference's callers see a RuntimeError)
        raise RuntimeError(f"conv3x3: weight of size {list(weight.shape)}, expected input{list(x.shape)} to have {weight.shape[1]} channels, "
                           f"but got {x.shape[1]} channels instead")
    if _needs_grad(x, weight, bias):
        return _Conv3x3ExFunction.apply(x, None, weight, None if bias is None else _dev(bias, "bias"), None, act, float(post_scale), 0, 0, True)
    with _on(x, weight):
        return conv3x3_packed(x, pack_conv3x3(weight, bias), act, post_scale)


def conv3x3_ex(x, weight, bias=None, x2=None, residual=None, act="none", post_scale=1.0, unshuffle=0, shuffle=0, out=None, out_c0=0):
    """crfp_conv3x3_ex_f32: conv3x3(cat([x, x2], 1)) + bias -> activation -> * post_scale (+ residual), with the reference's layout steps
    fused: ``unshuffle=4`` reads x [n, c, 4h, 4w] as pixel_unshuffle(x, 4) (model/CRFP.py:28-42), ``shuffle=r`` stores pixel_shuffle(., r)
    (:184-193), ``out`` / ``out_c0`` write the result into channels [out_c0, out_c0 + cout) of an existing [n, C, h, w] tensor.
    Forward and backward: with grad mode on and at least one of ``x``, ``x2``, ``weight``, ``bias``, ``residual`` requiring grad the result
    carries a ``grad_fn`` whose backward is crfp_conv3x3_ex_backward_f32 (fp32 on the exact f32-input MFMA, first order only; all gradients
    bitwise reproducible; the residual's gradient is grad_out itself).  Under grad ``out`` / ``out_c0`` raise RuntimeError (a store into
    an existing tensor has no graph node) and a residual combined with an activation raises NotImplementedError (no call site, no
    backward).  Otherwise this is the plain forward call."""
    if _needs_grad(x, x2, weight, bias, residual):
        if out is not None or out_c0:
            raise RuntimeError("conv3x3_ex: `out` / `out_c0` store into an existing tensor, which has no graph node; call it under "
                               "torch.no_grad() or without them")
        if residual is not None and act != "none":
            raise NotImplementedError(f"conv3x3_ex: no backward for a residual combined with an activation (act={act!r})")
        x, x2, weight, bias, residual = (t if t is None else _dev(t, k) for t, k in zip((x, x2, weight, bias, residual),
                                                                                        ("x", "x2", "weight", "bias", "residual")))
        return _Conv3x3ExFunction.apply(x, x2, weight, bias, residual, act, float(post_scale), int(unshuffle), int(shuffle), False)
    return _conv3x3_ex_forward(x, weight, bias, x2, residual, act, post_scale, unshuffle, shuffle, out, out_c0)


class _Conv3x3ExFunction(torch.autograd.Function):
    """``conv3x3`` / ``conv3x3_ex`` under autograd: forward = the wrapper's own plain call (``packed``: conv3x3's pack + conv3x3_packed
    route), backward = crfp_conv3x3_ex_backward_f32 with a NULL pointer for every gradient ``ctx.needs_input_grad`` does not ask for."""

    @staticmethod
    def forward(ctx, x, x2, weight, bias, residual, act, post_scale, unshuffle, shuffle, packed):
        if packed:
            with _on(x, weight):
                out = conv3x3_packed(x, pack_conv3x3(weight, bias), act, post_scale)
        else:
            out = _conv3x3_ex_forward(x, weight, bias, x2, residual, act, post_scale, unshuffle, shuffle, None, 0)
        ctx.save_for_backward(x, x2, weight, out if act != "none" else None)
        ctx.cfg = (act, post_scale, unshuffle, int(shuffle) if shuffle and shuffle > 1 else 0)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, x2, weight, out = ctx.saved_tensors
        act, post_scale, unshuffle, r = ctx.cfg
        grad_out = _dev(grad_out, "grad_out")
        n = x.shape[0]
        cin, h, w = (16 * x.shape[1], x.shape[2] // 4, x.shape[3] // 4) if unshuffle == 4 else tuple(x.shape[1:])
        cin2 = 0 if x2 is None else x2.shape[1]
        cout = weight.shape[0]
        need_x, need_x2, need_w, need_b, need_res = ctx.needs_input_grad[:5]
        need_x2 = need_x2 and x2 is not None
        gx = gx2 = gw = gb = None
        if need_x or need_x2 or need_w or need_b:
            L = _lib.lib()
            ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
            with _on(x, weight, grad_out):
                gx = torch.empty_like(x) if need_x else None
                gx2 = torch.empty_like(x2) if need_x2 else None
                gw = torch.empty_like(weight) if need_w else None
                gb = torch.empty(cout, dtype=torch.float32, device=x.device) if need_b else None
                nb = L.crfp_conv3x3_ex_backward_workspace_bytes(n, cin, cin2, cout, h, w, unshuffle, r)
                if nb == 0:
                    _lib.check(-3, "crfp_conv3x3_ex_backward_workspace_bytes")
                ws = _ws(nb, x.device)
                _lib.check(L.crfp_conv3x3_ex_backward_f32(x.data_ptr(), cin, ptr(x2), cin2, weight.data_ptr(), ptr(out), grad_out.data_ptr(),
                                                          ptr(gx), ptr(gx2), ptr(gw), ptr(gb), n, cout, h, w, ACT[act], post_scale, unshuffle, r,
                                                          ws.data_ptr(), ws.numel(), _stream()), "crfp_conv3x3_ex_backward_f32")
        return gx, gx2, gw, gb, (grad_out if need_res else None), None, None, None, None, None


def _conv3x3_ex_forward(x, weight, bias, x2, residual, act, post_scale, unshuffle, shuffle, out, out_c0):
    """crfp_conv3x3_ex_f32 (the plain forward call of ``conv3x3_ex``)."""
    x, weight = _dev(x, "x"), _dev(weight, "weight")
    n = x.shape[0]
    if unshuffle == 4:
        cin, h, w = 16 * x.shape[1], x.shape[2] // 4, x.shape[3] // 4
        assert x.shape[2] % 4 == 0 and x.shape[3] % 4 == 0, "conv3x3_ex: pixel_unshuffle(4) needs H, W divisible by 4"
    else:
        cin, h, w = x.shape[1], x.shape[2], x.shape[3]
    cin2 = 0
    if x2 is not None:
        x2 = _dev(x2, "x2")
        cin2 = x2.shape[1]
        assert tuple(x2.shape) == (n, cin2, h, w), "conv3x3_ex: x2 must match x in n, h, w"
    cout = weight.shape[0]
    if tuple(weight.shape) != (cout, cin + cin2, 3, 3):
        raise RuntimeError(f"conv3x3_ex: weight of size {list(weight.shape)}, expected input to have {weight.shape[1]} channels, "
                           f"but got {cin + cin2} channels instead")
    bias = torch.zeros(cout, dtype=torch.float32, device=x.device) if bias is None else _dev(bias, "bias")
    if residual is not None:
        residual = _dev(residual, "residual")
        assert tuple(residual.shape) == (n, cout, h, w), "conv3x3_ex: residual must be [n, cout, h, w]"
    r = int(shuffle) if shuffle and shuffle > 1 else 0
    if r:
        assert out is None, "conv3x3_ex: a pixel-shuffle store writes its own tensor"
        out = torch.empty((n, cout // (r * r), h * r, w * r), dtype=torch.float32, device=x.device)
        ctot = cout
    elif out is None:
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
        ctot = cout
    else:
        # written in place: a copy made here would never reach the caller's tensor
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()):
            raise ValueError("conv3x3_ex: `out` must be a contiguous float32 CUDA/HIP tensor (it is written in place)")
        assert out.shape[0] == n and tuple(out.shape[2:]) == (h, w), "conv3x3_ex: out must be [n, C, h, w]"
        ctot = out.shape[1]
    L = _lib.lib()
    with _on(x, weight, bias, x2, residual, out):
        nb = L.crfp_conv3x3_ex_workspace_bytes(n, cin, cin2, cout, h, w, int(unshuffle), r, int(residual is not None))
        if nb == 0:
            _lib.check(-3, "crfp_conv3x3_ex_workspace_bytes")
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        _lib.check(L.crfp_conv3x3_ex_f32(x.data_ptr(), cin, x2.data_ptr() if x2 is not None else None, cin2, weight.data_ptr(), bias.data_ptr(),
                                         residual.data_ptr() if residual is not None else None, out.data_ptr(), n, cout, h, w, ACT[act],
                                         float(post_scale), int(unshuffle), r, int(out_c0), int(ctot), ws.data_ptr(), nb, _stream()),
                   "crfp_conv3x3_ex_f32")
    return out


def conv3x3_unpacked(x, weight, bias, act="none", post_scale=1.0):
    """The one-call form (crfp_conv3x3_f32: repacks the weights inside the call) -- what a caller without a cache pays."""
    x, weight, bias = _dev(x, "x"), _dev(weight, "weight"), _dev(bias, "bias")
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    L = _lib.lib()
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    ws = _ws(L.crfp_conv3x3_workspace_bytes(n, cin, cout, h, w), x.device)
    with _on(x, weight, bias):
        _lib.check(L.crfp_conv3x3_f32(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), n, cin, cout,
                                      h, w, ACT[act], float(post_scale), ws.data_ptr(), ws.numel(), _stream()),
                   "crfp_conv3x3_f32")
    return out


def upsample_bilinear(x, scale_factor=None, size=None, mul=1.0):
    """nn.Upsample(scale_factor=.., 'bilinear', align_corners=False) or F.interpolate(size=..), times ``mul``; forward and backward.  With
    grad mode on and ``x`` requiring grad the result carries a ``grad_fn`` whose backward is crfp_upsample_bilinear_backward_f32 (fp32,
    first order only, bitwise reproducible); otherwise this is the plain forward call."""
    x = _dev(x, "x")
    n, c, h, w = x.shape
    if scale_factor is not None:
        oh, ow = int(h * scale_factor), int(w * scale_factor)
        sh = sw = 1.0 / float(scale_factor)
    else:
        oh, ow = size
        # PyTorch computes in/out in float32 when only a size is given
        sh = float(torch.tensor(h, dtype=torch.float32) / torch.tensor(oh, dtype=torch.float32))
        sw = float(torch.tensor(w, dtype=torch.float32) / torch.tensor(ow, dtype=torch.float32))
    if _needs_grad(x):
        return _UpsampleBilinearFunction.apply(x, int(oh), int(ow), sh, sw, float(mul))
    return _upsample_bilinear_forward(x, oh, ow, sh, sw, mul)


def _upsample_bilinear_forward(x, oh, ow, sh, sw, mul):
    """crfp_upsample_bilinear_f32 on a float32, contiguous device tensor."""
    n, c, h, w = x.shape
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    with _on(x):
        _lib.check(_lib.lib().crfp_upsample_bilinear_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, oh, ow, sh, sw,
                                                         float(mul), _stream()), "crfp_upsample_bilinear_f32")
    return out


class _UpsampleBilinearFunction(torch.autograd.Function):
    """``upsample_bilinear`` under autograd: forward = ``_upsample_bilinear_forward``, backward = crfp_upsample_bilinear_backward_f32."""

    @staticmethod
    def forward(ctx, x, oh, ow, sh, sw, mul):
        ctx.cfg = (tuple(x.shape), oh, ow, sh, sw, mul)
        return _upsample_bilinear_forward(x, oh, ow, sh, sw, mul)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (n, c, h, w), oh, ow, sh, sw, mul = ctx.cfg
        grad_out = _dev(grad_out, "grad_out")
        gx = torch.empty((n, c, h, w), dtype=torch.float32, device=grad_out.device)
        with _on(grad_out):
            _lib.check(_lib.lib().crfp_upsample_bilinear_backward_f32(grad_out.data_ptr(), gx.data_ptr(), n, c, h, w, oh, ow, sh, sw, mul,
                                                                      _stream()), "crfp_upsample_bilinear_backward_f32")
        return gx, None, None, None, None, None


def sq_err_sums(a, b):
    """(sum (a-b)^2, sum (Y(a)-Y(b))^2) as float64 -- raw material of psnr / psnr_y."""
    a, b = _dev(a, "a"), _dev(b, "b")
    n, c, h, w = a.shape
    acc = torch.zeros(2, dtype=torch.float64, device=a.device)
    with _on(a, b):
        _lib.check(_lib.lib().crfp_psnr_partial_f32(a.data_ptr(), b.data_ptr(), acc.data_ptr(), n, c, h, w, _stream()),
                   "crfp_psnr_partial_f32")
    return acc


def avgpool2(x):
    """nn.AvgPool2d(2, 2) (floor mode) on an NCHW tensor, forward and backward.  With grad mode on and ``x`` requiring grad the result
    carries a ``grad_fn`` whose backward is crfp_avgpool2_backward_f32; otherwise this is the plain forward call."""
    x = _dev(x, "x")
    if _needs_grad(x):
        return _AvgPool2Function.apply(x)
    return _avgpool2_forward(x)


def _avgpool2_forward(x):
    """crfp_avgpool2_f32 on a float32, contiguous device tensor."""
    n, c, h, w = x.shape
    out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    with _on(x):
        _lib.check(_lib.lib().crfp_avgpool2_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, _stream()), "crfp_avgpool2_f32")
    return out


class _AvgPool2Function(torch.autograd.Function):
    """``avgpool2`` under autograd: forward = ``_avgpool2_forward``, backward = crfp_avgpool2_backward_f32."""

    @staticmethod
    def forward(ctx, x):
        ctx.shape = tuple(x.shape)
        return _avgpool2_forward(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        n, c, h, w = ctx.shape
        grad_out = _dev(grad_out, "grad_out")
        gx = torch.empty((n, c, h, w), dtype=torch.float32, device=grad_out.device)
        with _on(grad_out):
            _lib.check(_lib.lib().crfp_avgpool2_backward_f32(grad_out.data_ptr(), gx.data_ptr(), n, c, h, w, _stream()),
                       "crfp_avgpool2_backward_f32")
        return gx


def charbonnier(pred, target, weight=None, eps=1e-12):
    """The raw material of the reference's masked Charbonnier loss (loss/loss.py:26-68,115-124) in one pass: ``sums[n, 2]`` (float64, on the
    device) = per sample (sum sqrt((pred - target)^2 + eps) * weight, sum weight), the weight [n,1,h,w] or [n,c,h,w] expanded over the
    channels (none: the second column is the element count).  Forward and backward: with grad mode on and ``pred`` or ``target`` requiring
    grad the result carries a ``grad_fn`` whose backward is crfp_charbonnier_backward_f32 on the upstream gradient of ``sums[:, 0]`` (the
    gradient of ``target`` is the negation of ``pred``'s; the weight gets none).  crfp_amd.loss builds the reductions on it."""
    pred, target = _dev(pred, "pred"), _dev(target, "target")
    if pred.dim() != 4 or tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"charbonnier: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be the same [n, c, h, w]")
    if weight is not None:
        weight = _dev(weight, "weight")
        n, c, h, w = pred.shape
        if tuple(weight.shape) not in ((n, 1, h, w), (n, c, h, w)):
            raise ValueError(f"charbonnier: weight {tuple(weight.shape)} must be [n, 1, h, w] or [n, c, h, w]")
    if _needs_grad(pred, target):
        return _CharbonnierFunction.apply(pred, target, weight, float(eps))
    return _charbonnier_forward(pred, target, weight, float(eps))


def _charbonnier_forward(pred, target, weight, eps):
    """crfp_charbonnier_f32 on float32, contiguous device tensors."""
    n, c, h, w = pred.shape
    L = _lib.lib()
    sums = torch.empty((n, 2), dtype=torch.float64, device=pred.device)
    with _on(pred, target, weight):
        nb = L.crfp_charbonnier_workspace_bytes(n, c, h, w)
        if nb == 0:
            _lib.check(-3, "crfp_charbonnier_workspace_bytes")
        ws = _ws(nb, pred.device)
        _lib.check(L.crfp_charbonnier_f32(pred.data_ptr(), target.data_ptr(), None if weight is None else weight.data_ptr(),
                                          0 if weight is None else weight.shape[1], sums.data_ptr(), n, c, h, w, eps, ws.data_ptr(), ws.numel(),
                                          _stream()), "crfp_charbonnier_f32")
    return sums


class _CharbonnierFunction(torch.autograd.Function):
    """``charbonnier`` under autograd: forward = ``_charbonnier_forward``, backward = crfp_charbonnier_backward_f32 with scale = the upstream
    gradient of sums[:, 0] (float32, made on the device: no host sync)."""

    @staticmethod
    def forward(ctx, pred, target, weight, eps):
        ctx.save_for_backward(pred, target, weight)
        ctx.eps = eps
        return _charbonnier_forward(pred, target, weight, eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_sums):
        pred, target, weight = ctx.saved_tensors
        n, c, h, w = pred.shape
        scale = grad_sums[:, 0].to(torch.float32).contiguous()
        gp = torch.empty_like(pred)
        with _on(pred, target, weight, scale):
            _lib.check(_lib.lib().crfp_charbonnier_backward_f32(pred.data_ptr(), target.data_ptr(), None if weight is None else weight.data_ptr(),
                                                                0 if weight is None else weight.shape[1], scale.data_ptr(), gp.data_ptr(),
                                                                n, c, h, w, ctx.eps, _stream()), "crfp_charbonnier_backward_f32")
        return (gp if ctx.needs_input_grad[0] else None), (-gp if ctx.needs_input_grad[1] else None), None, None


def fovea_head(state, x_hr, mask, lr, w_tttf, b_tttf, w_last, b_last, y_only=False):
    """Fused fovea fusion + output head (model/CRFP.py:1672-1684) -> (new_state [n,4,8h,8w], out [n,3|1,8h,8w])."""
    state, x_hr, lr = _dev(state, "state"), _dev(x_hr, "x_hr"), _dev(lr, "lr")
    w_tttf, b_tttf, w_last, b_last = (_dev(t, "weights") for t in (w_tttf, b_tttf, w_last, b_last))
    n, _, h, w = lr.shape
    H, W = 8 * h, 8 * w
    if tuple(state.shape) != (n, 4, H, W) or tuple(x_hr.shape) != (n, 4, H, W):
        raise ValueError("state / x_hr must be [n,4,8h,8w]")
    m8 = (mask != 0 if mask.dtype != torch.bool else mask).to(state.device).expand(n, 1, H, W).contiguous().view(torch.uint8)
    L = _lib.lib()
    ws = torch.empty(L.crfp_fovea_head_workspace_bytes(n, h, w), dtype=torch.uint8, device=state.device)
    new_state = torch.empty_like(state)
    out = torch.empty((n, 1 if y_only else 3, H, W), dtype=torch.float32, device=state.device)
    with _on(state, x_hr, lr, w_tttf, b_tttf, w_last, b_last):
        _lib.check(L.crfp_fovea_head_f32(state.data_ptr(), x_hr.data_ptr(), m8.data_ptr(), lr.data_ptr(), w_tttf.data_ptr(),
                                         b_tttf.data_ptr(), w_last.data_ptr(), b_last.data_ptr(), new_state.data_ptr(),
                                         out.data_ptr(), n, h, w, int(bool(y_only)), ws.data_ptr(), ws.numel(), _stream()),
                   "crfp_fovea_head_f32")
    return new_state, out


def upsample_bilinear_ac(x, scale_factor, mul=1.0):
    """F.interpolate(x, scale_factor=.., mode='bilinear', align_corners=True) * mul (SPyNet's flow upsampling)."""
    x = _dev(x, "x")
    n, c, h, w = x.shape
    oh, ow = int(h * scale_factor), int(w * scale_factor)
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    with _on(x):
        _lib.check(_lib.lib().crfp_upsample_bilinear_ac_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, oh, ow, float(mul), _stream()),
                   "crfp_upsample_bilinear_ac_f32")
    return out


def convkxk(x, weight, bias, pre_relu=False):
    """k x k stride-1 'same' convolution (k in 3, 5, 7), optional ReLU on the input (reference `conv`, model/CRFP.py:145-152)."""
    x, weight, bias = _dev(x, "x"), _dev(weight, "weight"), _dev(bias, "bias")
    n, cin, h, w = x.shape
    cout, cin_w, k, k2 = weight.shape
    assert cin_w == cin and k == k2
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    with _on(x, weight, bias):
        _lib.check(_lib.lib().crfp_convkxk_f32(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), n, cin, cout, h, w,
                                               k, int(bool(pre_relu)), _stream()), "crfp_convkxk_f32")
    return out


def spynet_forward(params, ref, supp):
    """SPyNet.forward(ref, supp) (reference model/CRFP.py:698-741) in one native call; params = the 60 conv tensors in
    state_dict order."""
    import ctypes as C
    ref, supp = _dev(ref, "ref"), _dev(supp, "supp")
    if len(params) != 60:
        raise ValueError(f"SPyNet has 60 conv parameters, got {len(params)}")
    keep = [_dev(p.detach(), "params") for p in params]
    n, c, h, w = ref.shape
    assert c == 3 and tuple(supp.shape) == tuple(ref.shape)
    L = _lib.lib()
    ptrs = (C.c_void_p * 60)(*[t.data_ptr() for t in keep])
    ws = _ws(L.crfp_spynet_workspace_bytes(n, h, w), ref.device)
    flow = torch.empty((n, 2, h, w), dtype=torch.float32, device=ref.device)
    with _on(ref, supp, *keep):
        _lib.check(L.crfp_spynet_forward(ptrs, ref.data_ptr(), supp.data_ptr(), flow.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(),
                                         _stream()), "crfp_spynet_forward")
    return flow


def _probe_desc(spec, n, h, w, dev, keep, own_sources, want_raw, elem_bytes):
    """crfp_probe_conv for one conv of a conv_probe call -> (struct, destination tensors, raw tensors)."""
    d = _lib.ProbeConv()
    srcs = spec.get("srcs", []) if own_sources else []
    d.nsrc = len(srcs)
    cin = 0
    for i, s in enumerate(srcs):
        kind, t = s[0], _dev(s[1], f"srcs[{i}]")
        keep.append(t)
        nch = {"q4": t.shape[1], "unshuf4": 16 * t.shape[1], "flow2": 2}[kind]
        want = {"q4": (n, nch, h, w), "unshuf4": (n, nch // 16, 4 * h, 4 * w), "flow2": (n, h, w, 2)}[kind]
        assert tuple(t.shape) == want, f"conv_probe: source {i} ({kind}) is {tuple(t.shape)}, expected {want}"
        d.src[i], d.src_kind[i], d.src_nch[i], d.src_pad[i] = t.data_ptr(), _lib.PROBE_SRC[kind], nch, int(s[2]) if len(s) > 2 else 0
        cin += nch
    for name in ("weight", "bias", "weight2", "bias2", "residual", "flow"):
        t = spec.get(name)
        if t is not None:
            t = _dev(t, name)
            keep.append(t)
            setattr(d, name, t.data_ptr())
    cout = spec["weight"].shape[0] + (spec["weight2"].shape[0] if spec.get("weight2") is not None else 0)
    d.cout, d.cout_split = cout, spec["weight"].shape[0] if spec.get("weight2") is not None else 0
    store = spec.get("store", "q4")
    d.store, d.ps_r, d.act, d.post_scale = _lib.PROBE_STORE[store], int(spec.get("ps_r", 0)), ACT[spec.get("act", "none")], float(spec.get("post_scale", 1.0))
    d.n_off_quads, d.strict, d.dst_f32 = int(spec.get("n_off_quads", 0)), int(bool(spec.get("strict"))), int(bool(spec.get("dst_f32")))
    outs, raws = [], []
    if store == "ps":
        r = d.ps_r
        dsts = [(0, 0, 0)]
        shapes = [(n, cout // (r * r), h * r, w * r)]
    else:
        ncq = (cout + 3) // 4
        dsts = spec.get("dsts")
        dsts = [(0, ncq, 0)] if dsts is None else [tuple(x) + (0,) * (3 - len(x)) for x in dsts]
        shapes = [(n, min(4 * q1, cout) - 4 * q0, h, w) for q0, q1, _ in dsts]
    d.ndst = len(dsts)
    for i, ((q0, q1, pad), shp) in enumerate(zip(dsts, shapes)):
        o = torch.empty(shp, dtype=torch.float32, device=dev)
        outs.append(o)
        d.dst[i], d.dst_q0[i], d.dst_q1[i], d.dst_pad[i] = o.data_ptr(), q0, q1, pad
        if want_raw and store == "q4":
            eb = 4 if d.dst_f32 else elem_bytes
            rw = torch.empty(n * (q1 - q0) * (h + pad) * (w + pad) * 4 * eb, dtype=torch.uint8, device=dev)
            raws.append(rw)
            d.dst_raw[i] = rw.data_ptr()
    return d, outs, raws


def conv_probe(a, b=None, mode="single", storage="f32", raw=False):
    """Test hook (crfp_conv_probe / crfp_conv_probe_bf16): one launch of the engines' own MFMA conv kernels on the caller's tensors.

    ``a`` / ``b`` describe a conv each: ``srcs`` = [(kind, tensor[, pad])] with kind "q4" ([n, c, h, w]), "unshuf4" ([n, c, 4h, 4w]) or
    "flow2" ([n, h, w, 2]); ``weight`` / ``bias`` (and ``weight2`` / ``bias2`` for the rows behind them); ``residual``; ``flow``;
    ``store`` "q4" (``dsts`` = [(q0, q1[, pad])] quad ranges, default one destination with everything), "ps" (``ps_r``) or "offmask"
    (``n_off_quads``); ``act``, ``post_scale``, ``strict``, ``dst_f32``.  mode: "single", "dual" (a and b side by side), "pair" (bf16: a
    feeds b in one launch), "pair_f32" (the same through the fp32 build's pair kernel) or "s3_chain" (fp32: a's output reaches b as the pre-split fp16 image; give a ``dsts=[]``).
    Returns a dict: ``out`` (per conv, the list of its destination tensors, NCHW fp32; elements no lane wrote are NaN), ``status``
    (int32 [2, n]: the range-guard word of every batch item, per conv), ``kernel`` (the variant names the launcher chose, per conv),
    ``raw`` (with raw=True: per conv the raw bytes of each "q4" destination, pads included)."""
    import ctypes as C
    L = _lib.lib()
    sfx = "_bf16" if storage == "bf16" else ""
    first = a["srcs"][0]
    t0 = first[1]
    if first[0] == "flow2":
        n, h, w = t0.shape[0], t0.shape[1], t0.shape[2]
    else:
        n, h, w = t0.shape[0], t0.shape[2] // (4 if first[0] == "unshuf4" else 1), t0.shape[3] // (4 if first[0] == "unshuf4" else 1)
    dev = t0.device
    keep = []
    eb = 2 if storage == "bf16" else 4
    da, outs_a, raws_a = _probe_desc(a, n, h, w, dev, keep, True, raw, eb)
    if b is not None:
        db, outs_b, raws_b = _probe_desc(b, n, h, w, dev, keep, mode == "dual", raw, eb)
    m = _lib.PROBE_MODES[mode]
    pa, pb = C.byref(da), (C.byref(db) if b is not None else None)
    with _on(*keep):
        nb = getattr(L, "crfp_conv_probe_workspace_bytes" + sfx)(m, pa, pb, n, h, w)
        if nb == 0:
            _lib.check(-1, "crfp_conv_probe_workspace_bytes" + sfx)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        status = torch.zeros((2, n), dtype=torch.int32, device=dev)
        kern = (C.c_int * 2)()
        _lib.check(getattr(L, "crfp_conv_probe" + sfx)(m, pa, pb, n, h, w, status.data_ptr(), kern, ws.data_ptr(), nb, _stream()),
                   "crfp_conv_probe" + sfx)
        torch.cuda.current_stream().synchronize()   # the workspace goes away with this call
    res = {"out": [outs_a] + ([outs_b] if b is not None else []), "status": status,
           "kernel": tuple(_lib.CONV_KERNELS[k] for k in kern)}
    if raw:
        res["raw"] = [raws_a] + ([raws_b] if b is not None else [])
    return res


def _narrow_desc(spec, n, h, w, dev, keep, last, want_raw, elem_bytes):
    """crfp_narrow_stencil for one stencil of a narrow_probe call -> (struct, dst, dst2, raw, raw2); tensors only where `dev` is given."""
    d = _lib.NarrowStencil()
    srcs = spec.get("srcs", [])
    d.nsrc = len(srcs)
    for i, s in enumerate(srcs[:3]):
        kind, t = s[0], s[1]
        if isinstance(t, torch.Tensor):
            t = _dev(t, f"srcs[{i}]")
            want = (n, t.shape[1], h, w) if kind == "q4" else (n, h, w, 2)
            assert tuple(t.shape) == want, f"narrow_probe: source {i} ({kind}) is {tuple(t.shape)}, expected {want}"
            keep.append(t)
            d.src[i], nch = t.data_ptr(), (t.shape[1] if kind == "q4" else 2)
        else:   # plan only: the channel count stands for the tensor
            nch = int(t)
        d.src_kind[i], d.src_nch[i] = _lib.PROBE_SRC[kind], nch
    for name in ("weight", "bias", "weight2", "bias2", "residual", "flow", "base_lr", "mask"):
        t = spec.get(name)
        if isinstance(t, torch.Tensor):
            t = _dev(t, name, torch.uint8 if name == "mask" else torch.float32)
            keep.append(t)
            setattr(d, name, t.data_ptr())
    if isinstance(spec.get("weight"), torch.Tensor):
        cout = spec["weight"].shape[0] + (spec["weight2"].shape[0] if spec.get("weight2") is not None else 0)
        split = spec["weight"].shape[0] if spec.get("weight2") is not None else 0
    else:
        cout, split = int(spec["cout"]), int(spec.get("cout_split", 0))
    d.cout, d.cout_split = cout, split
    d.act, d.post_scale, d.epi = ACT[spec.get("act", "none")], float(spec.get("post_scale", 1.0)), _lib.NARROW_EPI[spec.get("epi", "plain")]
    d.y_only, d.src_pad, d.dst_pad = int(bool(spec.get("y_only"))), int(spec.get("src_pad", 0)), int(spec.get("dst_pad", 0))
    d.gate_h = -1 if spec.get("gate_h") is None else int(spec["gate_h"])
    d.dst2_on = int(bool(spec.get("dst2")))
    out = out2 = raw = raw2 = None
    if last and dev is not None:
        epi = spec.get("epi", "plain")
        out = torch.empty((n, (1 if d.y_only else 3) if epi == "last" else 4, h, w), dtype=torch.float32, device=dev)
        d.dst = out.data_ptr()
        if want_raw and epi != "last":
            eb = 4 if epi == "offmask3" else elem_bytes
            raw = torch.empty(n * (h + d.dst_pad) * (w + d.dst_pad) * 4 * eb, dtype=torch.uint8, device=dev)
            d.dst_raw = raw.data_ptr()
        if d.dst2_on:
            out2 = torch.empty((n, 4, h, w), dtype=torch.float32, device=dev)
            d.dst2 = out2.data_ptr()
            if want_raw:
                raw2 = torch.empty(n * (h + 1) * (w + 1) * 4 * elem_bytes, dtype=torch.uint8, device=dev)
                d.dst2_raw = raw2.data_ptr()
    return d, out, out2, raw, raw2


def _narrow_report(r):
    return {"kernel": _lib.NARROW_KERNELS[r.kernel], "kq": r.kq, "epi": {v: k for k, v in _lib.NARROW_EPI.items()}[r.epi], "gate": bool(r.gate),
            "st2": bool(r.st2), "kqg": r.kqg, "res": bool(r.res), "tiles": r.tiles, "workgroups": r.workgroups}


def narrow_probe_plan(a, b=None, c=None, mode="single", storage="f32", res=False, n=1, h=1, w=1):
    """crfp_narrow_probe_plan: what narrow_probe would report for the same stencils on an [n, ., h, w] map, on the host alone.  Sources are
    given as (kind, channels), weights as ``cout`` (and ``cout_split``)."""
    import ctypes as C
    L = _lib.lib()
    sfx = "_bf16" if storage == "bf16" else ""
    specs = [s for s in (a, b, c) if s is not None]
    ds = [_narrow_desc(s, n, h, w, None, [], i == len(specs) - 1, False, 0)[0] for i, s in enumerate(specs)]
    ps = [C.byref(d) for d in ds] + [None] * (3 - len(ds))
    rep = _lib.NarrowReport()
    _lib.check(getattr(L, "crfp_narrow_probe_plan" + sfx)(_lib.NARROW_MODES[mode], *ps, int(bool(res)), n, h, w, C.byref(rep)), "crfp_narrow_probe_plan" + sfx)
    return _narrow_report(rep)


def narrow_probe(a, b=None, c=None, mode="single", storage="f32", res=False, status=None, raw=False):
    """Test hook (crfp_narrow_probe / crfp_narrow_probe_bf16): one launch of the engines' own 8x narrow conv kernels on the caller's tensors.

    ``a`` / ``b`` / ``c`` describe a 3x3 stencil each: ``srcs`` = [(kind, tensor)] with kind "q4" ([n, c <= 4, h, w]) or "flow2" ([n, h, w, 2]);
    ``weight`` / ``bias`` (and ``weight2`` / ``bias2`` for the rows behind them); ``act``, ``post_scale``, ``residual`` [n, 4, h, w]; ``epi``
    "plain" / "blend" (``mask`` uint8 [n, 1, h, w]) / "last" (``base_lr`` [n, 3, h / 8, w / 8], ``y_only``) / "offmask3" (``flow``);
    ``src_pad`` / ``dst_pad`` (0, 1 = padded planes, p > 1 = a window inside planes p wider); ``dst2`` (the second destination); ``gate_h``
    (0 .. 3: the mask-gated form over ``mask``).  mode "single", "pair" (a feeds b) or "chain" (a -> b -> c; ``res``: c adds a's output).
    ``status``: int32 [n], the range-guard words before the launch.  Returns a dict: ``out`` (the last stencil's destination, NCHW fp32; elements
    no lane wrote are NaN), ``out2``, ``status`` (int32 [n] after the launch), ``report`` (kernel family, template arguments, tiles and
    workgroups per batch item), and with raw=True ``raw`` / ``raw2`` (the raw bytes of the destinations, pads included)."""
    import ctypes as C
    L = _lib.lib()
    sfx = "_bf16" if storage == "bf16" else ""
    first = a["srcs"][0]
    t0 = first[1]
    n, h, w = (t0.shape[0], t0.shape[1], t0.shape[2]) if first[0] == "flow2" else (t0.shape[0], t0.shape[2], t0.shape[3])
    dev = t0.device
    keep = []
    specs = [s for s in (a, b, c) if s is not None]
    eb = 2 if storage == "bf16" else 4
    descs = [_narrow_desc(s, n, h, w, dev, keep, i == len(specs) - 1, raw, eb) for i, s in enumerate(specs)]
    ps = [C.byref(d[0]) for d in descs] + [None] * (3 - len(descs))
    m = mode if isinstance(mode, int) else _lib.NARROW_MODES[mode]
    with _on(*keep):
        nb = getattr(L, "crfp_narrow_probe_workspace_bytes" + sfx)(m, *ps, int(bool(res)), n, h, w)
        if nb == 0:
            _lib.check(-1, "crfp_narrow_probe_workspace_bytes" + sfx)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        st_in = None if status is None else _dev(status, "status", torch.int32)
        st_out = torch.zeros(n, dtype=torch.int32, device=dev)
        rep = _lib.NarrowReport()
        _lib.check(getattr(L, "crfp_narrow_probe" + sfx)(m, *ps, int(bool(res)), n, h, w, None if st_in is None else st_in.data_ptr(), st_out.data_ptr(),
                                                         C.byref(rep), ws.data_ptr(), nb, _stream()), "crfp_narrow_probe" + sfx)
        torch.cuda.current_stream().synchronize()   # the workspace goes away with this call
    _, out, out2, rw, rw2 = descs[-1]
    result = {"out": out, "out2": out2, "status": st_out, "report": _narrow_report(rep)}
    if raw:
        result["raw"], result["raw2"] = rw, rw2
    return result


def _gather_report(r):
    return {"kernel": _lib.GATHER_KERNELS[r.kernel], "cus": r.cus, "tiles": r.tiles, "persistent": bool(r.persistent), "split": bool(r.split),
            "out_stride": r.out_stride, "out2_stride": r.out2_stride}


def gather_probe_plan(mode, n, h, w, c=32, storage="f32"):
    """crfp_gather_probe_plan: what gather_probe would report for an [n, ., h, w] launch of `mode`, on the host alone (the fused DCN launch asks
    the current device for its CU count)."""
    import ctypes as C
    L = _lib.lib()
    sfx = "_bf16" if storage == "bf16" else ""
    a = _lib.GatherArgs(mode=_lib.GATHER_MODES[mode], c=c, n=n, h=h, w=w)
    rep = _lib.GatherReport()
    _lib.check(getattr(L, "crfp_gather_probe_plan" + sfx)(C.byref(a), C.byref(rep)), "crfp_gather_probe_plan" + sfx)
    return _gather_report(rep)


def gather_probe(mode, x, storage="f32", raw=False, x2=None, aux=None, mask=None, flow=None, head_w=None, head_b=None, weight=None, bias=None):
    """Test hook (crfp_gather_probe / crfp_gather_probe_bf16): one launch of the engines' own gather kernels on the caller's NCHW fp32 tensors.

    mode "warp" (x [n, 4 | 24 | 32, h, w], flow [n, h, w, 2]), "warp_dual" (x 32 and x2 24 channels, one flow), "dcn_g8" (x 32, aux = offsets
    [n, 144, h, w], mask [n, 72, h, w], weight, bias), "dcn_fused" (aux = the offset feature [n, 32, h, w], flow, head_w [216, 32, 3, 3], head_b,
    weight, bias), "dcn3" (x 4, aux [n, 3, h, w] = (dy, dx, mask), weight [4, 4, 3, 3], bias) or "dcn3_fused" (aux = the head's input [n, 4, h, w],
    flow, head_w [3, 4, 3, 3], head_b, weight, bias).  Returns a dict: ``out`` (NCHW fp32; elements no lane wrote are NaN), ``out2`` (warp_dual),
    ``status`` (int32 [n]: the range-guard word of every batch item), ``report`` (the kernel taken, the fused launch's sizing, the raw strides),
    and with raw=True ``raw`` / ``raw2``: the destinations' raw bytes as uint8 [n, stride in bytes], an item's map first, then its slack."""
    import ctypes as C
    L = _lib.lib()
    sfx = "_bf16" if storage == "bf16" else ""
    eb = 2 if storage == "bf16" else 4
    x = _dev(x, "x")
    n, c, h, w = x.shape
    dev = x.device
    keep = [x]

    def ptr(t, name):
        if t is None:
            return None
        t = _dev(t, name)
        keep.append(t)
        return t.data_ptr()

    a = _lib.GatherArgs(mode=_lib.GATHER_MODES[mode], c=c, n=n, h=h, w=w, x=x.data_ptr(), x2=ptr(x2, "x2"), aux=ptr(aux, "aux"), mask=ptr(mask, "mask"),
                        flow=ptr(flow, "flow"), head_w=ptr(head_w, "head_w"), head_b=ptr(head_b, "head_b"), weight=ptr(weight, "weight"),
                        bias=ptr(bias, "bias"))
    with _on(*keep):
        plan = _lib.GatherReport()
        _lib.check(getattr(L, "crfp_gather_probe_plan" + sfx)(C.byref(a), C.byref(plan)), "crfp_gather_probe_plan" + sfx)
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)
        out2 = torch.empty((n, 24, h, w), dtype=torch.float32, device=dev) if mode == "warp_dual" else None
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        a.out, a.out2, a.status = out.data_ptr(), None if out2 is None else out2.data_ptr(), status.data_ptr()
        rw = rw2 = None
        if raw:
            rw = torch.empty((n, plan.out_stride * eb), dtype=torch.uint8, device=dev)
            a.out_raw = rw.data_ptr()
            if out2 is not None:
                rw2 = torch.empty((n, plan.out2_stride * eb), dtype=torch.uint8, device=dev)
                a.out2_raw = rw2.data_ptr()
        nb = getattr(L, "crfp_gather_probe_workspace_bytes" + sfx)(C.byref(a))
        if nb == 0:
            _lib.check(-1, "crfp_gather_probe_workspace_bytes" + sfx)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        rep = _lib.GatherReport()
        _lib.check(getattr(L, "crfp_gather_probe" + sfx)(C.byref(a), C.byref(rep), ws.data_ptr(), nb, _stream()), "crfp_gather_probe" + sfx)
        torch.cuda.current_stream().synchronize()   # the workspace goes away with this call
    result = {"out": out, "out2": out2, "status": status, "report": _gather_report(rep)}
    if raw:
        result["raw"], result["raw2"] = rw, rw2
    return result
