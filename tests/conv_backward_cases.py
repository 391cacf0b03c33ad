"""The cases of the conv3x3 backward (crfp_conv3x3_ex_backward_f32 / ops.conv3x3 and ops.conv3x3_ex under autograd), their float64
references, and the module graphs of tests/test_gpu_conv_backward.py.

Reference: torch.autograd.grad on CPU float64 tensors holding the cases' float32 values, with a random grad_out, through
F.pixel_unshuffle -> cat -> F.conv2d(padding=1) -> act -> * s -> + residual -> F.pixel_shuffle.  The ``out`` handed to the C-ABI is that
float64 forward rounded to float32.  ``reference_from_out(name, out)`` is the same gradient with the activation's derivative taken from a
given ``out`` (the backward's own contract: relu / lrelu the sign of out, tanh 1 - (out/s)^2, sigmoid (out/s)(1 - out/s)): gz in float64,
then autograd through the linear part.  It is what ops.conv3x3_ex under autograd is compared with, on the forward kernel's own output:
the forward's split-fp16 error is not the backward's to answer for.

A condition on the inputs (pinned by tests/test_conv_backward_cases.py): in every relu / lrelu case every float64 pre-activation has
|z| >= 2e-4 max|z|, about 7x the forward operator's 3e-5 bound, so that float32, float64 and the split-fp16 forward pick the same branch.
A plain draw of some ten thousand pre-activations never meets it (each falls below with probability ~6e-4), so the bias of each output
channel is stepped away from its drawn value in steps of 0.003 until the channel does (``_condition_bias``), with twice the margin.

Tolerance (per case and gradient tensor): max|got - ref64| <= TOL * max|ref64| with TOL = 8 * max(E32, 2^-23).  E32 is the float32 CPU
graph's own error against float64 (``measure_e32``), written down below; 8 is the project's margin for a different summation order and
2^-23 one float32 ulp.
"""
import functools

import torch
import torch.nn.functional as F

import dcn_backward_cases as dc
from oracle import crfp_oracle as orc

GRADS = ("x", "x2", "weight", "bias", "residual")
ULP = 2.0 ** -23
ZMIN = 2e-4   # the |z| condition

# name -> n, cin (after the unshuffle), cin2, cout, h, w (the conv's), act, post_scale, residual, shuffle r, unshuffle r
CASES = {
    "odd":        dict(n=2, cin=5, cin2=3, cout=7, h=9, w=11, act="lrelu", s=0.5),      # nothing tile-aligned, two inputs
    "cat66":      dict(n=1, cin=32, cin2=34, cout=32, h=20, w=36, act="lrelu", s=1.0),  # dcn_block.0's counts: two channel groups, cin2 % 4 != 0
    "tanh":       dict(n=1, cin=8, cin2=0, cout=18, h=10, w=13, act="tanh", s=10.0),    # the offset head; some outputs saturated
    "sigmoid":    dict(n=1, cin=8, cin2=0, cout=9, h=10, w=13, act="sigmoid", s=1.0),   # the mask head
    "resid":      dict(n=2, cin=8, cin2=0, cout=8, h=9, w=11, act="none", s=0.7, resid=True),   # grad_residual is grad_out
    "shuffle2":   dict(n=1, cin=16, cin2=0, cout=12, h=7, w=10, act="relu", s=1.0, shuffle=2),   # inverse-shuffle read of grad_out and out
    "shuffle4":   dict(n=1, cin=8, cin2=0, cout=32, h=5, w=6, act="none", s=1.0, shuffle=4),
    "unshuffle4": dict(n=1, cin=32, cin2=0, cout=9, h=5, w=7, act="none", s=1.0, unshuffle=4),   # x [1,2,20,28]: scatter of grad_x, unshuffle read
    "wide":       dict(n=1, cin=4, cin2=4, cout=4, h=6, w=150, act="none", s=1.0),      # three 64-pixel tiles per row, tail tile
    "slabs":      dict(n=3, cin=4, cin2=0, cout=4, h=33, w=47, act="lrelu", s=1.0),     # J > 1 slabs of several tiles, tail tiles, batch stride
    "line":       dict(n=1, cin=3, cin2=0, cout=3, h=1, w=7, act="none", s=1.0),        # every tap but the centre row is padding
    "column":     dict(n=1, cin=3, cin2=0, cout=3, h=6, w=1, act="none", s=1.0),        # ... the centre column
}
SIGNED = tuple(k for k, c in CASES.items() if c["act"] in ("relu", "lrelu"))
ONE_INPUT = tuple(k for k, c in CASES.items() if not (c["cin2"] or c.get("resid") or c.get("shuffle") or c.get("unshuffle")))   # ops.conv3x3 takes them


def tensors(name):
    """the gradient tensors the case has"""
    c = CASES[name]
    return tuple(k for k in GRADS if not (k == "x2" and not c["cin2"]) and not (k == "residual" and not c.get("resid")))


# E32[case][tensor]: max|float32 CPU graph - float64| / max|float64| of that gradient (measure_e32; torch 2.x CPU kernels).
E32 = {
    "odd":        dict(x=3.16e-07, x2=2.22e-07, weight=2.37e-07, bias=2.01e-07),
    "cat66":      dict(x=3.14e-07, x2=3.83e-07, weight=5.49e-07, bias=6.71e-07),
    "tanh":       dict(x=3.63e-07, weight=6.85e-07, bias=3.08e-07),
    "sigmoid":    dict(x=1.32e-07, weight=3.72e-07, bias=4.90e-08),
    "resid":      dict(x=2.24e-07, weight=3.37e-07, bias=4.35e-07, residual=0.0),   # the residual's gradient is grad_out in any precision
    "shuffle2":   dict(x=1.15e-07, weight=1.93e-07, bias=7.61e-08),
    "shuffle4":   dict(x=1.00e-07, weight=1.12e-07, bias=9.62e-08),
    "unshuffle4": dict(x=1.07e-07, weight=1.69e-07, bias=5.71e-08),
    "wide":       dict(x=1.02e-07, x2=9.74e-08, weight=3.95e-07, bias=5.79e-08),
    "slabs":      dict(x=3.32e-07, weight=8.43e-07, bias=1.79e-07),
    "line":       dict(x=4.11e-08, weight=3.17e-08, bias=2.91e-07),
    "column":     dict(x=6.57e-08, weight=4.62e-08, bias=5.24e-08),
}
# GPU_ERR: the same ratio for the C-ABI on an MI355X, for the record (the GPU test prints it)
GPU_ERR = {
    "odd":        dict(x=1.45e-07, x2=1.28e-07, weight=1.10e-07, bias=5.49e-08),
    "cat66":      dict(x=4.23e-07, x2=3.95e-07, weight=1.92e-07, bias=1.26e-07),
    "tanh":       dict(x=2.37e-07, weight=2.09e-07, bias=1.55e-07),
    "sigmoid":    dict(x=1.77e-07, weight=1.47e-07, bias=4.72e-08),
    "resid":      dict(x=1.71e-07, weight=1.24e-07, bias=2.02e-07),
    "shuffle2":   dict(x=1.88e-07, weight=1.53e-07, bias=4.66e-08),
    "shuffle4":   dict(x=1.95e-07, weight=8.25e-08, bias=6.15e-08),
    "unshuffle4": dict(x=1.63e-07, weight=1.13e-07, bias=5.71e-08),
    "wide":       dict(x=1.07e-07, x2=1.17e-07, weight=1.09e-07, bias=1.37e-07),
    "slabs":      dict(x=1.11e-07, weight=2.18e-07, bias=5.85e-08),
    "line":       dict(x=8.16e-08, weight=3.17e-08, bias=1.99e-07),
    "column":     dict(x=8.87e-08, weight=4.62e-08, bias=2.74e-08),
}
TOL = {c: {k: 8.0 * max(v, ULP) for k, v in row.items()} for c, row in E32.items()}


def _gen(name):
    return torch.Generator().manual_seed(3000 + list(CASES).index(name))


def _act(z, act):
    return {"none": lambda t: t, "relu": torch.relu, "lrelu": lambda t: F.leaky_relu(t, 0.1), "tanh": torch.tanh, "sigmoid": torch.sigmoid}[act](z)


def _condition_bias(z0, bias):
    """z0 [n,cout,h,w]: float64 pre-activations without the bias; bias float32 [cout].  Steps each channel's bias away from its drawn
    value (+0.003, -0.003, +0.006, ...) until min|z| of the channel >= 2 ZMIN max|z| (the maximum taken with a unit of head room for
    the steps themselves)."""
    bias = bias.clone()
    zmax = float((z0 + bias.double().view(1, -1, 1, 1)).abs().max()) + 1.0
    for co in range(z0.shape[1]):
        for k in range(2000):
            b = (bias[co].double() + 0.003 * ((k + 1) // 2) * (1 if k % 2 else -1)).float()
            if float((z0[:, co] + b.double()).abs().min()) >= 2 * ZMIN * zmax:
                bias[co] = b
                break
        else:
            raise AssertionError("no bias meets the |z| condition")
    return bias


def _linear(c, x, x2, weight, bias):
    a = F.pixel_unshuffle(x, 4) if c.get("unshuffle") else x
    if x2 is not None:
        a = torch.cat([a, x2], 1)
    return F.conv2d(a, weight, bias, padding=1)


@functools.lru_cache(maxsize=None)
def leaves(name):
    """The case's float32 CPU tensors x, x2, weight, bias, residual (None where the case has none) and grad_out (never modified)."""
    c = CASES[name]
    g = _gen(name)
    n, cin, cin2, cout, h, w = (c[k] for k in ("n", "cin", "cin2", "cout", "h", "w"))
    x = torch.randn(n, cin // 16, 4 * h, 4 * w, generator=g) if c.get("unshuffle") else torch.randn(n, cin, h, w, generator=g)
    x2 = torch.randn(n, cin2, h, w, generator=g) if cin2 else None
    gain = 4.0 if c["act"] == "tanh" else 1.0   # tanh: pre-activations beyond +-9, where float32 tanh is +-1
    weight = torch.randn(cout, cin + cin2, 3, 3, generator=g) * (gain / (3.0 * (cin + cin2) ** 0.5))
    bias = torch.randn(cout, generator=g) * 0.5
    residual = torch.randn(n, cout, h, w, generator=g) if c.get("resid") else None
    r = c.get("shuffle", 1)
    grad_out = torch.randn(n, cout // (r * r), h * r, w * r, generator=g)
    if name in SIGNED:
        with torch.no_grad():
            z0 = _linear(c, x.double(), None if x2 is None else x2.double(), weight.double(), None)
        bias = _condition_bias(z0, bias)
    return dict(x=x, x2=x2, weight=weight, bias=bias, residual=residual, grad_out=grad_out)


def graph(name, x, x2, weight, bias, residual):
    """the forward in the tensors' dtype: (out, z)"""
    c = CASES[name]
    z = _linear(c, x, x2, weight, bias)
    y = _act(z, c["act"]) * c["s"]
    if residual is not None:
        y = y + residual
    if c.get("shuffle"):
        y = F.pixel_shuffle(y, c["shuffle"])
    return y, z


def run(name, dtype=torch.float64):
    L = leaves(name)
    t = {k: (None if L[k] is None else L[k].clone().to(dtype).requires_grad_(True)) for k in GRADS}
    out, z = graph(name, *(t[k] for k in GRADS))
    ks = tensors(name)
    grads = dict(zip(ks, torch.autograd.grad(out, [t[k] for k in ks], L["grad_out"].to(dtype))))
    return grads, out.detach(), z.detach()


@functools.lru_cache(maxsize=None)
def _reference(name):
    return run(name)


def reference(name):
    """The float64 gradients of the case (computed once, shared by the tests; not to be modified)."""
    return _reference(name)[0]


def reference_out(name):
    """the float64 forward, in out's own (shuffled) layout"""
    return _reference(name)[1]


def preactivations(name):
    return _reference(name)[2]


def gz_from_out(name, out, grad_out):
    """float64 gz [n,cout,h,w] = grad_out * s * act'(.), the derivative taken from `out` as the backward's contract states it"""
    c = CASES[name]
    r, s = c.get("shuffle", 1), c["s"]
    go = grad_out.double()
    if r > 1:
        go = F.pixel_unshuffle(go, r)
    if c["act"] == "none":
        return go * s
    o = out.detach().double().cpu()
    if r > 1:
        o = F.pixel_unshuffle(o, r)
    t = o / s
    d = {"relu": lambda: (o > 0).double(), "lrelu": lambda: torch.where(o > 0, 1.0, 0.1).double(), "tanh": lambda: 1.0 - t * t,
         "sigmoid": lambda: t * (1.0 - t)}[c["act"]]()
    return go * s * d


def reference_from_out(name, out):
    """The float64 gradients with the activation's derivative taken from `out` (any dtype / device; out's own layout)."""
    c, L = CASES[name], leaves(name)
    gz = gz_from_out(name, out, L["grad_out"])
    t = {k: (None if L[k] is None else L[k].clone().double().requires_grad_(True)) for k in ("x", "x2", "weight", "bias")}
    z = _linear(c, t["x"], t["x2"], t["weight"], t["bias"])
    ks = [k for k in tensors(name) if k != "residual"]
    grads = dict(zip(ks, torch.autograd.grad(z, [t[k] for k in ks], gz)))
    if c.get("resid"):
        grads["residual"] = L["grad_out"].double()
    return grads


rel_err = dc.rel_err


def measure_e32(name):
    g32, _, _ = run(name, torch.float32)
    return {k: rel_err(g32[k], reference(name)[k]) for k in tensors(name)}


# ---------------------------------------------------------------- the modules that train
# crfp_amd.model.CRFP modules on the device in float32 against the same graph in float64 on the CPU, built from F.conv2d and
# oracle.crfp_oracle.dcnv2, with a squared-error loss on the module's outputs.  The heads get random non-zero weights (init_dcn zeroes
# them) small enough that offset + flow stays a tenth of a pixel from any integer, and every relu / lrelu layer's biases are conditioned
# like the cases' (layer by layer, in forward order).
MODULES = {
    "dcn8":     dict(kind="dcn", mid=8, dg=2, repeat=False, interpolate="none", h=12, w=16, poff=(1, 8, 12, 16)),
    "dcn4":     dict(kind="dcn", mid=4, dg=1, repeat=True, interpolate="pixelshuffle", h=8, w=12, poff=(1, 32, 2, 3)),
    "resblock": dict(kind="res", cin=16, mid=8, h=9, w=11),
}
MODULE_INPUTS = {"dcn": ("cur_x", "pre_x", "pre_x_aligned", "flow", "pre_offset"), "res": ("feat",)}
MODULE_LR = 0.05
# MODULE_E32[module][leaf]: the float32 CPU graph's error of each gradient against float64 (measure_module_e32); MODULE_EFWD[module]: the
# relative error of the module's outputs on the device against float64, max over the outputs (the forward is not code under test: its
# split-fp16 products reach the gradients through the saved activations); MODULE_GPU_ERR: the gradients' measured errors on an MI355X.
MODULE_E32 = {
    "dcn8": {"dcn_block.0.weight": 1.74e-07, "dcn_block.0.bias": 1.42e-07, "dcn_block.2.weight": 2.17e-07, "dcn_block.2.bias": 1.16e-07,
             "conv_fuse.weight": 1.58e-07, "conv_fuse.bias": 6.65e-08, "dcn_offset.weight": 6.00e-07, "dcn_offset.bias": 5.55e-07,
             "dcn_mask.weight": 4.99e-07, "dcn_mask.bias": 2.15e-07, "dcn.weight": 4.64e-07, "dcn.bias": 1.08e-07, "cur_x": 2.20e-07,
             "pre_x": 5.33e-07, "pre_x_aligned": 3.66e-07, "flow": 2.45e-07, "pre_offset": 1.42e-07},
    "dcn4": {"dcn_block.0.weight": 2.56e-07, "dcn_block.0.bias": 3.53e-08, "dcn_block.2.weight": 1.79e-07, "dcn_block.2.bias": 1.38e-07,
             "conv_fuse.weight": 3.30e-07, "conv_fuse.bias": 7.69e-08, "dcn_offset.weight": 6.34e-07, "dcn_offset.bias": 4.59e-07,
             "dcn_mask.weight": 2.63e-07, "dcn_mask.bias": 2.30e-08, "dcn.weight": 4.01e-07, "dcn.bias": 5.32e-08,
             "upsample.upsample_conv.weight": 2.69e-07, "upsample.upsample_conv.bias": 1.68e-07, "cur_x": 2.30e-07, "pre_x": 7.86e-07,
             "pre_x_aligned": 2.67e-07, "flow": 3.86e-07, "pre_offset": 2.90e-07},
    "resblock": {"main.0.weight": 3.65e-07, "main.0.bias": 4.87e-08, "main.2.0.conv1.weight": 3.59e-07, "main.2.0.conv1.bias": 9.76e-08,
                 "main.2.0.conv2.weight": 2.82e-07, "main.2.0.conv2.bias": 9.44e-08, "feat": 2.70e-07},
}
MODULE_EFWD = {"dcn8": 5.10e-07, "dcn4": 5.84e-07, "resblock": 2.64e-07}
MODULE_GPU_ERR = {
    "dcn8": {"dcn_block.0.weight": 2.15e-07, "dcn_block.0.bias": 1.63e-07, "dcn_block.2.weight": 2.35e-07,
            "dcn_block.2.bias": 5.37e-08, "conv_fuse.weight": 2.06e-07, "conv_fuse.bias": 4.39e-08,
            "dcn_offset.weight": 6.34e-07, "dcn_offset.bias": 6.23e-07, "dcn_mask.weight": 5.51e-07, "dcn_mask.bias": 4.05e-07,
            "dcn.weight": 4.40e-07, "dcn.bias": 8.78e-08, "cur_x": 3.15e-07, "pre_x": 5.95e-07, "pre_x_aligned": 4.27e-07,
            "flow": 3.08e-07, "pre_offset": 2.34e-07},
    "dcn4": {"dcn_block.0.weight": 2.59e-07, "dcn_block.0.bias": 1.37e-07, "dcn_block.2.weight": 2.07e-07,
            "dcn_block.2.bias": 1.39e-07, "conv_fuse.weight": 3.16e-07, "conv_fuse.bias": 7.69e-08,
            "dcn_offset.weight": 7.59e-07, "dcn_offset.bias": 5.25e-07, "dcn_mask.weight": 3.12e-07, "dcn_mask.bias": 2.97e-07,
            "dcn.weight": 4.15e-07, "dcn.bias": 5.32e-08, "upsample.upsample_conv.weight": 2.95e-07,
            "upsample.upsample_conv.bias": 1.64e-07, "cur_x": 2.53e-07, "pre_x": 5.73e-07, "pre_x_aligned": 2.49e-07,
            "flow": 4.43e-07, "pre_offset": 2.60e-07},
    "resblock": {"main.0.weight": 2.66e-07, "main.0.bias": 4.01e-08, "main.2.0.conv1.weight": 1.47e-07,
                "main.2.0.conv1.bias": 5.06e-08, "main.2.0.conv2.weight": 1.81e-07, "main.2.0.conv2.bias": 7.48e-08,
                "feat": 3.18e-07},
}


def module_tol(name, leaf):
    return 8.0 * max(MODULE_E32[name][leaf], MODULE_EFWD[name], ULP)


def module_param_shapes(name):
    m = MODULES[name]
    if m["kind"] == "res":
        return {"main.0": (m["mid"], m["cin"]), "main.2.0.conv1": (m["mid"], m["mid"]), "main.2.0.conv2": (m["mid"], m["mid"])}
    mid, dg, npos = m["mid"], m["dg"], 1 if m["repeat"] else 9
    shapes = {"dcn_block.0": (mid, 2 * mid + 2), "dcn_block.2": (mid, mid), "conv_fuse": (mid, 2 * mid), "dcn_offset": (dg * 2 * npos, mid),
              "dcn_mask": (dg * npos, mid), "dcn": (mid, mid)}
    if m["interpolate"] == "pixelshuffle":
        shapes["upsample.upsample_conv"] = (mid * 16, mid * 8)
    return shapes


def _module_forward(name, P, I, record=None):
    """the module's graph from the state dict P and the inputs I (any dtype, CPU): its outputs; record: [(layer, z)] of the relu / lrelu
    pre-activations, and ("offset", offset + flow) of the DCN"""
    m = MODULES[name]

    def conv(layer, inp, act="none"):
        z = F.conv2d(inp, P[layer + ".weight"], P[layer + ".bias"], padding=1)
        if record is not None and act in ("relu", "lrelu"):
            record.append((layer, z.detach()))
        return _act(z, act)

    if m["kind"] == "res":
        x = conv("main.0", I["feat"], "lrelu")
        return (x + conv("main.2.0.conv2", conv("main.2.0.conv1", x, "relu")),)
    f = conv("dcn_block.0", torch.cat([I["cur_x"], I["pre_x_aligned"], I["flow"]], 1), "lrelu")
    f = conv("dcn_block.2", f, "lrelu")
    poff = I["pre_offset"]
    if m["interpolate"] == "pixelshuffle":
        poff = F.pixel_shuffle(conv("upsample.upsample_conv", poff), 4) * 2.0
    f = conv("conv_fuse", torch.cat([f, poff], 1), "lrelu")
    offset = 10.0 * conv("dcn_offset", f, "tanh")
    mask = conv("dcn_mask", f, "sigmoid")
    flow_yx = I["flow"].flip(1)
    if m["repeat"]:
        offset = (offset + flow_yx).repeat(1, 9, 1, 1)
        mask = mask.repeat(1, 9, 1, 1)
    else:
        offset = offset + flow_yx.repeat(1, offset.size(1) // 2, 1, 1)
    if record is not None:
        record.append(("offset", offset.detach()))
    return orc.dcnv2(I["pre_x"], offset, mask, P["dcn.weight"], P["dcn.bias"], m["dg"]), f


@functools.lru_cache(maxsize=None)
def module_leaves(name):
    """(P, I, targets): the state dict, the inputs and one target per output as float32 CPU tensors (never modified)"""
    m = MODULES[name]
    g = torch.Generator().manual_seed(4000 + list(MODULES).index(name))
    P = {}
    for layer, (co, ci) in module_param_shapes(name).items():
        scale = 2e-3 if layer == "dcn_offset" else 1.0   # 10 tanh(.) stays within a few hundredths of a pixel
        P[layer + ".weight"] = torch.randn(co, ci, 3, 3, generator=g) * (scale / (3.0 * ci ** 0.5))
        P[layer + ".bias"] = torch.randn(co, generator=g) * (0.3 * scale)
    h, w = m["h"], m["w"]
    if m["kind"] == "res":
        I = dict(feat=torch.randn(1, m["cin"], h, w, generator=g))
        nout = ((1, m["mid"], h, w),)
    else:
        ints = torch.randint(-2, 3, (1, 2, h, w), generator=g).double()
        flow = (ints + 0.3 + 0.4 * torch.rand(1, 2, h, w, generator=g, dtype=torch.float64)).float()
        I = dict(cur_x=torch.randn(1, m["mid"], h, w, generator=g), pre_x=torch.randn(1, m["mid"], h, w, generator=g),
                 pre_x_aligned=torch.randn(1, m["mid"], h, w, generator=g), flow=flow, pre_offset=torch.randn(*m["poff"], generator=g))
        nout = ((1, m["mid"], h, w),) * 2
    targets = tuple(torch.randn(*s, generator=g) for s in nout)
    # condition the relu / lrelu layers' biases in forward order: a layer's fix leaves the layers in front of it alone
    for _ in range(8):
        rec = []
        with torch.no_grad():
            _module_forward(name, {k: v.double() for k, v in P.items()}, {k: v.double() for k, v in I.items()}, rec)
        bad = [(layer, z) for layer, z in rec if layer != "offset" and float(z.abs().min()) < 2 * ZMIN * (float(z.abs().max()) + 1.0)]
        if not bad:
            break
        layer, z = bad[0]
        P[layer + ".bias"] = _condition_bias(z - P[layer + ".bias"].double().view(1, -1, 1, 1), P[layer + ".bias"])
    else:
        raise AssertionError("the module's layers do not meet the |z| condition")
    return P, I, targets


def module_loss(outs, targets):
    return sum(((o - t.to(device=o.device, dtype=o.dtype)) ** 2).mean() for o, t in zip(outs, targets))


def module_run(name, dtype=torch.float64):
    """the CPU graph: loss, the gradient of every parameter and input, the loss after one SGD step of MODULE_LR on the parameters, the outputs"""
    P0, I0, targets = module_leaves(name)
    P = {k: v.clone().to(dtype).requires_grad_(True) for k, v in P0.items()}
    I = {k: v.clone().to(dtype).requires_grad_(True) for k, v in I0.items()}
    outs = _module_forward(name, P, I)
    loss = module_loss(outs, targets)
    names = list(P) + list(I)
    grads = dict(zip(names, torch.autograd.grad(loss, [*P.values(), *I.values()])))
    with torch.no_grad():
        P2 = {k: v - MODULE_LR * grads[k] for k, v in P.items()}
        loss2 = module_loss(_module_forward(name, P2, {k: v.detach() for k, v in I.items()}), targets)
    return float(loss.detach()), grads, float(loss2), tuple(o.detach() for o in outs)


@functools.lru_cache(maxsize=None)
def module_reference(name):
    return module_run(name)


def module_records(name):
    """[(layer, float64 pre-activation)] of the relu / lrelu layers and ("offset", the DCN's offset + flow)"""
    P, I, _ = module_leaves(name)
    rec = []
    with torch.no_grad():
        _module_forward(name, {k: v.double() for k, v in P.items()}, {k: v.double() for k, v in I.items()}, rec)
    return rec


def measure_module_e32(name):
    _, g32, _, _ = module_run(name, torch.float32)
    ref = module_reference(name)[1]
    return {k: rel_err(g32[k], ref[k]) for k in ref}
