"""The cases of the flow_warp backward (crfp_flow_warp_backward_f32 / ops.flow_warp under autograd) and of the shared-offset DCNv2 backward
(crfp_dcnv2_shared_backward_f32 / ops.dcnv2_shared under autograd), and their float64 references.

flow_warp.  Reference: torch.autograd.grad through oracle.crfp_oracle.flow_warp on CPU float64 tensors holding the cases' float32 values,
with a random grad_out; each case in both padding modes.  The gradient with respect to the flow jumps where a sample crosses a pixel
boundary, so every flow is an integer shift plus a fraction in [0.1, 0.9]: float32 and float64 then pick the same bilinear cell even
after the round trip through the [-1, 1] normalisation.  The ``integer`` case is 9 x 17 because with H - 1 and W - 1 powers of two
integer positions survive that round trip exactly (at 9 x 11 the float32 oracle lands a hair below an integer and picks the neighbouring
cell).  The ``nonfinite`` case's reference is computed on the flow with NaN, -inf and -1e30 replaced by -4 max(h, w) and +inf / +1e30 by
+4 max(h, w): the same function under the forward's clamps, and inside the defined behaviour of ATen's CPU kernel.

dcnv2_shared.  The ``shared`` case and its float64 leaf gradients come from tests/dcn_backward_cases.py; ``shared_motion`` and
``shared_integer`` are of the same kind: compact leaves offset [n,2,h,w] and mask [n,1,h,w], reference = autograd through
oracle.crfp_oracle.dcnv2 on the 9x-tiled tensors in float64.

Tolerance (per case, mode and gradient tensor): max|got - ref64| <= TOL * max|ref64| with TOL = 8 * max(E32, 2^-23).  E32 is the float32
oracle's own error against float64, max|oracle32 - oracle64| / max|oracle64|, measured on the CPU by ``measure_e32`` /
``measure_shared_e32`` and written down below.  The factor 8 is the project's margin for a different summation order and the unordered
atomic sum of grad_x; the floor 2^-23 is one float32 ulp -- the exact cases have E32 ~ 0, which no float32 sum can meet.
"""
import functools

import torch
import torch.nn.functional as F

import dcn_backward_cases as dc
from oracle import crfp_oracle as orc

MODES = ("zeros", "border")
GRADS = ("x", "flow")
ULP = 2.0 ** -23

# name -> n, c, h, w, the integer shift of its flow
CASES = {
    "odd":       dict(n=2, c=5, h=9, w=11, shift=3),     # c not a multiple of 4, nothing tile-aligned; 39 % of the samples leave the frame
    "c32":       dict(n=1, c=32, h=20, w=36, shift=3),   # the 2x call's channel count: several channel chunks
    "motion":    dict(n=2, c=5, h=9, w=11, shift=15),    # 92 % of the samples leave the frame (88 % with no corner inside); beyond any window
    "wide":      dict(n=1, c=4, h=24, w=70, shift=10),   # two workgroup columns, six row tiles, overlapping windows; shifts inside and beyond a halo
    "line":      dict(n=1, c=3, h=1, w=7, shift=2),      # max(H - 1, 1): the chain factor 0 along y
    "column":    dict(n=1, c=3, h=6, w=1, shift=2),      # ... along x
    "integer":   dict(n=2, c=4, h=9, w=17, shift=3),     # image 0: zero flow (grad_x == grad_out bit for bit); image 1: integers, boundary hits
    "edges":     dict(n=2, c=5, h=9, w=11, shift=3),     # positions in (-1, 0) and (W - 1, W): one corner row / column valid; border: clamped
    "nonfinite": dict(n=1, c=4, h=9, w=17, shift=3),     # a dozen pixels NaN, +-inf, +-1e30: no address from an unbounded position
}
FRACTIONAL = ("odd", "c32", "motion", "wide", "line", "column", "edges", "nonfinite")
OUTSIDE_SHARE = {"odd": 0.389, "motion": 0.919}   # samples outside [0, W - 1] x [0, H - 1] (at least one corner outside the frame), this draw

# hand-set flows of "edges": (image, y, x, component (0: dx, 1: dy), value)
EDGES = ((0, 4, 0, 0, -0.5), (0, 4, 10, 0, 0.5), (0, 0, 5, 1, -0.5), (0, 8, 5, 1, 0.5),      # one step over each edge
         (1, 0, 0, 0, -0.75), (1, 0, 0, 1, -0.25), (1, 8, 10, 0, 0.625), (1, 8, 10, 1, 0.375),   # over a frame corner: one corner valid
         (1, 3, 2, 0, -2.5), (1, 5, 8, 0, 2.5), (1, 2, 6, 1, -2.5), (1, 6, 4, 1, 2.5))          # ... from the interior
# the touched pixels of "nonfinite": (y, x, component, value)
NONFINITE = ((0, 0, 0, float("nan")), (1, 3, 1, float("nan")), (2, 5, 0, float("inf")), (3, 7, 1, float("inf")),
             (4, 9, 0, float("-inf")), (5, 11, 1, float("-inf")), (6, 13, 0, 1e30), (7, 15, 1, 1e30), (8, 16, 0, -1e30),
             (8, 0, 1, -1e30), (4, 4, 0, float("nan")), (4, 4, 1, float("inf")), (0, 16, 0, float("inf")), (0, 16, 1, float("-inf")))

# E32[case][mode][tensor]: max|oracle float32 - oracle float64| / max|oracle float64| of that gradient on the CPU (measure_e32; torch 2.x
# CPU kernels); TOL = 8 * max(E32, 2^-23).  GPU_ERR: the same ratio for ops.flow_warp on an MI355X, for the record (the test prints it).
E32 = {
    "odd":       dict(zeros=dict(x=4.56e-07, flow=4.02e-07), border=dict(x=3.09e-07, flow=4.02e-07)),
    "c32":       dict(zeros=dict(x=2.04e-06, flow=1.48e-06), border=dict(x=1.77e-06, flow=1.48e-06)),
    "motion":    dict(zeros=dict(x=2.98e-07, flow=2.16e-07), border=dict(x=2.23e-07, flow=1.39e-07)),
    "wide":      dict(zeros=dict(x=3.00e-06, flow=3.72e-06), border=dict(x=2.51e-06, flow=3.72e-06)),
    "line":      dict(zeros=dict(x=2.77e-07, flow=3.12e-08), border=dict(x=2.84e-07, flow=3.12e-08)),
    "column":    dict(zeros=dict(x=5.70e-08, flow=8.91e-08), border=dict(x=8.14e-08, flow=8.91e-08)),
    "integer":   dict(zeros=dict(x=4.13e-08, flow=4.88e-08), border=dict(x=4.13e-08, flow=4.88e-08)),
    "edges":     dict(zeros=dict(x=1.22e-06, flow=1.01e-06), border=dict(x=2.80e-07, flow=3.74e-07)),
    "nonfinite": dict(zeros=dict(x=3.51e-07, flow=6.97e-07), border=dict(x=3.51e-07, flow=6.75e-07)),
}
GPU_ERR = {
    "odd":       dict(zeros=dict(x=4.77e-07, flow=3.94e-07), border=dict(x=3.09e-07, flow=3.94e-07)),
    "c32":       dict(zeros=dict(x=2.05e-06, flow=1.48e-06), border=dict(x=1.77e-06, flow=1.48e-06)),
    "motion":    dict(zeros=dict(x=2.98e-07, flow=2.16e-07), border=dict(x=1.89e-07, flow=1.39e-07)),
    "wide":      dict(zeros=dict(x=3.00e-06, flow=3.69e-06), border=dict(x=2.49e-06, flow=3.69e-06)),
    "line":      dict(zeros=dict(x=2.77e-07, flow=3.12e-08), border=dict(x=2.84e-07, flow=3.12e-08)),
    "column":    dict(zeros=dict(x=5.70e-08, flow=8.91e-08), border=dict(x=8.14e-08, flow=8.91e-08)),
    "integer":   dict(zeros=dict(x=4.13e-08, flow=4.88e-08), border=dict(x=4.13e-08, flow=4.88e-08)),
    "edges":     dict(zeros=dict(x=1.22e-06, flow=1.01e-06), border=dict(x=2.80e-07, flow=3.74e-07)),
    "nonfinite": dict(zeros=dict(x=3.51e-07, flow=6.97e-07), border=dict(x=3.51e-07, flow=6.75e-07)),
}   # the kernel restates the oracle's float32 arithmetic, so most entries equal E32 to three digits; the adjoint test sits below 4e-8
TOL = {c: {m: {k: 8.0 * max(v, ULP) for k, v in row.items()} for m, row in modes.items()} for c, modes in E32.items()}

# the shared-offset DCNv2 cases: n, h, w, kind (4 -> 4 channels, one group)
SHARED_CASES = {
    "shared":         dict(n=1, h=24, w=40, kind="shared", shift=3),      # tests/dcn_backward_cases.py's own
    "shared_motion":  dict(n=1, h=9, w=70, kind="motion", shift=15),      # large shifts, hand-set edge straddles, two workgroup columns
    "shared_integer": dict(n=2, h=9, w=11, kind="integer", shift=3),      # image 0: zero offsets; image 1: integer offsets
}
SHARED_E32 = {
    "shared":         dc.E32["shared"],
    "shared_motion":  dict(x=3.23e-06, offset=1.60e-06, mask=2.48e-06, weight=1.43e-06, bias=1.11e-07),
    "shared_integer": dict(x=1.02e-07, offset=1.16e-07, mask=1.90e-07, weight=3.99e-07, bias=2.67e-07),
}
SHARED_GPU_ERR = {
    "shared":         dict(x=1.61e-06, offset=2.27e-06, mask=2.44e-06, weight=1.19e-06, bias=2.48e-07),
    "shared_motion":  dict(x=3.20e-06, offset=1.67e-06, mask=2.48e-06, weight=1.40e-06, bias=1.27e-07),
    "shared_integer": dict(x=1.43e-07, offset=1.06e-07, mask=1.25e-07, weight=1.03e-07, bias=5.22e-07),
}   # the largest share of a tolerance: bias of "shared_integer", 0.24
SHARED_TOL = {c: {k: 8.0 * max(v, ULP) for k, v in row.items()} for c, row in SHARED_E32.items()}

# the alignment graph of tests/test_gpu_warp_backward.py (flow_warp -> two conv heads -> dcnv2_shared at 12 x 16 -> squared error): E32 of
# each gradient, and of the loss after one SGD step on the heads, for the same graph in float32 on the CPU
GRAPH_E32 = dict(flow=6.44e-07, prev=6.15e-07, off_w=4.20e-07, off_b=2.29e-07, mask_w=4.12e-07, mask_b=9.29e-08, dcn_w=6.18e-07, dcn_b=1.79e-07,
                 loss2=1.20e-07)
GRAPH_GPU_ERR = dict(flow=6.44e-07, prev=5.62e-07, off_w=5.13e-07, off_b=1.67e-07, mask_w=6.15e-07, mask_b=1.69e-07, dcn_w=6.38e-07, dcn_b=2.40e-07,
                     loss2=1.20e-07)
GRAPH_TOL = {k: 8.0 * max(v, ULP) for k, v in GRAPH_E32.items()}
GRAPH_LR = 0.05
GRAPH_GRADS = ("flow", "prev", "off_w", "off_b", "mask_w", "mask_b", "dcn_w", "dcn_b")
GRAPH_HEADS = ("off_w", "off_b", "mask_w", "mask_b")


def _gen(name):
    return torch.Generator().manual_seed(2000 + (list(CASES) + list(SHARED_CASES)).index(name))


# ---------------------------------------------------------------- flow_warp
@functools.lru_cache(maxsize=None)
def leaves(name):
    """The case's float32 CPU tensors x, flow [n,h,w,2] = (dx, dy), grad_out (never modified: callers clone)."""
    c = CASES[name]
    g = _gen(name)
    n, ch, h, w = (c[k] for k in ("n", "c", "h", "w"))
    x = torch.randn(n, ch, h, w, generator=g)
    grad_out = torch.randn(n, ch, h, w, generator=g)
    if name == "integer":
        flow = torch.zeros(n, h, w, 2)
        flow[1:] = torch.randint(-c["shift"], c["shift"] + 1, (n - 1, h, w, 2), generator=g).float()
    else:
        flow = dc._frac_offsets(g, (n, h, w, 2), c["shift"])
    if name == "edges":
        for i, y, xx, k, v in EDGES:
            flow[i, y, xx, k] = v
    if name == "nonfinite":
        for y, xx, k, v in NONFINITE:
            flow[0, y, xx, k] = v
    return dict(x=x, flow=flow, grad_out=grad_out)


def touched(name="nonfinite"):
    """[h, w] bool: the pixels of the case whose flow is not finite or huge"""
    f = leaves(name)["flow"][0]
    return (~torch.isfinite(f) | (f.abs() > 1e20)).any(-1)


def reference_flow(name):
    """The flow the reference is computed on: the case's own, except that "nonfinite" has its touched values replaced (module docstring)."""
    c, f = CASES[name], leaves(name)["flow"]
    if name != "nonfinite":
        return f
    big = 4.0 * max(c["h"], c["w"])
    neg = torch.isnan(f) | (f < -1e20)
    return torch.where(neg, torch.full_like(f, -big), torch.where(f > 1e20, torch.full_like(f, big), f))


def sample_positions(name, dtype=torch.float64):
    """(iy, ix) [n, h, w]: the unclamped sample coordinates of the (reference) flow after the normalisation round trip, computed in dtype"""
    c = CASES[name]
    h, w = c["h"], c["w"]
    f = reference_flow(name).to(dtype)
    gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    nx = 2.0 * (gx.to(dtype) + f[..., 0]) / max(w - 1, 1) - 1.0
    ny = 2.0 * (gy.to(dtype) + f[..., 1]) / max(h - 1, 1) - 1.0
    return (ny + 1.0) * ((h - 1) / 2.0), (nx + 1.0) * ((w - 1) / 2.0)


def run(fn, name, mode, dtype=torch.float64, device="cpu", needs=GRADS, flow=None):
    """fn(x, flow, padding_mode) -> out through backward(grad_out): {tensor name: gradient, or None} and out"""
    L = leaves(name)
    src = dict(x=L["x"], flow=L["flow"] if flow is None else flow)
    t = {k: src[k].clone().to(device=device, dtype=dtype).requires_grad_(k in needs) for k in GRADS}
    out = fn(t["x"], t["flow"], mode)
    out.backward(L["grad_out"].to(device=device, dtype=dtype))
    return {k: t[k].grad for k in GRADS}, out.detach()


def oracle_fn(x, flow, mode):
    return orc.flow_warp(x, flow, padding_mode=mode)


@functools.lru_cache(maxsize=None)
def _reference(name, mode):
    return run(oracle_fn, name, mode, flow=reference_flow(name))


def reference(name, mode):
    """The float64 gradients of the case (computed once, shared by the tests; not to be modified)."""
    return _reference(name, mode)[0]


def reference_out(name, mode):
    return _reference(name, mode)[1]


rel_err = dc.rel_err


def measure_e32(name, mode):
    g32, _ = run(oracle_fn, name, mode, torch.float32, flow=reference_flow(name))
    return {k: rel_err(g32[k], reference(name, mode)[k]) for k in GRADS}


# ---------------------------------------------------------------- dcnv2_shared
SHARED_GRADS = dc.GRADS


@functools.lru_cache(maxsize=None)
def shared_leaves(name):
    """x, the compact offset [n,2,h,w] = (dy, dx) and mask [n,1,h,w], weight, bias, grad_out as float32 CPU tensors"""
    if name == "shared":
        return dc.leaves("shared")
    c = SHARED_CASES[name]
    g = _gen(name)
    n, h, w = c["n"], c["h"], c["w"]
    x = torch.randn(n, 4, h, w, generator=g)
    weight = torch.randn(4, 4, 3, 3, generator=g) * 0.2
    bias = torch.randn(4, generator=g)
    grad_out = torch.randn(n, 4, h, w, generator=g)
    mask = torch.rand(n, 1, h, w, generator=g)
    if c["kind"] == "integer":
        offset = torch.zeros(n, 2, h, w)
        offset[1:] = torch.randint(-c["shift"], c["shift"] + 1, (n - 1, 2, h, w), generator=g).float()
    else:
        offset = dc._frac_offsets(g, (n, 2, h, w), c["shift"])
        # samples that straddle an edge with one corner row / column inside (tap (ky, kx) of pixel (y, x) sits at (y - 1 + ky + dy, x - 1 + kx + dx))
        offset[0, 0, 0, 0], offset[0, 1, 0, 0] = 0.5, 2.5               # pixel (0, 0), taps ky = 0: py = -0.5, only the bottom corner row counts
        offset[0, 0, 0, 2], offset[0, 1, 0, 2] = 3.5, w - 2.5           # pixel (0, 2), taps kx = 1: px = w - 0.5, only the left corner column counts
        offset[0, 0, h - 1, 0], offset[0, 1, h - 1, 0] = 0.5, 0.5       # pixel (h - 1, 0), taps ky = 1: py = h - 0.5, only the top corner row counts
        offset[0, 0, 0, 3], offset[0, 1, 0, 3] = 0.5, 0.5               # pixel (0, 3), taps ky = 0: (-0.5, x + 0.5): one corner row, both columns
    return dict(x=x, offset=offset, mask=mask, weight=weight, bias=bias, grad_out=grad_out)


def shared_sample_positions(name):
    """float64 (py, px) [n, 9, h, w] of the case's float32 offsets"""
    L = shared_leaves(name)
    n, _, h, w = L["offset"].shape
    off = L["offset"].double()
    k = torch.arange(9)
    ys = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1) + (k // 3 - 1).double().view(1, 9, 1, 1)
    xs = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w) + (k % 3 - 1).double().view(1, 9, 1, 1)
    return ys + off[:, 0:1], xs + off[:, 1:2]


def run_shared(fn, name, dtype=torch.float64, device="cpu", needs=SHARED_GRADS):
    """fn(x, offset [n,2,h,w], mask [n,1,h,w], weight, bias) -> out through backward(grad_out): {tensor name: gradient, or None} and out"""
    L = shared_leaves(name)
    t = {k: L[k].clone().to(device=device, dtype=dtype).requires_grad_(k in needs) for k in SHARED_GRADS}
    out = fn(*(t[k] for k in SHARED_GRADS))
    out.backward(L["grad_out"].to(device=device, dtype=dtype))
    return {k: t[k].grad for k in SHARED_GRADS}, out.detach()


def shared_oracle_fn(x, offset, mask, weight, bias):
    """the reference's tiled form (model/CRFP.py:341-350)"""
    return orc.dcnv2(x, offset.repeat(1, 9, 1, 1), mask.repeat(1, 9, 1, 1), weight, bias, 1)


@functools.lru_cache(maxsize=None)
def shared_reference(name):
    """The float64 leaf gradients of the case (computed once; not to be modified)."""
    if name == "shared":
        return dc.reference("shared")
    return run_shared(shared_oracle_fn, name)[0]


def measure_shared_e32(name):
    g32, _ = run_shared(shared_oracle_fn, name, torch.float32)
    return {k: rel_err(g32[k], shared_reference(name)[k]) for k in SHARED_GRADS}


# ---------------------------------------------------------------- the alignment graph
def graph_params(dtype=torch.float64, device="cpu"):
    """leaves of the graph: the flow [1,12,16,2] (integer in +-2 plus a fraction in [0.3, 0.7]), prev, the two heads (small enough that
    offset + flow stays a tenth of a pixel from any integer) and the DCN's weight / bias"""
    g = torch.Generator().manual_seed(177)
    mk = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale   # noqa: E731
    ints = torch.randint(-2, 3, (1, 12, 16, 2), generator=g).double()
    flow = (ints + 0.3 + 0.4 * torch.rand(1, 12, 16, 2, generator=g, dtype=torch.float64)).float()
    P = dict(flow=flow, prev=mk(1, 4, 12, 16), off_w=mk(2, 10, 3, 3, scale=5e-4), off_b=mk(2, scale=5e-4), mask_w=mk(1, 10, 3, 3, scale=0.1),
             mask_b=mk(1, scale=0.1), dcn_w=mk(4, 4, 3, 3, scale=2.0 / 6.0), dcn_b=mk(4, scale=0.1))
    return {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in P.items()}


def graph_data(dtype=torch.float64, device="cpu"):
    g = torch.Generator().manual_seed(178)
    cur = torch.randn(1, 4, 12, 16, generator=g)
    target = torch.randn(1, 4, 12, 16, generator=g)
    return cur.to(device=device, dtype=dtype), target.to(device=device, dtype=dtype)


def graph_offsets(P, cur, warp=oracle_fn):
    """warped prev, and the DCN's offset (dy, dx) = 10 tanh(head) + flow (dx, dy) flipped, and its mask (model/CRFP.py:337-349)"""
    flow_c = P["flow"].permute(0, 3, 1, 2)
    feat = torch.cat((cur, warp(P["prev"], P["flow"], "zeros"), flow_c), 1)
    offset = 10.0 * torch.tanh(F.conv2d(feat, P["off_w"], P["off_b"], padding=1))
    mask = torch.sigmoid(F.conv2d(feat, P["mask_w"], P["mask_b"], padding=1))
    return offset + flow_c.flip(1), mask


def graph_loss(P, cur, target, warp=oracle_fn, dcn=shared_oracle_fn):
    offset, mask = graph_offsets(P, cur, warp)
    return ((dcn(P["prev"], offset, mask, P["dcn_w"], P["dcn_b"]) - target) ** 2).mean()


def graph_step(P, grads):
    """one SGD step of GRAPH_LR on the heads"""
    with torch.no_grad():
        return {k: (v - GRAPH_LR * grads[k] if k in GRAPH_HEADS else v.detach()) for k, v in P.items()}


def graph_run(dtype=torch.float64, device="cpu", warp=oracle_fn, dcn=shared_oracle_fn):
    """the loss, the gradient of every leaf, and the loss after one SGD step on the heads"""
    P = graph_params(dtype, device)
    data = graph_data(dtype, device)
    loss = graph_loss(P, *data, warp, dcn)
    grads = dict(zip(GRAPH_GRADS, torch.autograd.grad(loss, [P[k] for k in GRAPH_GRADS])))
    with torch.no_grad():
        loss2 = graph_loss(graph_step(P, grads), *data, warp, dcn)
    return float(loss.detach()), grads, float(loss2)


@functools.lru_cache(maxsize=None)
def graph_reference():
    return graph_run()


def graph_errors(loss2, grads):
    """each gradient's rel_err against the float64 graph, and the relative error of the loss after the step"""
    _, gref, loss2_ref = graph_reference()
    errs = {k: rel_err(grads[k], gref[k]) for k in GRAPH_GRADS}
    errs["loss2"] = abs(loss2 - loss2_ref) / abs(loss2_ref)
    return errs


def measure_graph_e32():
    _, g32, loss2 = graph_run(torch.float32)
    return graph_errors(loss2, g32)
