"""The cases of the DCNv2 backward (crfp_dcnv2_backward_f32 / ops.dcnv2 under autograd) and their float64 reference.

Reference: torch.autograd.grad through oracle.crfp_oracle.dcnv2 on CPU float64 tensors holding the cases' float32 values, with a random
grad_out.  The gradient with respect to an offset jumps where a sample crosses a pixel boundary, so every offset is an integer shift plus
a fraction in [0.1, 0.9]: float32 and float64 then pick the same bilinear cell (the integer case is exact in both).  ``run`` is the one
harness every implementation goes through -- the oracle in float64 / float32 on the CPU, ops.dcnv2 on the GPU.

Tolerance (per case and gradient tensor): max|got - ref64| <= TOL * max|ref64| with TOL = 8 * E32, where E32 is the reference's own fp32
error, max|oracle32 - oracle64| / max|oracle64|, measured on the CPU by ``measure_e32`` and written down below.  The factor 8 covers a
different summation order over up to n*h*w terms and the unordered atomic sum of grad_x.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import crfp_oracle as orc

GRADS = ("x", "offset", "mask", "weight", "bias")   # the order of ops.dcnv2's tensor arguments; offset / mask: at the case's leaves

# name -> n, cin, cout, dg, h, w, kind
CASES = {
    "odd":      dict(n=2, cin=8, cout=6, dg=2, h=9, w=11, kind="shift", shift=3),     # 1: odd sizes, nothing aligns to a tile
    "g8":       dict(n=1, cin=32, cout=32, dg=8, h=20, w=36, kind="shift", shift=3),  # 2: the reference's 2x call (forward: MFMA path)
    "shared":   dict(n=1, cin=4, cout=4, dg=1, h=24, w=40, kind="shared", shift=3),   # 3: dcn_3: 2 + 1 channel leaves tiled 9x
    "motion":   dict(n=2, cin=8, cout=6, dg=2, h=9, w=11, kind="shift", shift=15),    # 4: shifts up to +-(max(h, w) + 4)
    "integer":  dict(n=2, cin=8, cout=6, dg=2, h=9, w=11, kind="integer", shift=3),   # 5: offsets 0 (image 0) and an integer shift (image 1)
    "identity": dict(n=1, cin=8, cout=8, dg=2, h=10, w=13, kind="identity", shift=3), # 6: the reference's identity KAT
    # 7 (the kernels' own paths): groups of 6 channels = a whole and a partial chunk of the pixel kernel's 4-channel LDS window, 2 x 2
    # workgroups whose windows overlap, 36 outputs = two channel tiles of the weight pass, shifts inside and beyond the window's halo
    "chunks":   dict(n=1, cin=12, cout=36, dg=2, h=6, w=70, kind="shift", shift=10),
}

# E32[case][tensor]: max|oracle float32 - oracle float64| / max|oracle float64| of that gradient, measured on the CPU (measure_e32; torch
# 2.x CPU kernels); TOL = 8 * E32.  GPU_ERR: the same ratio for ops.dcnv2 on an MI355X, for the record (the test prints it).
E32 = {
    "odd":      dict(x=5.49e-07, offset=3.71e-07, mask=4.78e-07, weight=6.13e-07, bias=6.13e-08),
    "g8":       dict(x=1.68e-06, offset=2.18e-06, mask=2.39e-06, weight=1.15e-06, bias=9.06e-08),
    "shared":   dict(x=1.61e-06, offset=2.24e-06, mask=2.44e-06, weight=1.08e-06, bias=1.94e-07),
    "motion":   dict(x=4.79e-07, offset=3.27e-07, mask=4.45e-07, weight=4.96e-07, bias=3.58e-08),
    "integer":  dict(x=1.07e-07, offset=1.55e-07, mask=1.01e-07, weight=4.46e-07, bias=6.13e-08),
    "identity": dict(x=4.61e-07, offset=3.08e-07, mask=5.23e-07, weight=4.44e-07, bias=1.36e-07),
    "chunks":   dict(x=2.78e-06, offset=2.28e-06, mask=4.15e-06, weight=2.03e-06, bias=9.82e-08),
}
GPU_ERR = {
    "odd":      dict(x=5.49e-07, offset=3.31e-07, mask=4.93e-07, weight=3.79e-07, bias=8.76e-08),
    "g8":       dict(x=1.73e-06, offset=2.25e-06, mask=2.39e-06, weight=1.21e-06, bias=1.47e-07),
    "shared":   dict(x=1.61e-06, offset=2.27e-06, mask=2.43e-06, weight=1.19e-06, bias=2.48e-07),
    "motion":   dict(x=4.79e-07, offset=3.85e-07, mask=4.26e-07, weight=4.08e-07, bias=1.82e-07),
    "integer":  dict(x=1.37e-07, offset=1.07e-07, mask=1.25e-07, weight=1.58e-07, bias=1.52e-07),
    "identity": dict(x=4.61e-07, offset=2.81e-07, mask=5.23e-07, weight=3.51e-07, bias=1.32e-07),
    "chunks":   dict(x=2.74e-06, offset=2.28e-06, mask=4.22e-06, weight=2.08e-06, bias=1.40e-07),
}   # grad_x moves in its last digits from run to run (1.73e-06 / 1.70e-06 on "g8"); the largest share of a tolerance: bias of "motion", 0.64
TOL = {c: {k: 8.0 * v for k, v in row.items()} for c, row in E32.items()}

# the module-level graph of tests/test_gpu_dcn_backward.py (two conv heads -> DCNv2(8, 8, dg 2) at 12 x 16 -> squared error): E32 of each
# parameter's gradient for the same graph in float32 on the CPU, in the order of ``module_params``
MODULE_E32 = dict(off_w=1.63e-06, off_b=1.87e-06, mask_w=1.91e-06, mask_b=6.17e-07, dcn_w=2.33e-06, dcn_b=3.15e-07)
MODULE_GPU_ERR = dict(off_w=2.37e-06, off_b=2.91e-06, mask_w=2.60e-06, mask_b=8.44e-07, dcn_w=2.11e-06, dcn_b=4.70e-07)
MODULE_TOL = {k: 8.0 * v for k, v in MODULE_E32.items()}
MODULE_LR = 0.05


def _gen(name):
    return torch.Generator().manual_seed(1000 + list(CASES).index(name))


def _frac_offsets(g, shape, shift):
    """integer shift in [-shift, shift] plus a fraction in [0.1, 0.9], as float32"""
    ints = torch.randint(-shift, shift + 1, shape, generator=g).to(torch.float64)
    frac = 0.1 + 0.8 * torch.rand(shape, generator=g, dtype=torch.float64)
    off = (ints + frac).to(torch.float32)
    # the float32 rounding may leave the interval by one ulp at its ends: step such a value one ulp back inside
    f = off.double() - torch.floor(off.double())
    off = torch.where(f < 0.1, torch.nextafter(off, torch.full_like(off, float("inf"))), off)
    off = torch.where(f > 0.9, torch.nextafter(off, torch.full_like(off, float("-inf"))), off)
    return off


@functools.lru_cache(maxsize=None)
def leaves(name):
    """The case's float32 CPU tensors: x, offset leaf, mask leaf, weight, bias, grad_out (never modified: callers clone)."""
    c = CASES[name]
    g = _gen(name)
    n, cin, cout, dg, h, w = (c[k] for k in ("n", "cin", "cout", "dg", "h", "w"))
    x = torch.randn(n, cin, h, w, generator=g)
    weight = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    bias = torch.randn(cout, generator=g)
    grad_out = torch.randn(n, cout, h, w, generator=g)
    if c["kind"] == "shared":
        offset = _frac_offsets(g, (n, 2, h, w), c["shift"])
        mask = torch.rand(n, 1, h, w, generator=g)
    elif c["kind"] == "integer":
        offset = torch.zeros(n, 2 * dg * 9, h, w)
        offset[1:] = torch.randint(-c["shift"], c["shift"] + 1, (n - 1, 2 * dg * 9, h, w), generator=g).float()
        mask = torch.rand(n, dg * 9, h, w, generator=g)
    elif c["kind"] == "identity":
        flow = _frac_offsets(g, (n, 2, h, w), c["shift"])    # (dx, dy) in pixels
        offset = flow                                        # the leaf IS the flow; expand() flips and tiles it
        mask = torch.full((n, dg * 9, h, w), 0.5)
        weight = torch.zeros(cout, cin, 3, 3)
        weight[torch.arange(cout), torch.arange(cin), 1, 1] = 1.0
        bias = torch.zeros(cout)
    else:
        offset = _frac_offsets(g, (n, 2 * dg * 9, h, w), c["shift"])
        mask = torch.rand(n, dg * 9, h, w, generator=g)
        if name == "motion":   # samples that straddle an edge with one corner row / column inside: tap 0 of pixel (0, 0) sits at (-1, -1)
            offset[0, 0, 0, 0], offset[0, 1, 0, 0] = 0.5, 2.5            # py = -0.5: only the bottom corner row counts
            offset[0, 2, 0, 0], offset[0, 3, 0, 0] = 3.5, w - 0.5        # tap 1 (-1, 0): px = w - 0.5: only the left corner column counts
            offset[1, 0, 0, 0], offset[1, 1, 0, 0] = float(h) + 0.5, 0.5  # py = h - 0.5: only the top corner row counts
            offset[1, 2, 0, 0], offset[1, 3, 0, 0] = 0.5, 0.5            # (-0.5, 0.5): one corner row, both columns
    return dict(x=x, offset=offset, mask=mask, weight=weight, bias=bias, grad_out=grad_out)


def expand(name, offset, mask):
    """leaves -> the [n, 2*dg*9, h, w] offset and [n, dg*9, h, w] mask DCNv2 takes (differentiable)"""
    kind, dg = CASES[name]["kind"], CASES[name]["dg"]
    if kind == "shared":
        return offset.repeat(1, 9, 1, 1), mask.repeat(1, 9, 1, 1)     # model/CRFP.py:341-347
    if kind == "identity":
        return offset.flip(1).repeat(1, dg * 9, 1, 1), mask            # model/CRFP.py:337-349 with zero offset / mask convs
    return offset, mask


def sample_positions(name):
    """float64 sample positions (py, px) [n, dg, 9, h, w] of the case's float32 offsets"""
    c, L = CASES[name], leaves(name)
    off, _ = expand(name, L["offset"].double(), L["mask"].double())
    n, dg, h, w = c["n"], c["dg"], c["h"], c["w"]
    off = off.reshape(n, dg, 9, 2, h, w)
    k = torch.arange(9)
    ys = torch.arange(h, dtype=torch.float64).view(1, 1, 1, h, 1) + (k // 3 - 1).double().view(1, 1, 9, 1, 1)
    xs = torch.arange(w, dtype=torch.float64).view(1, 1, 1, 1, w) + (k % 3 - 1).double().view(1, 1, 9, 1, 1)
    return ys + off[:, :, :, 0], xs + off[:, :, :, 1]


def run(fn, name, dtype=torch.float64, device="cpu", needs=GRADS):
    """fn(x, offset, mask, weight, bias, dg) -> out through backward(grad_out): {tensor name: gradient at the leaf, or None} and out"""
    L = leaves(name)
    t = {k: L[k].clone().to(device=device, dtype=dtype).requires_grad_(k in needs) for k in GRADS}
    off, msk = expand(name, t["offset"], t["mask"])
    out = fn(t["x"], off, msk, t["weight"], t["bias"], CASES[name]["dg"])
    out.backward(L["grad_out"].to(device=device, dtype=dtype))
    return {k: t[k].grad for k in GRADS}, out.detach()


def oracle_fn(x, offset, mask, weight, bias, dg):
    return orc.dcnv2(x, offset, mask, weight, bias, dg)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return run(oracle_fn, name)


def reference(name):
    """The float64 gradients of the case (computed once, shared by the tests; not to be modified)."""
    return _reference(name)[0]


def reference_out(name):
    """The float64 forward result the gradients belong to."""
    return _reference(name)[1]


def rel_err(got, ref):
    """max|got - ref| / max|ref| (ref float64)"""
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def measure_e32(name):
    g32, _ = run(oracle_fn, name, torch.float32)
    return {k: rel_err(g32[k], reference(name)[k]) for k in GRADS}


@functools.lru_cache(maxsize=None)
def identity_reference():
    """Case 6 from the reference's side (KAT 1): an identity-initialised DCN is 0.5 * flow_warp, so grad_x is the
    float64 autograd gradient of 0.5 * F.grid_sample(x, ..., align_corners=True, zeros) and the gradient of the flow that of the same
    function -- which the tiled offset spreads over the taps (only the centre tap carries weight)."""
    L = leaves("identity")
    x = L["x"].double().requires_grad_(True)
    flow = L["offset"].double().requires_grad_(True)      # [n, 2, h, w] = (dx, dy)
    out = 0.5 * orc.flow_warp(x, flow.permute(0, 2, 3, 1))
    gx, gflow = torch.autograd.grad(out, (x, flow), L["grad_out"].double())
    return gx, gflow


# ---------------------------------------------------------------- the module-level graph
def module_params(dtype=torch.float64, device="cpu"):
    g = torch.Generator().manual_seed(77)
    mk = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(device=device, dtype=dtype).requires_grad_(True)
    stdv = 1.0 / (8 * 9) ** 0.5
    return dict(off_w=mk(36, 8, 3, 3, scale=0.1), off_b=mk(36, scale=0.1), mask_w=mk(18, 8, 3, 3, scale=0.1), mask_b=mk(18, scale=0.1),
                dcn_w=mk(8, 8, 3, 3, scale=2 * stdv), dcn_b=mk(8, scale=0.1))


def module_data(dtype=torch.float64, device="cpu"):
    g = torch.Generator().manual_seed(78)
    feat = torch.randn(1, 8, 12, 16, generator=g)
    x = torch.randn(1, 8, 12, 16, generator=g)
    target = torch.randn(1, 8, 12, 16, generator=g)
    return tuple(t.to(device=device, dtype=dtype) for t in (feat, x, target))


def module_heads(P, feat):
    """the two nn.Conv2d heads' arithmetic: 10 * tanh offsets and a sigmoid mask (model/CRFP.py:337-340)"""
    offset = 10.0 * torch.tanh(F.conv2d(feat, P["off_w"], P["off_b"], padding=1))
    mask = torch.sigmoid(F.conv2d(feat, P["mask_w"], P["mask_b"], padding=1))
    return offset, mask


def module_loss(P, feat, x, target, dcn=oracle_fn):
    offset, mask = module_heads(P, feat)
    return ((dcn(x, offset, mask, P["dcn_w"], P["dcn_b"], 2) - target) ** 2).mean()


@functools.lru_cache(maxsize=None)
def module_reference():
    """float64 CPU: the loss, every parameter's gradient, and the loss after one SGD step of MODULE_LR"""
    P = module_params()
    data = module_data()
    loss = module_loss(P, *data)
    grads = dict(zip(P, torch.autograd.grad(loss, list(P.values()))))
    with torch.no_grad():
        P2 = {k: v - MODULE_LR * grads[k] for k, v in P.items()}
        loss2 = module_loss(P2, *data)
    return float(loss.detach()), grads, float(loss2)


def measure_module_e32():
    P = module_params(torch.float32)
    loss = module_loss(P, *module_data(torch.float32))
    g32 = dict(zip(P, torch.autograd.grad(loss, list(P.values()))))
    ref = module_reference()[1]
    return {k: rel_err(g32[k], ref[k]) for k in P}
