"""Cases, float64 references and bounds of the training backward: the resize and pool backward kernels, the fused Charbonnier loss and
the CRFP_DSV model gradients (tests/test_train_backward_cases.py pins them on the CPU, tests/test_gpu_train_backward.py,
test_gpu_charbonnier.py and test_gpu_train_model.py run them on the device).

Pass rule, per gradient tensor (the project's existing one): max|gpu - ref64| <= TOL * max|ref64|, TOL = 8 * max(E32, one ulp), E32 = the
error of the same graph in float32 on the CPU (ATen) against float64.  TOL is computed here from that CPU run, never from the device.

The references are ATen's float64 autograd of F.interpolate(mode='bilinear', align_corners=False) (* mul), F.avg_pool2d(2, 2), the
Charbonnier formula of loss/loss.py, and oracle.crfp_oracle.crfp_dsv_forward for the model.

Exact cases: scales 2, 4, 8 with integer grad_out in [-8, 8]: every weight is dyadic, so any summation order is exact and the gradient must
equal the float64 one bit for bit (float32 ATen autograd already does: the CPU test asserts it).

Measured (E32 = the CPU float32 graph's error -> TOL; device errors on an MI355X):
  resize: E32 6.6e-08 .. 4.1e-07 at the scales, 6.8e-07 / 1.4e-06 in size mode (float32 in / out ratio), 0 for the identity and the exact cases;
          device errors 0 .. 4e-07, the exact cases and the identity bit-equal to float64.
  pool: E32 0 (0.25 * g is exact); the device equals float64 bit for bit.
  charbonnier: TOL 9.5e-07 .. 1.4e-06; device loss errors <= 3e-08, gradient errors <= 1.3e-07.
  model A (mid 32, 1x3x20x24): worst E32 7.76e-03 (dcn_3.upsample.upsample_conv.bias: bilinear cell crossings), worst TOL 6.21e-02; device forward
          error 2.9e-07, all 118 gradients inside their TOL, worst against its TOL dcn_3.dcn_mask.bias 1.2e-05 of 4.3e-05, largest error 7.8e-03.
  model B (mid 16, y_only, 2x2x12x16): worst E32 5.8e-05 (dcn_3.dcn_block.2.weight), worst TOL 4.6e-04; all 118 device gradients inside their TOL.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from crfp_amd import synth
from oracle import crfp_oracle as orc

ULP = 2.0 ** -23

# ---- resize: n, c, h, w and either scale (+ mul) or size
RESIZE = {}
for _s, _m in ((2, 2.0), (4, 1.0), (8, 8.0)):
    for _h, _w in ((1, 5), (3, 1), (5, 7)):
        RESIZE[f"s{_s}_{_h}x{_w}"] = dict(n=2, c=3, h=_h, w=_w, scale=_s, mul=_m)
RESIZE["size_16x24_20x24"] = dict(n=2, c=3, h=16, w=24, size=(20, 24), mul=1.0)     # FNet's tail at h = 20
RESIZE["size_8x20_11x23"] = dict(n=2, c=3, h=8, w=20, size=(11, 23), mul=1.0)
RESIZE["identity_6x9"] = dict(n=2, c=3, h=6, w=9, size=(6, 9), mul=1.0)
RESIZE["down_9x7_5x4"] = dict(n=2, c=3, h=9, w=7, size=(5, 4), mul=1.0)
EXACT = {f"exact_s{_s}": dict(n=2, c=3, h=5, w=7, scale=_s, mul=_m, exact=True) for _s, _m in ((2, 2.0), (4, 1.0), (8, 8.0))}
RESIZE_ALL = {**RESIZE, **EXACT}

POOL = {"4x6": dict(n=2, c=3, h=4, w=6), "5x7": dict(n=2, c=3, h=5, w=7), "2x3": dict(n=2, c=3, h=2, w=3),
        "45x80": dict(n=1, c=2, h=45, w=80)}   # floor to 22 rows


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def out_size(c):
    return (int(c["h"] * c["scale"]), int(c["w"] * c["scale"])) if "scale" in c else tuple(c["size"])


def src_scales(c):
    """the source-index scales the C-ABI takes (crfp_amd.ops.upsample_bilinear's): 1 / scale_factor, or in / out formed in float32"""
    if "scale" in c:
        return 1.0 / c["scale"], 1.0 / c["scale"]
    oh, ow = c["size"]
    return float(np.float32(c["h"]) / np.float32(oh)), float(np.float32(c["w"]) / np.float32(ow))


@functools.lru_cache(maxsize=None)
def resize_leaves(name):
    c = RESIZE_ALL[name]
    rs = np.random.RandomState(_seed(name))
    oh, ow = out_size(c)
    x = torch.from_numpy(rs.standard_normal((c["n"], c["c"], c["h"], c["w"])).astype(np.float32))
    if c.get("exact"):
        go = torch.from_numpy(rs.randint(-8, 9, (c["n"], c["c"], oh, ow)).astype(np.float32))
    else:
        go = torch.from_numpy(rs.standard_normal((c["n"], c["c"], oh, ow)).astype(np.float32))
    return x, go


def resize_graph(c, x):
    kw = dict(scale_factor=c["scale"]) if "scale" in c else dict(size=tuple(c["size"]))
    return F.interpolate(x, mode="bilinear", align_corners=False, **kw) * c["mul"]


def _resize_grad(name, dtype):
    c = RESIZE_ALL[name]
    x, go = resize_leaves(name)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    resize_graph(c, x).backward(go.to(dtype))
    return x.grad


@functools.lru_cache(maxsize=None)
def resize_reference(name):
    return _resize_grad(name, torch.float64)


@functools.lru_cache(maxsize=None)
def pool_leaves(name):
    c = POOL[name]
    rs = np.random.RandomState(_seed("pool" + name))
    x = torch.from_numpy(rs.standard_normal((c["n"], c["c"], c["h"], c["w"])).astype(np.float32))
    go = torch.from_numpy(rs.standard_normal((c["n"], c["c"], c["h"] // 2, c["w"] // 2)).astype(np.float32))
    return x, go


def _pool_grad(name, dtype):
    x, go = pool_leaves(name)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    F.avg_pool2d(x, 2, 2).backward(go.to(dtype))
    return x.grad


@functools.lru_cache(maxsize=None)
def pool_reference(name):
    return _pool_grad(name, torch.float64)


def rel_err(got, ref):
    ref = ref.detach().double().cpu()
    d = float((got.detach().double().cpu() - ref).abs().max())
    m = float(ref.abs().max())
    return d / m if m > 0 else d


def _tol(e32):
    return 8.0 * max(e32, ULP)


@functools.lru_cache(maxsize=None)
def resize_e32(name):
    return rel_err(_resize_grad(name, torch.float32), resize_reference(name))


@functools.lru_cache(maxsize=None)
def pool_e32(name):
    return rel_err(_pool_grad(name, torch.float32), pool_reference(name))


def resize_tol(name):
    return _tol(resize_e32(name))


def pool_tol(name):
    return _tol(pool_e32(name))


# ---- Charbonnier: shapes x weight variants x reductions
CB_SHAPES = {"1x3x5x7": (1, 3, 5, 7), "3x3x16x24": (3, 3, 16, 24)}   # the first: an element count that is no multiple of a wave
CB_WEIGHTS = ("none", "n1hw", "nchw")
CB_REDUCTIONS = (("mean", False), ("sum", False), ("mean", True))   # (reduction, sample_wise)
CB_EPS = 1e-12
CB_LOSS_WEIGHT = 0.75
CB_CASES = [(s, wk, r, sw) for s in CB_SHAPES for wk in CB_WEIGHTS for r, sw in CB_REDUCTIONS]


def cb_id(case):
    s, wk, r, sw = case
    return f"{s}-{wk}-{r}{'-samplewise' if sw else ''}"


@functools.lru_cache(maxsize=None)
def cb_leaves(shape, wkind):
    n, c, h, w = CB_SHAPES[shape]
    rs = np.random.RandomState(_seed("cb" + shape))
    pred = torch.from_numpy(rs.rand(n, c, h, w).astype(np.float32))
    target = torch.from_numpy(rs.rand(n, c, h, w).astype(np.float32))
    w01 = torch.from_numpy((rs.rand(n, 1, h, w) < 0.6).astype(np.float32))
    wfr = torch.from_numpy(rs.rand(n, c, h, w).astype(np.float32))
    return pred, target, {"none": None, "n1hw": w01, "nchw": wfr}[wkind]


def cb_formula(pred, target, weight, reduction, sample_wise, eps=CB_EPS):
    """loss/loss.py:26-68 on sqrt((pred - target)^2 + eps), restated"""
    loss = torch.sqrt((pred - target) ** 2 + eps)
    if weight is not None:
        loss = loss * weight
    if weight is None or reduction == "sum":
        return loss.mean() if reduction == "mean" else loss.sum()
    wexp = weight.expand_as(loss)
    if sample_wise:
        ws = wexp.sum(dim=[1, 2, 3], keepdim=True)
        return (loss / (ws + 1e-12)).sum() / ws.size(0)
    return loss.sum() / (wexp.sum() + 1e-12)


def _cb_run(case, dtype):
    shape, wkind, reduction, sample_wise = case
    pred, target, weight = cb_leaves(shape, wkind)
    pred = pred.detach().clone().to(dtype).requires_grad_(True)
    loss = CB_LOSS_WEIGHT * cb_formula(pred, target.to(dtype), None if weight is None else weight.to(dtype), reduction, sample_wise)
    loss.backward()
    return loss.detach(), pred.grad


@functools.lru_cache(maxsize=None)
def cb_reference(case):
    """(loss, grad_pred) in float64"""
    return _cb_run(case, torch.float64)


@functools.lru_cache(maxsize=None)
def cb_tol(case):
    """(TOL of the loss value, TOL of grad_pred)"""
    l64, g64 = cb_reference(case)
    l32, g32 = _cb_run(case, torch.float32)
    return _tol(abs(float(l32) - float(l64)) / abs(float(l64))), _tol(rel_err(g32, g64))


# ---- the model: Charbonnier mean of CRFP_DSV's output against a seeded HR target, every parameter's gradient
MODEL = {
    "A": dict(mid=32, y_only=False, weights_seed=3, clip_seed=5, n=1, t=3, h=20, w=24, fv_size=64),   # h = 20: FNet's tail is a real 16 -> 20 resize
    "B": dict(mid=16, y_only=True, weights_seed=3, clip_seed=5, n=2, t=2, h=12, w=16, fv_size=64),    # the smallest size FNet's three pools leave a pixel of
}
MODEL_FWD_BOUND = 2e-4    # forward_train against the float64 oracle: the bound of the composed-route tests
MODEL_TOL_CAP = 0.1       # no tensor's TOL may exceed it (the CPU test asserts it)


@functools.lru_cache(maxsize=None)
def model_leaves(name):
    """(state_dict as numpy, lrs, fvs, mks, hr target) -- float32 / bool CPU tensors"""
    c = MODEL[name]
    sd = synth.make_state_dict(c["weights_seed"], c["mid"], c["y_only"])
    lrs, fvs, mks = (torch.from_numpy(a) for a in synth.make_clip(c["clip_seed"], c["n"], c["t"], c["h"], c["w"], fv_size=c["fv_size"]))
    cout = 1 if c["y_only"] else 3
    hr = torch.from_numpy(np.random.RandomState(1).rand(c["n"], c["t"], cout, 8 * c["h"], 8 * c["w"]).astype(np.float32))
    return sd, lrs, fvs, mks, hr


def model_loss(out, hr):
    """Charbonnier mean (torch formula) of out [n,t,c,H,W] against hr"""
    return cb_formula(out.reshape(-1, *out.shape[2:]), hr.reshape(-1, *hr.shape[2:]), None, "mean", False)


def _model_run(name, dtype):
    c = MODEL[name]
    sd, lrs, fvs, mks, hr = model_leaves(name)
    P = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    out = orc.crfp_dsv_forward(P, lrs.to(dtype), fvs.to(dtype), mks, orc.DSVConfig(c["mid"], y_only=c["y_only"]))
    loss = model_loss(out, hr.to(dtype))
    loss.backward()
    return out.detach(), float(loss.detach()), {k: v.grad for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def model_reference(name):
    """(out, loss, {parameter: gradient}) of the float64 oracle"""
    return _model_run(name, torch.float64)


@functools.lru_cache(maxsize=None)
def model_e32(name):
    _, _, g64 = model_reference(name)
    _, _, g32 = _model_run(name, torch.float32)
    return {k: rel_err(g32[k], g64[k]) for k in g64}


def model_tol(name):
    return {k: _tol(e) for k, e in model_e32(name).items()}
