"""GPU: the resize and pool backward (crfp_upsample_bilinear_backward_f32 / crfp_avgpool2_backward_f32, and ops.upsample_bilinear /
ops.avgpool2 under autograd) on the cases of tests/helpers/train_backward_cases.py against their float64 gradients; pass test per
gradient tensor: max|gpu - ref64| <= TOL * max|ref64|, TOL = 8 * max(the float32 CPU graph's own error, one ulp)."""
import math

import pytest
import torch

from helpers import train_backward_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT, PAD = -7777.25, 4099


def _lib():
    from crfp_amd import _lib
    return _lib, _lib.lib()


def abi_resize(name, go=None, side_stream=False, guards=False):
    """crfp_upsample_bilinear_backward_f32 on the case (its own grad_out, or `go`): grad_x, inside a sentinel-filled buffer with guards"""
    L, lib = _lib()
    c = tc.RESIZE_ALL[name]
    oh, ow = tc.out_size(c)
    sh, sw = tc.src_scales(c)
    go = (tc.resize_leaves(name)[1] if go is None else go).to(DEV).contiguous()
    numel = c["n"] * c["c"] * c["h"] * c["w"]
    pad = PAD if guards else 0
    buf = torch.full((numel + 2 * pad,), SENT, dtype=torch.float32, device=DEV)
    view = buf[pad:pad + numel]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV) if side_stream else torch.cuda.current_stream()
    L.check(lib.crfp_upsample_bilinear_backward_f32(go.data_ptr(), view.data_ptr(), c["n"], c["c"], c["h"], c["w"], oh, ow, sh, sw, c["mul"],
                                                    stream.cuda_stream), "crfp_upsample_bilinear_backward_f32")
    stream.synchronize()
    torch.cuda.synchronize()
    g = view.reshape(c["n"], c["c"], c["h"], c["w"])
    return (g, buf) if guards else g


def abi_pool(name, go=None, side_stream=False, guards=False):
    L, lib = _lib()
    c = tc.POOL[name]
    go = (tc.pool_leaves(name)[1] if go is None else go).to(DEV).contiguous()
    numel = c["n"] * c["c"] * c["h"] * c["w"]
    pad = PAD if guards else 0
    buf = torch.full((numel + 2 * pad,), SENT, dtype=torch.float32, device=DEV)
    view = buf[pad:pad + numel]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV) if side_stream else torch.cuda.current_stream()
    L.check(lib.crfp_avgpool2_backward_f32(go.data_ptr(), view.data_ptr(), c["n"], c["c"], c["h"], c["w"], stream.cuda_stream),
            "crfp_avgpool2_backward_f32")
    stream.synchronize()
    torch.cuda.synchronize()
    g = view.reshape(c["n"], c["c"], c["h"], c["w"])
    return (g, buf) if guards else g


def ops_resize(c, x, **kw):
    from crfp_amd import ops
    if "scale" in c:
        return ops.upsample_bilinear(x, scale_factor=c["scale"], mul=c["mul"], **kw)
    return ops.upsample_bilinear(x, size=tuple(c["size"]), mul=c["mul"], **kw)


def autograd_resize(name):
    c = tc.RESIZE_ALL[name]
    x, go = tc.resize_leaves(name)
    x = x.clone().to(DEV).requires_grad_(True)
    out = ops_resize(c, x)
    assert out.grad_fn is not None
    out.backward(go.to(DEV))
    return x.grad


def autograd_pool(name):
    from crfp_amd import ops
    x, go = tc.pool_leaves(name)
    x = x.clone().to(DEV).requires_grad_(True)
    out = ops.avgpool2(x)
    assert out.grad_fn is not None
    out.backward(go.to(DEV))
    return x.grad


def check(what, name, g, ref, tol):
    err = tc.rel_err(g, ref)
    print(f"train_backward {what} {name}: {err:.2e} (tol {tol:.2e})")
    assert g.shape == ref.shape and bool(torch.isfinite(g).all())
    assert err <= tol, (what, name, err, tol)


@pytest.mark.parametrize("name", list(tc.RESIZE))
def test_resize_gradients_match_float64(name):
    """every resize case through the C-ABI and through autograd"""
    ref, tol = tc.resize_reference(name), tc.resize_tol(name)
    g = abi_resize(name)
    check("resize c-abi", name, g, ref, tol)
    ga = autograd_resize(name)
    check("resize autograd", name, ga, ref, tol)
    assert torch.equal(g, ga)


@pytest.mark.parametrize("name", list(tc.EXACT))
def test_exact_cases_equal_float64_bit_for_bit(name):
    """integer grad_out, dyadic weights: any summation order is exact"""
    ref = tc.resize_reference(name).float().to(DEV)
    assert torch.equal(abi_resize(name), ref)
    assert torch.equal(autograd_resize(name), ref)


@pytest.mark.parametrize("name", list(tc.POOL))
def test_pool_gradients_match_float64(name):
    """every pool case through the C-ABI and through autograd; 0.25 * g is exact, so the float64 gradient bit for bit, the dropped odd row
    and column an exact zero"""
    ref, tol = tc.pool_reference(name), tc.pool_tol(name)
    g, ga = abi_pool(name), autograd_pool(name)
    check("pool c-abi", name, g, ref, tol)
    check("pool autograd", name, ga, ref, tol)
    assert torch.equal(g, ref.float().to(DEV)) and torch.equal(ga, g)
    c = tc.POOL[name]
    assert bool((g[:, :, 2 * (c["h"] // 2):] == 0).all()) and bool((g[:, :, :, 2 * (c["w"] // 2):] == 0).all())


@pytest.mark.parametrize("name", ["s2_5x7", "s8_1x5", "s4_3x1", "size_16x24_20x24", "size_8x20_11x23", "down_9x7_5x4"])
def test_resize_adjoint_identity(name):
    """<up(x), g> == <x, up_backward(g)> with the library's own forward, both sums in float64 on the host.  Bound from the operand magnitudes
    and the term count: the forward rounds each output at most 8 times on terms bounded by mul * max|x| (weights sum to one), the backward
    each input's sum of at most K terms K + 8 times, K = the candidate outputs of one input; A = up_backward(|g|) bounds the magnitude
    of those terms."""
    c = tc.RESIZE_ALL[name]
    x, go = tc.resize_leaves(name)
    with torch.no_grad():
        y = ops_resize(c, x.to(DEV)).double().cpu()
    gx = abi_resize(name).double().cpu()
    A = abi_resize(name, go=go.abs()).double().cpu()
    lhs, rhs = float((y * go.double()).sum()), float((x.double() * gx).sum())
    sh, sw = tc.src_scales(c)
    K = (math.ceil(2 / sh) + 3) * (math.ceil(2 / sw) + 3)
    bound = tc.ULP * (8 * abs(c["mul"]) * float(x.abs().max()) * float(go.abs().sum()) + (K + 8) * float((x.double().abs() * A).sum()))
    print(f"train_backward adjoint {name}: |lhs - rhs| {abs(lhs - rhs):.3e}, bound {bound:.3e}, lhs {lhs:.6f}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("name", ["5x7", "45x80"])
def test_pool_adjoint_identity(name):
    """<pool(x), g> == <x, pool_backward(g)>: the forward rounds each output 4 times on terms bounded by max|x|, the backward is exact"""
    from crfp_amd import ops
    x, go = tc.pool_leaves(name)
    with torch.no_grad():
        y = ops.avgpool2(x.to(DEV)).double().cpu()
    gx = abi_pool(name).double().cpu()
    lhs, rhs = float((y * go.double()).sum()), float((x.double() * gx).sum())
    bound = tc.ULP * 4 * float(x.abs().max()) * float(go.abs().sum())
    print(f"train_backward pool adjoint {name}: |lhs - rhs| {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_two_runs_guards_and_side_stream_give_the_same_bits():
    """two runs are bit-identical; the outputs sit inside sentinel-filled buffers, every element of them is written and nothing outside
    changes; a side stream gives the same bits"""
    for name in ("s8_5x7", "s2_1x5", "size_8x20_11x23", "down_9x7_5x4", "identity_6x9"):
        base = abi_resize(name)
        (g, buf), side = abi_resize(name, guards=True), abi_resize(name, side_stream=True)
        assert torch.equal(base, abi_resize(name)) and torch.equal(base, g) and torch.equal(base, side), name
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all()) and not bool((buf[PAD:-PAD] == SENT).any()), name
    for name in ("5x7", "2x3", "45x80"):
        base = abi_pool(name)
        (g, buf), side = abi_pool(name, guards=True), abi_pool(name, side_stream=True)
        assert torch.equal(base, abi_pool(name)) and torch.equal(base, g) and torch.equal(base, side), name
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all()) and not bool((buf[PAD:-PAD] == SENT).any()), name


def test_an_input_no_output_reads_gets_an_exact_zero():
    """9 x 7 -> 2 x 2: most inputs lie in no output's footprint; the float64 gradient has exact zeros there and so has the kernel's"""
    L, lib = _lib()
    x = torch.randn(1, 2, 9, 7, dtype=torch.float64, requires_grad=True)
    go = torch.randn(1, 2, 2, 2)
    torch.nn.functional.interpolate(x, size=(2, 2), mode="bilinear", align_corners=False).backward(go.double())
    gx = torch.full((1, 2, 9, 7), SENT, dtype=torch.float32, device=DEV)
    god = go.to(DEV)
    L.check(lib.crfp_upsample_bilinear_backward_f32(god.data_ptr(), gx.data_ptr(), 1, 2, 9, 7, 2, 2, 4.5, 3.5, 1.0,
                                                    torch.cuda.current_stream().cuda_stream), "crfp_upsample_bilinear_backward_f32")
    torch.cuda.synchronize()
    zero = x.grad == 0
    assert int(zero.sum()) > 0 and bool((gx.cpu()[zero] == 0).all())
    assert tc.rel_err(gx, x.grad) <= 8 * tc.ULP   # the rule's floor: at these scales (4.5, 3.5) every weight is dyadic


def test_refusal_codes():
    """every argument error comes back as its negative code (before any HIP call: the pointers below are never dereferenced)"""
    _, lib = _lib()
    t = torch.zeros(64, device=DEV)
    p, s = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    up = lib.crfp_upsample_bilinear_backward_f32
    BADARG, UNSUPPORTED = -1, -3
    assert up(None, p, 1, 1, 2, 2, 4, 4, 0.5, 0.5, 1.0, s) == BADARG and up(p, None, 1, 1, 2, 2, 4, 4, 0.5, 0.5, 1.0, s) == BADARG
    for bad in ((0, 1, 2, 2, 4, 4), (1, 0, 2, 2, 4, 4), (1, 1, 0, 2, 4, 4), (1, 1, 2, 0, 4, 4), (1, 1, 2, 2, 0, 4), (1, 1, 2, 2, 4, 0)):
        assert up(p, p, *bad, 0.5, 0.5, 1.0, s) == BADARG, bad
    for sh, sw in ((0.0, 0.5), (0.5, -1.0), (float("nan"), 0.5), (0.5, float("inf"))):
        assert up(p, p, 1, 1, 2, 2, 4, 4, sh, sw, 1.0, s) == BADARG, (sh, sw)
    assert up(p, p, 65536, 1, 2, 2, 4, 4, 0.5, 0.5, 1.0, s) == UNSUPPORTED and up(p, p, 256, 256, 2, 2, 4, 4, 0.5, 0.5, 1.0, s) == UNSUPPORTED
    assert up(p, p, 1, 1, 262141, 2, 4, 4, 0.5, 0.5, 1.0, s) == UNSUPPORTED
    assert b"upsample_backward" in lib.crfp_last_error_string()
    pool = lib.crfp_avgpool2_backward_f32
    assert pool(None, p, 1, 1, 2, 2, s) == BADARG and pool(p, None, 1, 1, 2, 2, s) == BADARG
    for bad in ((0, 1, 2, 2), (1, 0, 2, 2), (1, 1, 1, 2), (1, 1, 2, 1)):
        assert pool(p, p, *bad, s) == BADARG, bad
    assert pool(p, p, 65536, 1, 2, 2, s) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((t == 0).all())


def test_no_grad_paths_are_the_plain_forward():
    """grad mode off, or nothing requiring grad: no grad_fn, and bit for bit the grad-mode forward"""
    from crfp_amd import ops
    for name in ("s8_5x7", "size_16x24_20x24", "down_9x7_5x4"):
        c = tc.RESIZE_ALL[name]
        x = tc.resize_leaves(name)[0].to(DEV)
        req = x.clone().requires_grad_(True)
        with torch.no_grad():
            plain, off = ops_resize(c, x), ops_resize(c, req)
        none_req, on = ops_resize(c, x), ops_resize(c, req)
        assert off.grad_fn is None and none_req.grad_fn is None and not off.requires_grad and not none_req.requires_grad
        assert on.grad_fn is not None
        assert torch.equal(off, plain) and torch.equal(none_req, plain) and torch.equal(on.detach(), plain)
    for name in ("5x7", "45x80"):
        x = tc.pool_leaves(name)[0].to(DEV)
        req = x.clone().requires_grad_(True)
        with torch.no_grad():
            plain, off = ops.avgpool2(x), ops.avgpool2(req)
        none_req, on = ops.avgpool2(x), ops.avgpool2(req)
        assert off.grad_fn is None and none_req.grad_fn is None and on.grad_fn is not None
        assert torch.equal(off, plain) and torch.equal(none_req, plain) and torch.equal(on.detach(), plain)
