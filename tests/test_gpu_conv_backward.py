"""GPU: the conv3x3 backward (crfp_conv3x3_ex_backward_f32, and ops.conv3x3 / ops.conv3x3_ex under autograd) on the cases of
tests/conv_backward_cases.py against their float64 gradients; pass test per gradient tensor: max|gpu - ref64| <= TOL * max|ref64|,
TOL = 8 * max(the float32 CPU graph's own error, one ulp)."""
import itertools

import pytest
import torch

import conv_backward_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ABI_GRADS = ("x", "x2", "weight", "bias")   # the entry point's outputs (the residual's gradient is grad_out: no kernel)
SENT, PAD = -7777.25, 4099


def abi_tensors(name):
    return tuple(k for k in cc.tensors(name) if k != "residual")


def abi_run(name, needs=None, go_scale=1.0, nan_workspace=False, side_stream=False, guards=False):
    """crfp_conv3x3_ex_backward_f32 on the case with out = the float64 forward rounded to float32: {tensor: gradient} for `needs`
    (guards: also the sentinel-filled buffers the outputs sit in the middle of)"""
    from crfp_amd import _lib, ops
    lib = _lib.lib()
    c = cc.CASES[name]
    needs = abi_tensors(name) if needs is None else needs
    L = {k: (None if v is None else v.to(DEV).contiguous()) for k, v in cc.leaves(name).items()}
    out = None if c["act"] == "none" else cc.reference_out(name).float().to(DEV).contiguous()
    go = (L["grad_out"] * go_scale).contiguous()
    pad = PAD if guards else 0
    bufs = {k: torch.full((L[k].numel() + 2 * pad,), SENT, dtype=torch.float32, device=DEV) for k in needs}
    views = {k: bufs[k][pad:pad + L[k].numel()] for k in needs}
    nb = lib.crfp_conv3x3_ex_backward_workspace_bytes(c["n"], c["cin"], c["cin2"], c["cout"], c["h"], c["w"], c.get("unshuffle", 0), c.get("shuffle", 0))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    if nan_workspace:
        ws.fill_(0xFF)   # every float of it a NaN
    P = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV) if side_stream else torch.cuda.current_stream()
    need_w = "weight" in needs
    _lib.check(lib.crfp_conv3x3_ex_backward_f32(P(L["x"]) if need_w else None, c["cin"], P(L["x2"]) if need_w else None, c["cin2"],
                                                P(L["weight"]) if ("x" in needs or "x2" in needs) else None, P(out), P(go),
                                                *(P(views.get(k)) for k in ABI_GRADS), c["n"], c["cout"], c["h"], c["w"], ops.ACT[c["act"]],
                                                float(c["s"]), c.get("unshuffle", 0), c.get("shuffle", 0), ws.data_ptr(), nb, stream.cuda_stream),
               "crfp_conv3x3_ex_backward_f32")
    stream.synchronize()
    torch.cuda.synchronize()
    grads = {k: views[k].reshape(L[k].shape) for k in needs}
    return (grads, bufs) if guards else grads


def ex_fn(name):
    """the case through ops.conv3x3_ex: fn(x, x2, weight, bias, residual) -> out"""
    from crfp_amd import ops
    c = cc.CASES[name]
    return lambda x, x2, weight, bias, residual, **kw: ops.conv3x3_ex(x, weight, bias, x2=x2, residual=residual, act=c["act"], post_scale=c["s"],
                                                                       unshuffle=c.get("unshuffle", 0), shuffle=c.get("shuffle", 0), **kw)


def plain_fn(name):
    """a one-input case through ops.conv3x3"""
    from crfp_amd import ops
    c = cc.CASES[name]
    return lambda x, x2, weight, bias, residual: ops.conv3x3(x, weight, bias, c["act"], c["s"])


def ops_run(name, fn, needs=None):
    """fn on the case's float32 device leaves through backward(grad_out): {tensor: gradient or None}, out"""
    L = cc.leaves(name)
    needs = cc.tensors(name) if needs is None else needs
    t = {k: (None if L[k] is None else L[k].clone().to(DEV).requires_grad_(k in needs)) for k in cc.GRADS}
    out = fn(*(t[k] for k in cc.GRADS))
    out.backward(L["grad_out"].to(DEV))
    return {k: t[k].grad for k in cc.tensors(name)}, out.detach()


def check(what, name, grads, ref, tensors):
    errs = {k: cc.rel_err(grads[k], ref[k]) for k in tensors}
    print(f"conv_backward {what} {name}: " + ", ".join(f"{k} {errs[k]:.2e} (tol {cc.TOL[name][k]:.2e})" for k in tensors))
    for k in tensors:
        assert grads[k].shape == ref[k].shape and bool(torch.isfinite(grads[k]).all())
        assert errs[k] <= cc.TOL[name][k], (name, k, errs[k], cc.TOL[name][k])


@pytest.mark.parametrize("name", list(cc.CASES))
def test_c_abi_gradients_match_float64(name):
    """1: every case and tensor through the C-ABI, out = the float64 forward rounded to float32"""
    check("c-abi", name, abi_run(name), cc.reference(name), abi_tensors(name))


@pytest.mark.parametrize("name", list(cc.CASES))
def test_autograd_gradients_match_float64_from_the_forwards_out(name):
    """2: through ops.conv3x3_ex under autograd (and ops.conv3x3 for the one-input cases) against the float64 gradients whose activation
    derivative is taken from the forward kernel's own output"""
    routes = [("conv3x3_ex", ex_fn(name))] + ([("conv3x3", plain_fn(name))] if name in cc.ONE_INPUT else [])
    for what, fn in routes:
        grads, out = ops_run(name, fn)
        assert float((out.double().cpu() - cc.reference_out(name)).abs().max()) <= 1e-4 * float(cc.reference_out(name).abs().max())   # the forward it differentiates
        check(what, name, grads, cc.reference_from_out(name, out), cc.tensors(name))
    if cc.CASES[name].get("resid"):
        assert torch.equal(grads["residual"].cpu(), cc.leaves(name)["grad_out"])


@pytest.mark.parametrize("name", ["odd", "wide"])
def test_scaling_grad_out_by_a_power_of_two_is_exact(name):
    """3: grad_out * 2^-40 and * 2^20 scale every gradient by that power of two bit for bit: no operand passes through fp16"""
    base = abi_run(name)
    for e in (-40, 20):
        scaled = abi_run(name, go_scale=2.0 ** e)
        for k in abi_tensors(name):
            assert float(base[k].abs().max()) > 0
            assert torch.equal(scaled[k], base[k] * 2.0 ** e), (name, e, k)


def test_two_runs_and_every_subset_give_the_same_bits():
    """4: two runs are bit-identical in all four gradients, and every subset of the outputs gives the full run's bits"""
    for name in ("odd", "cat66", "slabs", "unshuffle4"):
        full, again = abi_run(name), abi_run(name)
        for k in abi_tensors(name):
            assert torch.equal(full[k], again[k]), (name, k)
    for name in ("odd", "wide"):
        full = abi_run(name)
        for m in range(1, 4):
            for needs in itertools.combinations(ABI_GRADS, m):
                part = abi_run(name, needs)
                for k in needs:
                    assert torch.equal(part[k], full[k]), (name, needs, k)
    # and through autograd's needs_input_grad
    full, _ = ops_run("odd", ex_fn("odd"))
    for needs in (("x",), ("x2",), ("weight",), ("bias",), ("x2", "bias"), ("x", "weight")):
        part, _ = ops_run("odd", ex_fn("odd"), needs)
        for k in cc.tensors("odd"):
            assert (part[k] is None) if k not in needs else torch.equal(part[k], full[k]), (needs, k)


def test_c_abi_writes_inside_its_outputs_only():
    """4: the outputs sit in the middle of sentinel-filled buffers; every sentinel stays intact, every output element is written"""
    for name in ("odd", "unshuffle4", "wide", "line", "column", "shuffle4"):
        grads, bufs = abi_run(name, guards=True)
        check("guards", name, grads, cc.reference(name), abi_tensors(name))
        for k, b in bufs.items():
            assert bool((b[:PAD] == SENT).all()) and bool((b[-PAD:] == SENT).all()), (name, k)
            assert not bool((b[PAD:-PAD] == SENT).any()), (name, k)


def test_dirty_workspace_and_side_stream_give_the_same_bits():
    """4: a workspace pre-filled with NaN bytes and a non-default stream change nothing"""
    for name in ("odd", "cat66", "slabs", "shuffle2"):
        base = abi_run(name)
        dirty = abi_run(name, nan_workspace=True, side_stream=True)
        for k in abi_tensors(name):
            assert bool(torch.isfinite(dirty[k]).all()) and torch.equal(base[k], dirty[k]), (name, k)


def test_no_grad_paths_are_the_plain_forward():
    """5: grad mode off, or nothing requiring grad: no grad_fn, and bit for bit the grad-mode forward; `out=` and a residual with an
    activation are refused under grad"""
    from crfp_amd import ops
    for name in ("odd", "resid", "shuffle2", "unshuffle4", "tanh"):
        routes = [ex_fn(name)] + ([plain_fn(name)] if name in cc.ONE_INPUT else [])
        for fn in routes:
            L = cc.leaves(name)
            args = [None if L[k] is None else L[k].to(DEV) for k in cc.GRADS]
            req = [None if a is None else a.clone().requires_grad_(True) for a in args]
            with torch.no_grad():
                plain = fn(*args)
                off = fn(*req)
            none_req = fn(*args)
            on = fn(*req)
            assert off.grad_fn is None and none_req.grad_fn is None and not off.requires_grad and not none_req.requires_grad
            assert on.grad_fn is not None
            assert torch.equal(off, plain) and torch.equal(none_req, plain) and torch.equal(on.detach(), plain)
    L = {k: (None if v is None else v.to(DEV)) for k, v in cc.leaves("resid").items()}
    w = L["weight"].clone().requires_grad_(True)
    dst = torch.zeros(2, 8, 9, 11, device=DEV)
    with pytest.raises(RuntimeError):
        ops.conv3x3_ex(L["x"], w, L["bias"], out=dst)
    with torch.no_grad():
        assert ops.conv3x3_ex(L["x"], w, L["bias"], out=dst) is dst
    with pytest.raises(NotImplementedError, match="lrelu"):
        ops.conv3x3_ex(L["x"], w, L["bias"], residual=L["residual"], act="lrelu")
    with torch.no_grad():
        ops.conv3x3_ex(L["x"], w, L["bias"], residual=L["residual"], act="lrelu")


def _module(name):
    from crfp_amd.model import CRFP
    m = {"dcn8": lambda: CRFP.DCN_module(8, dg=2, pre_offset=True, interpolate="none"),
         "dcn4": lambda: CRFP.DCN_module(4, 1, repeat=True, pre_offset=True, interpolate="pixelshuffle"),
         "resblock": lambda: CRFP.ResidualBlocksWithInputConv(16, 8, 1)}[name]()
    m.load_state_dict(cc.module_leaves(name)[0], strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("name", list(cc.MODULES))
def test_modules_train(name):
    """6: the module in float32 on the device against the same graph in float64 on the CPU (F.conv2d and the oracle's dcnv2), squared-error
    loss: every parameter and every input gets a finite, non-zero gradient within 8 * max(E32, EFWD, one ulp) of float64, and one SGD step
    on the parameters lowers the loss."""
    _, I0, targets = cc.module_leaves(name)
    loss_ref, gref, _, outs_ref = cc.module_reference(name)
    m = _module(name)
    I = {k: v.clone().to(DEV).requires_grad_(True) for k, v in I0.items()}
    order = cc.MODULE_INPUTS[cc.MODULES[name]["kind"]]

    def forward():
        outs = m(*(I[k] for k in order))
        return outs if isinstance(outs, tuple) else (outs,)

    outs = forward()
    efwd = max(cc.rel_err(o, r) for o, r in zip(outs, outs_ref))
    loss = cc.module_loss(outs, targets)
    loss.backward()
    grads = {**{k: p.grad for k, p in m.named_parameters()}, **{k: v.grad for k, v in I.items()}}
    assert set(grads) == set(gref)
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    errs = {k: cc.rel_err(grads[k], gref[k]) for k in gref}
    print(f"conv_backward module {name}: forward error {efwd:.2e} (written down {cc.MODULE_EFWD[name]:.2e}), loss {float(loss.detach()):.6f} (float64 {loss_ref:.6f})")
    print(f"conv_backward module {name}: " + ", ".join(f"{k} {errs[k]:.2e} (tol {cc.module_tol(name, k):.2e})" for k in errs))
    with torch.no_grad():
        for p in m.parameters():
            p -= cc.MODULE_LR * p.grad
        loss2 = cc.module_loss(forward(), targets)
    assert float(loss2) < float(loss.detach())
    assert efwd <= 2 * cc.MODULE_EFWD[name]   # the written-down forward error is the measured one
    for k in gref:
        assert errs[k] <= cc.module_tol(name, k), (name, k, errs[k], cc.module_tol(name, k))
