"""GPU: the flow_warp backward (crfp_flow_warp_backward_f32 through ops.flow_warp under autograd) and the shared-offset DCNv2 backward
(crfp_dcnv2_shared_backward_f32 through ops.dcnv2_shared) on the cases of tests/warp_backward_cases.py against their float64 oracle
gradients; pass test per gradient tensor: max|gpu - ref64| <= TOL * max|ref64|, TOL = 8 * max(the oracle's own fp32 error, one ulp)."""
import pytest
import torch

import warp_backward_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASE_MODES = [(name, mode) for name in wc.CASES for mode in wc.MODES]
SHARED_DETERMINISTIC = ("offset", "mask", "weight", "bias")
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3


def warp_fn(x, flow, mode):
    from crfp_amd import ops
    return ops.flow_warp(x, flow, padding_mode=mode)


def shared_fn(x, offset, mask, weight, bias):
    from crfp_amd import ops
    return ops.dcnv2_shared(x, offset, mask, weight, bias)


def tiled_fn(x, offset, mask, weight, bias):
    """the route to the same gradients before the shared backward: ops.dcnv2 on the 9x-tiled tensors"""
    from crfp_amd import ops
    return ops.dcnv2(x, offset.repeat(1, 9, 1, 1), mask.repeat(1, 9, 1, 1), weight, bias, 3, 1, 1, 1)


def gpu_run(name, mode, needs=wc.GRADS):
    return wc.run(warp_fn, name, mode, torch.float32, DEV, needs)


def check(name, mode, grads, tensors=wc.GRADS):
    ref = wc.reference(name, mode)
    errs = {k: wc.rel_err(grads[k], ref[k]) for k in tensors}
    print(f"warp_backward {name} {mode}: " + ", ".join(f"{k} {errs[k]:.2e} (tol {wc.TOL[name][mode][k]:.2e})" for k in tensors))
    for k in tensors:
        assert grads[k].shape == ref[k].shape and bool(torch.isfinite(grads[k]).all())
        assert errs[k] <= wc.TOL[name][mode][k], (name, mode, k, errs[k], wc.TOL[name][mode][k])


def check_shared(name, grads, tensors=wc.SHARED_GRADS, what="dcnv2_shared"):
    ref = wc.shared_reference(name)
    errs = {k: wc.rel_err(grads[k], ref[k]) for k in tensors}
    print(f"{what} backward {name}: " + ", ".join(f"{k} {errs[k]:.2e} (tol {wc.SHARED_TOL[name][k]:.2e})" for k in tensors))
    for k in tensors:
        assert grads[k].shape == ref[k].shape and bool(torch.isfinite(grads[k]).all())
        assert errs[k] <= wc.SHARED_TOL[name][k], (name, k, errs[k], wc.SHARED_TOL[name][k])


# ---------------------------------------------------------------- flow_warp
@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_gradients_match_the_float64_oracle(name, mode):
    """1: every case and mode, grad_x and grad_flow, through ops.flow_warp under autograd"""
    L = wc.leaves(name)
    x = L["x"].to(DEV).requires_grad_(True)
    assert warp_fn(x, L["flow"].to(DEV), mode).grad_fn is not None
    grads, out = gpu_run(name, mode)
    assert float((out.double().cpu() - wc.reference_out(name, mode)).abs().max()) < 1e-4   # the forward it differentiates
    check(name, mode, grads)
    if name == "nonfinite":   # the gradient of the constant the forward computes there
        g = grads["flow"][0].cpu()
        for y, xx, k, _ in wc.NONFINITE:
            assert float(g[y, xx, k]) == 0.0
        if mode == "zeros":
            assert float(g[wc.touched()].abs().max()) == 0.0


@pytest.mark.parametrize("name,mode", CASE_MODES)
def test_adjoint_of_the_forward_kernel(name, mode):
    """2: <grad_x, x> against <grad_out, ops.flow_warp(x, flow)> in float64 accumulation, relative to sum|grad_out * out|: the backward's
    cells and weights are the forward kernel's own"""
    L = {k: v.to(DEV) for k, v in wc.leaves(name).items()}
    grads, out = gpu_run(name, mode, ("x",))
    assert grads["flow"] is None
    lhs = float((grads["x"].double() * L["x"].double()).sum())
    terms = L["grad_out"].double() * out.double()
    rhs, scale = float(terms.sum()), float(terms.abs().sum())
    print(f"warp_backward adjoint {name} {mode}: |lhs - rhs| / sum|terms| = {abs(lhs - rhs) / scale:.2e} (tol {wc.TOL[name][mode]['x']:.2e})")
    assert abs(lhs - rhs) <= wc.TOL[name][mode]["x"] * scale


@pytest.mark.parametrize("mode", wc.MODES)
def test_no_grad_paths_are_the_plain_forward(mode):
    """3: grad mode off, or nothing requiring grad: no grad_fn, and bit for bit the grad-mode forward"""
    from crfp_amd import ops
    for name in ("odd", "c32"):
        L = {k: v.to(DEV) for k, v in wc.leaves(name).items()}
        with torch.no_grad():
            plain = ops.flow_warp(L["x"], L["flow"], padding_mode=mode)
        xr, fr = L["x"].clone().requires_grad_(True), L["flow"].clone().requires_grad_(True)
        with torch.no_grad():
            off = ops.flow_warp(xr, fr, padding_mode=mode)
        none_req = ops.flow_warp(L["x"], L["flow"], padding_mode=mode)
        on = ops.flow_warp(xr, fr, padding_mode=mode)
        assert off.grad_fn is None and none_req.grad_fn is None and not off.requires_grad and not none_req.requires_grad
        assert on.grad_fn is not None
        assert torch.equal(off, plain) and torch.equal(none_req, plain) and torch.equal(on.detach(), plain)


@pytest.mark.parametrize("mode", wc.MODES)
def test_needs_input_grad_subsets(mode):
    """4: only grad_flow, or only grad_x, gives the values of asking for both; grad_flow is bitwise equal across calls"""
    name = "wide"
    full, _ = gpu_run(name, mode)
    again, _ = gpu_run(name, mode)
    only_flow, _ = gpu_run(name, mode, ("flow",))
    only_x, _ = gpu_run(name, mode, ("x",))
    assert only_flow["x"] is None and only_x["flow"] is None
    assert torch.equal(full["flow"], again["flow"]) and torch.equal(full["flow"], only_flow["flow"])
    check(name, mode, only_x, ("x",))
    check(name, mode, only_flow, ("flow",))
    # grad_x is an atomic sum: the same values up to the order of a few float32 additions
    assert float((only_x["x"] - full["x"]).abs().max()) <= wc.TOL[name][mode]["x"] * float(full["x"].abs().max())


@pytest.mark.parametrize("mode", wc.MODES)
def test_zero_flow_passes_grad_out_through(mode):
    """5: image 0 of "integer" has no flow: grad_x is grad_out bit for bit"""
    grads, _ = gpu_run("integer", mode)
    assert torch.equal(grads["x"][0].cpu(), wc.leaves("integer")["grad_out"][0])


def test_window_placement_does_not_change_the_result():
    """the measurement hook (window on the undisplaced tile) computes the same gradients"""
    from crfp_amd import _lib
    lib = _lib.lib()
    name, mode = "wide", "zeros"
    c = wc.CASES[name]
    L = {k: v.to(DEV).contiguous() for k, v in wc.leaves(name).items()}
    ws = torch.empty(lib.crfp_flow_warp_backward_workspace_bytes(c["n"], c["c"], c["h"], c["w"]), dtype=torch.uint8, device=DEV)
    got = {}
    for window in (0, 1):
        gx, gflow = torch.empty_like(L["x"]), torch.empty_like(L["flow"])
        _lib.check(lib.crfp_flow_warp_backward_window_f32(L["x"].data_ptr(), L["flow"].data_ptr(), L["grad_out"].data_ptr(), gx.data_ptr(),
                                                          gflow.data_ptr(), c["n"], c["c"], c["h"], c["w"], 0, window, ws.data_ptr(), ws.numel(),
                                                          torch.cuda.current_stream().cuda_stream), "crfp_flow_warp_backward_window_f32")
        torch.cuda.synchronize()
        got[window] = dict(x=gx, flow=gflow)
        check(name, mode, got[window])
    assert torch.equal(got[0]["flow"], got[1]["flow"])


def test_c_abi_writes_inside_its_outputs_only():
    """Large motion through the C-ABI: both outputs are views in the middle of sentinel-filled tensors; every sentinel stays intact."""
    from crfp_amd import _lib
    lib = _lib.lib()
    SENT, PAD = -7777.25, 4099
    for name, mode in (("motion", 0), ("nonfinite", 1)):
        c = wc.CASES[name]
        L = {k: v.to(DEV).contiguous() for k, v in wc.leaves(name).items()}
        bufs = {k: torch.full((L[k].numel() + 2 * PAD,), SENT, dtype=torch.float32, device=DEV) for k in wc.GRADS}
        views = {k: bufs[k][PAD:PAD + L[k].numel()] for k in wc.GRADS}
        ws = torch.empty(lib.crfp_flow_warp_backward_workspace_bytes(c["n"], c["c"], c["h"], c["w"]), dtype=torch.uint8, device=DEV)
        _lib.check(lib.crfp_flow_warp_backward_f32(L["x"].data_ptr(), L["flow"].data_ptr(), L["grad_out"].data_ptr(), views["x"].data_ptr(),
                                                   views["flow"].data_ptr(), c["n"], c["c"], c["h"], c["w"], mode, ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream), "crfp_flow_warp_backward_f32")
        torch.cuda.synchronize()
        check(name, wc.MODES[mode], {k: views[k].reshape(L[k].shape) for k in wc.GRADS})
        for k in wc.GRADS:
            assert bool((bufs[k][:PAD] == SENT).all()) and bool((bufs[k][PAD + L[k].numel():] == SENT).all()), (name, k)


def test_argument_errors_on_the_device():
    """the refusals of both entry points with real device pointers: a CRFP_E_* code, nothing launched, the outputs untouched"""
    from crfp_amd import _lib
    lib = _lib.lib()
    c = wc.CASES["odd"]
    L = {k: v.to(DEV).contiguous() for k, v in wc.leaves("odd").items()}
    gx, gflow = torch.full_like(L["x"], 3.0), torch.full_like(L["flow"], 3.0)
    need = lib.crfp_flow_warp_backward_workspace_bytes(c["n"], c["c"], c["h"], c["w"])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr() if t is not None else None   # noqa: E731

    def warp(x=L["x"], gx_=gx, gflow_=gflow, mode=0, ws_=ws, nb=need):
        return lib.crfp_flow_warp_backward_f32(P(x), P(L["flow"]), P(L["grad_out"]), P(gx_), P(gflow_), c["n"], c["c"], c["h"], c["w"], mode,
                                               P(ws_), nb, s)

    assert warp(gx_=None, gflow_=None) == BADARG
    assert warp(x=None) == BADARG
    assert warp(mode=2) == UNSUPPORTED
    assert warp(nb=need - 1) == WORKSPACE and warp(ws_=None) == WORKSPACE
    assert lib.crfp_flow_warp_backward_workspace_bytes(0, 5, 9, 11) == 0 and lib.crfp_flow_warp_backward_workspace_bytes(70000, 5, 9, 11) == 0
    assert warp(x=None, gflow_=None) == 0      # x is not needed for grad_x alone
    torch.cuda.synchronize()
    assert bool((gflow == 3.0).all()) and not bool((gx == 3.0).any())

    S = {k: v.to(DEV).contiguous() for k, v in wc.shared_leaves("shared").items()}
    n, _, h, w = S["x"].shape
    need = lib.crfp_dcnv2_shared_backward_workspace_bytes(n, 4, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    outs = [torch.full_like(S[k], 3.0) for k in wc.SHARED_GRADS]

    def shared(cin=4, cout=4, outs_=outs, nb=need):
        return lib.crfp_dcnv2_shared_backward_f32(*(P(S[k]) for k in ("x", "offset", "mask", "weight", "grad_out")), *(P(o) for o in outs_),
                                                  n, cin, cout, h, w, P(ws), nb, s)

    assert shared(cin=8) == UNSUPPORTED and shared(cout=8) == UNSUPPORTED
    assert shared(outs_=[None] * 5) == BADARG
    assert shared(nb=need - 1) == WORKSPACE
    assert lib.crfp_dcnv2_shared_backward_workspace_bytes(n, 8, h, w) == 0 and lib.crfp_dcnv2_shared_backward_workspace_bytes(0, 4, h, w) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 3.0).all()) for o in outs)


# ---------------------------------------------------------------- dcnv2_shared
@pytest.mark.parametrize("name", list(wc.SHARED_CASES))
def test_shared_gradients_match_the_float64_oracle(name):
    """6: a grad_fn, and the three shared cases against their float64 leaf gradients"""
    L = wc.shared_leaves(name)
    args = [L[k].to(DEV) for k in wc.SHARED_GRADS]
    assert shared_fn(args[0], args[1].clone().requires_grad_(True), *args[2:]).grad_fn is not None
    grads, _ = wc.run_shared(shared_fn, name, torch.float32, DEV)
    check_shared(name, grads)


@pytest.mark.parametrize("name", list(wc.SHARED_CASES))
def test_shared_reproducible_and_equal_to_the_tiled_route(name):
    """7: grad_offset, grad_mask, grad_weight and grad_bias bitwise equal across two calls, and within TOL of ops.dcnv2 on the tiled tensors
    (relative to the float64 reference's maximum, like every other bound here)"""
    a, _ = wc.run_shared(shared_fn, name, torch.float32, DEV)
    b, _ = wc.run_shared(shared_fn, name, torch.float32, DEV)
    for k in SHARED_DETERMINISTIC:
        assert torch.equal(a[k], b[k]), k
    t, _ = wc.run_shared(tiled_fn, name, torch.float32, DEV)
    check_shared(name, t, what="tiled dcnv2")
    ref = wc.shared_reference(name)
    for k in wc.SHARED_GRADS:
        d = float((a[k] - t[k]).abs().max()) / float(ref[k].abs().max())
        assert d <= wc.SHARED_TOL[name][k], (k, d)


def test_shared_needs_input_grad_subsets():
    name = "shared_motion"
    full, _ = wc.run_shared(shared_fn, name, torch.float32, DEV)
    for needs in (("weight", "bias"), ("x",), ("offset", "mask")):
        part, _ = wc.run_shared(shared_fn, name, torch.float32, DEV, needs)
        for k in wc.SHARED_GRADS:
            if k not in needs:
                assert part[k] is None, k
            elif k in SHARED_DETERMINISTIC:
                assert torch.equal(part[k], full[k]), k
        check_shared(name, part, needs)


def test_shared_forward_is_unchanged():
    """8: the no-grad forward is bitwise the forward taken with grad mode on (and the one with nothing requiring grad)"""
    from crfp_amd import ops
    for name in wc.SHARED_CASES:
        L = wc.shared_leaves(name)
        args = [L[k].to(DEV) for k in wc.SHARED_GRADS]
        with torch.no_grad():
            plain = ops.dcnv2_shared(*args)
        req = [a.clone().requires_grad_(True) for a in args]
        with torch.no_grad():
            off = ops.dcnv2_shared(*req)
        none_req = ops.dcnv2_shared(*args)
        on = ops.dcnv2_shared(*req)
        assert off.grad_fn is None and none_req.grad_fn is None and on.grad_fn is not None
        assert torch.equal(off, plain) and torch.equal(none_req, plain) and torch.equal(on.detach(), plain)


# ---------------------------------------------------------------- the alignment graph
def test_alignment_graph_trains():
    """9: flow leaf -> ops.flow_warp(prev, flow) -> two conv heads on cat(cur, warped, flow) -> ops.dcnv2_shared(prev, offset + flow.flip,
    mask, w, b) -> squared error at 12 x 16, float32 on the device against the same graph in float64 on the CPU through the oracle: the
    gradients of the flow, prev, the head weights and the DCN weight / bias, and the loss after one SGD step on the heads."""
    loss_ref, _, _ = wc.graph_reference()
    loss, grads, loss2 = wc.graph_run(torch.float32, DEV, warp_fn, shared_fn)
    assert abs(loss - loss_ref) < 1e-5 * loss_ref and loss2 < loss
    errs = wc.graph_errors(loss2, grads)
    print("warp_backward graph: " + ", ".join(f"{k} {errs[k]:.2e} (tol {wc.GRAPH_TOL[k]:.2e})" for k in errs))
    for k, e in errs.items():
        assert e <= wc.GRAPH_TOL[k], (k, e, wc.GRAPH_TOL[k])
