"""GPU: the DCNv2 backward (crfp_dcnv2_backward_f32 through ops.dcnv2 under autograd) on the cases of tests/dcn_backward_cases.py against
their float64 oracle gradients; pass test per gradient tensor: max|gpu - ref64| <= TOL * max|ref64|, TOL = 8 * the oracle's own fp32 error."""
import pytest
import torch

import dcn_backward_cases as dc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DETERMINISTIC = ("offset", "mask", "weight", "bias")


def ops_fn(x, offset, mask, weight, bias, dg):
    from crfp_amd import ops
    return ops.dcnv2(x, offset, mask, weight, bias, 3, 1, 1, dg)


def gpu_run(name, needs=dc.GRADS):
    return dc.run(ops_fn, name, torch.float32, DEV, needs)


def check(name, grads, tensors=dc.GRADS, ref=None):
    ref = ref or dc.reference(name)
    errs = {k: dc.rel_err(grads[k], ref[k]) for k in tensors}
    print(f"dcn_backward {name}: " + ", ".join(f"{k} {errs[k]:.2e} (tol {dc.TOL[name][k]:.2e})" for k in tensors))
    for k in tensors:
        assert grads[k].shape == ref[k].shape and bool(torch.isfinite(grads[k]).all())
        assert errs[k] <= dc.TOL[name][k], (name, k, errs[k], dc.TOL[name][k])


@pytest.mark.parametrize("name", list(dc.CASES))
def test_gradients_match_the_float64_oracle(name):
    grads, out = gpu_run(name)
    assert float((out.double().cpu() - dc.reference_out(name)).abs().max()) < 1e-4   # the forward it differentiates
    check(name, grads)


def test_dropped_samples_get_exactly_zero():
    """Large motion, gradients at the full offset / mask tensors: a sample outside (-1, size) contributes exactly 0."""
    c = dc.CASES["motion"]
    n, dg, h, w = c["n"], c["dg"], c["h"], c["w"]
    grads, _ = gpu_run("motion")
    py, px = dc.sample_positions("motion")
    dropped = ~((py > -1) & (py < h) & (px > -1) & (px < w))
    assert int(dropped.sum()) > dropped.numel() // 2
    assert float(grads["mask"].cpu().reshape(n, dg, 9, h, w)[dropped].abs().max()) == 0.0
    assert float(grads["offset"].cpu().reshape(n, dg, 9, 2, h, w).permute(0, 1, 2, 4, 5, 3)[dropped].abs().max()) == 0.0


def test_c_abi_writes_inside_its_outputs_only():
    """Large motion through the C-ABI with ctypes: each of the five outputs is a view in the middle of a larger sentinel-filled tensor;
    the gradients are right and every sentinel is intact."""
    from crfp_amd import _lib
    name, SENT, PAD = "motion", -7777.25, 4099
    c = dc.CASES[name]
    L = {k: v.to(DEV) for k, v in dc.leaves(name).items()}
    n, cin, cout, dg, h, w = (c[k] for k in ("n", "cin", "cout", "dg", "h", "w"))
    lib = _lib.lib()
    bufs, views = {}, {}
    for k in dc.GRADS:
        numel = L[k].numel()
        bufs[k] = torch.full((numel + 2 * PAD,), SENT, dtype=torch.float32, device=DEV)
        views[k] = bufs[k][PAD:PAD + numel]
    nb = lib.crfp_dcnv2_backward_workspace_bytes(n, cin, cout, h, w, 3, dg)
    ws = torch.full((nb + 2 * PAD,), 0xA5, dtype=torch.uint8, device=DEV)   # a dirty workspace, with margins of its own
    wsv = ws[PAD + (-(ws.data_ptr() + PAD)) % 256:][:nb]
    rc = lib.crfp_dcnv2_backward_f32(L["x"].data_ptr(), L["offset"].data_ptr(), L["mask"].data_ptr(), L["weight"].data_ptr(),
                                     L["grad_out"].data_ptr(), *(views[k].data_ptr() for k in dc.GRADS), n, cin, cout, h, w, 3, 1, 1, dg,
                                     wsv.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "crfp_dcnv2_backward_f32")
    torch.cuda.synchronize()
    check(name, {k: views[k].reshape(L[k].shape) for k in dc.GRADS})
    for k in dc.GRADS:
        numel = L[k].numel()
        assert bool((bufs[k][:PAD] == SENT).all()) and bool((bufs[k][PAD + numel:] == SENT).all()), k
    lo = wsv.data_ptr() - ws.data_ptr()
    assert bool((ws[:lo] == 0xA5).all()) and bool((ws[lo + nb:] == 0xA5).all())


@pytest.mark.parametrize("needs", [("weight", "bias"), ("x",), ("offset", "mask")])
def test_needs_input_grad_subsets(needs):
    """Unrequested gradients are None; requested ones are those of the full call -- the deterministic four bit for bit."""
    name = "odd"
    full, _ = gpu_run(name)
    part, _ = gpu_run(name, needs)
    for k in dc.GRADS:
        if k not in needs:
            assert part[k] is None, k
        elif k in DETERMINISTIC:
            assert torch.equal(part[k], full[k]), k
    check(name, part, needs)


def test_deterministic_gradients_are_bitwise_reproducible():
    a, _ = gpu_run("g8")
    b, _ = gpu_run("g8")
    for k in DETERMINISTIC:
        assert torch.equal(a[k], b[k]), k
    check("g8", b)


def test_identity_kat_against_grid_sample():
    """Case 6 from the reference's side: grad_x = float64 autograd of 0.5 * grid_sample(align_corners=True, zeros); the flow gradient
    of that function is what arrives at the tiled offset, all of it through the centre taps (the others carry no weight: exactly 0)."""
    from crfp_amd import ops
    name = "identity"
    c = dc.CASES[name]
    gx, gflow = dc.identity_reference()
    grads, _ = gpu_run(name)
    check(name, grads, ("x", "offset"), {"x": gx, "offset": gflow})
    L = dc.leaves(name)
    off, msk = dc.expand(name, L["offset"], L["mask"])
    off = off.to(DEV).requires_grad_(True)
    out = ops.dcnv2(L["x"].to(DEV), off, msk.to(DEV), L["weight"].to(DEV), L["bias"].to(DEV), 3, 1, 1, c["dg"])
    out.backward(L["grad_out"].to(DEV))
    g = off.grad.reshape(c["n"], c["dg"], 9, 2, c["h"], c["w"])
    taps = [k for k in range(9) if k != 4]
    assert float(g[:, :, taps].abs().max()) == 0.0
    spread = g[:, :, 4].sum(1).flip(1)   # (dy, dx) summed over the groups -> (dx, dy)
    assert dc.rel_err(spread, gflow) <= dc.TOL[name]["offset"]


def test_module_trains():
    """Two nn.Conv2d heads (10 * tanh offsets, sigmoid mask) -> crfp_amd.dcn_v2.DCNv2(8, 8, 3, 1, 1, deformable_groups=2) at 12 x 16 ->
    squared error: backward() gives every parameter the float64 CPU gradient of the same graph on oracle.dcnv2; one SGD step lowers the loss."""
    import torch.nn as nn
    from crfp_amd.dcn_v2 import DCNv2
    P = dc.module_params()
    loss_ref, grads_ref, loss2_ref = dc.module_reference()
    feat, x, target = dc.module_data(torch.float32, DEV)
    off_head, mask_head = nn.Conv2d(8, 36, 3, 1, 1), nn.Conv2d(8, 18, 3, 1, 1)
    dcn = DCNv2(8, 8, 3, 1, 1, deformable_groups=2)
    mods = dict(off_w=off_head.weight, off_b=off_head.bias, mask_w=mask_head.weight, mask_b=mask_head.bias, dcn_w=dcn.weight, dcn_b=dcn.bias)
    with torch.no_grad():
        for k, p in mods.items():
            p.copy_(P[k].detach().float())
    for m in (off_head, mask_head, dcn):
        m.to(DEV)

    def loss_fn():
        offset = 10.0 * torch.tanh(off_head(feat))
        mask = torch.sigmoid(mask_head(feat))
        return ((dcn(x, offset, mask) - target) ** 2).mean()

    params = [p for m in (off_head, mask_head, dcn) for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=dc.MODULE_LR)
    loss = loss_fn()
    assert loss.grad_fn is not None and abs(float(loss.detach()) - loss_ref) < 1e-4 * loss_ref
    opt.zero_grad()
    loss.backward()
    named = dict(off_w=off_head.weight, off_b=off_head.bias, mask_w=mask_head.weight, mask_b=mask_head.bias, dcn_w=dcn.weight, dcn_b=dcn.bias)
    errs = {k: dc.rel_err(p.grad, grads_ref[k]) for k, p in named.items()}
    print("dcn_backward module: " + ", ".join(f"{k} {errs[k]:.2e} (tol {dc.MODULE_TOL[k]:.2e})" for k in named))
    for k, p in named.items():
        assert p.grad is not None and errs[k] <= dc.MODULE_TOL[k], (k, errs[k], dc.MODULE_TOL[k])
    opt.step()
    with torch.no_grad():
        loss2 = float(loss_fn())
    assert loss2 < float(loss.detach()) and abs(loss2 - loss2_ref) < 1e-3 * loss2_ref


def test_no_grad_paths_are_the_plain_forward():
    """Grad mode off, or no input requiring grad: no grad_fn, and bit for bit the forward called inside no_grad (both DCN forward paths)."""
    from crfp_amd import ops
    for name in ("odd", "g8"):
        L = {k: v.to(DEV) for k, v in dc.leaves(name).items()}
        dg = dc.CASES[name]["dg"]
        args = [L[k] for k in dc.GRADS]
        with torch.no_grad():
            plain = ops.dcnv2(*args, 3, 1, 1, dg)
        req = [a.clone().requires_grad_(True) for a in args]
        with torch.no_grad():
            off = ops.dcnv2(*req, 3, 1, 1, dg)
        none_req = ops.dcnv2(*args, 3, 1, 1, dg)                    # grad mode on, nothing to differentiate
        on = ops.dcnv2(*req, 3, 1, 1, dg)
        assert off.grad_fn is None and none_req.grad_fn is None and not off.requires_grad and not none_req.requires_grad
        assert on.grad_fn is not None
        assert torch.equal(off, plain) and torch.equal(none_req, plain) and torch.equal(on.detach(), plain)
