"""GPU: the fused Charbonnier loss (crfp_charbonnier_f32 / crfp_charbonnier_backward_f32 through ops.charbonnier and crfp_amd.loss) on the
cases of tests/helpers/train_backward_cases.py: the loss value and grad_pred against float64, pass test max|gpu - ref64| <= TOL * max|ref64|
with TOL = 8 * max(the float32 CPU graph's own error, one ulp)."""
import math

import pytest
import torch

from helpers import train_backward_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run(case, pred=None, target=None, weight="case"):
    """CharbonnierLoss(loss_weight) on the case's device leaves -> (loss, grad_pred)"""
    from crfp_amd.loss import CharbonnierLoss
    shape, wkind, reduction, sample_wise = case
    p0, t0, w0 = tc.cb_leaves(shape, wkind)
    pred = (p0 if pred is None else pred).clone().to(DEV).requires_grad_(True)
    target = (t0 if target is None else target).to(DEV)
    weight = w0 if isinstance(weight, str) else weight
    weight = None if weight is None else weight.to(DEV)
    loss = CharbonnierLoss(loss_weight=tc.CB_LOSS_WEIGHT, reduction=reduction, sample_wise=sample_wise, eps=tc.CB_EPS)(pred, target, weight)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
    loss.backward()
    return loss.detach(), pred.grad


@pytest.mark.parametrize("case", tc.CB_CASES, ids=tc.cb_id)
def test_loss_and_gradient_match_float64(case):
    l64, g64 = tc.cb_reference(case)
    tol_l, tol_g = tc.cb_tol(case)
    loss, grad = run(case)
    el, eg = abs(float(loss) - float(l64)) / abs(float(l64)), tc.rel_err(grad, g64)
    print(f"charbonnier {tc.cb_id(case)}: loss {float(loss):.8f} (float64 {float(l64):.8f}) err {el:.2e} (tol {tol_l:.2e}), grad {eg:.2e} (tol {tol_g:.2e})")
    assert bool(torch.isfinite(grad).all()) and grad.shape == g64.shape
    assert el <= tol_l and eg <= tol_g


def test_sums_are_the_per_sample_float64_sums():
    """ops.charbonnier: sums[n, 2] float64 on the device = (sum sqrt(d^2 + eps) * w, sum w) per sample; without a weight the element count"""
    from crfp_amd import ops
    for shape in tc.CB_SHAPES:
        for wkind in tc.CB_WEIGHTS:
            pred, target, weight = tc.cb_leaves(shape, wkind)
            sums = ops.charbonnier(pred.to(DEV), target.to(DEV), None if weight is None else weight.to(DEV), tc.CB_EPS)
            assert sums.dtype == torch.float64 and sums.is_cuda and tuple(sums.shape) == (pred.shape[0], 2) and sums.grad_fn is None
            el = torch.sqrt((pred.double() - target.double()) ** 2 + tc.CB_EPS)
            wexp = torch.ones_like(el) if weight is None else weight.double().expand_as(el)
            ref = torch.stack([(el * wexp).sum(dim=[1, 2, 3]), wexp.sum(dim=[1, 2, 3])], 1)
            assert tc.rel_err(sums[:, 0], ref[:, 0]) <= 8 * tc.ULP
            assert tc.rel_err(sums[:, 1], ref[:, 1]) <= 8 * tc.ULP
            if wkind != "nchw":   # counts: exact in float64
                assert torch.equal(sums[:, 1].cpu(), ref[:, 1])
            if weight is None:
                assert float(sums[0, 1]) == pred[0].numel()


def test_target_gradient_is_the_negation():
    from crfp_amd import ops
    pred, target, weight = tc.cb_leaves("3x3x16x24", "nchw")
    p, t = pred.clone().to(DEV).requires_grad_(True), target.clone().to(DEV).requires_grad_(True)
    ops.charbonnier(p, t, weight.to(DEV))[:, 0].sum().backward()
    assert float(p.grad.abs().max()) > 0 and torch.equal(t.grad, -p.grad)
    t2 = target.clone().to(DEV).requires_grad_(True)
    ops.charbonnier(pred.to(DEV), t2, weight.to(DEV))[:, 0].sum().backward()
    assert torch.equal(t2.grad, t.grad)


@pytest.mark.parametrize("shape", list(tc.CB_SHAPES))
def test_pred_equal_target_gives_sqrt_eps_and_a_zero_gradient(shape):
    pred = tc.cb_leaves(shape, "none")[0]
    for wkind in tc.CB_WEIGHTS:
        case = (shape, wkind, "mean", False)
        loss, grad = run(case, pred=pred, target=pred)
        want = tc.CB_LOSS_WEIGHT * math.sqrt(tc.CB_EPS)
        assert abs(float(loss) - want) <= 8 * tc.ULP * want, (wkind, float(loss), want)
        assert bool((grad == 0).all())


@pytest.mark.parametrize("shape", list(tc.CB_SHAPES))
def test_all_zero_weight_gives_zero_loss_and_a_finite_zero_gradient(shape):
    n, c, h, w = tc.CB_SHAPES[shape]
    for wshape in ((n, 1, h, w), (n, c, h, w)):
        for reduction, sample_wise in tc.CB_REDUCTIONS:
            loss, grad = run((shape, "none", reduction, sample_wise), weight=torch.zeros(wshape))
            assert float(loss) == 0.0 and bool(torch.isfinite(grad).all()) and bool((grad == 0).all())


def test_two_runs_give_the_same_bits():
    for case in (("3x3x16x24", "nchw", "mean", True), ("1x3x5x7", "n1hw", "mean", False), ("3x3x16x24", "none", "sum", False)):
        (l1, g1), (l2, g2) = run(case), run(case)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)
    # more than one workgroup per sample: 2 x 3 x 96 x 128 elements -> 36 partials per sample, added in a fixed order
    from crfp_amd import ops
    g = torch.Generator().manual_seed(3)
    p, t = torch.rand(2, 3, 96, 128, generator=g).to(DEV), torch.rand(2, 3, 96, 128, generator=g).to(DEV)
    s1, s2 = ops.charbonnier(p, t), ops.charbonnier(p, t)
    assert torch.equal(s1, s2)
    ref = torch.sqrt((p.double() - t.double()) ** 2 + 1e-12).sum(dim=[1, 2, 3])
    assert tc.rel_err(s1[:, 0], ref) <= 8 * tc.ULP


def test_reduction_none_and_no_grad_paths():
    """reduction='none' is the torch formula on the device; grad mode off or nothing requiring grad: no grad_fn, the same bits"""
    from crfp_amd import ops
    from crfp_amd.loss import charbonnier_loss
    pred, target, weight = (t.to(DEV) for t in tc.cb_leaves("1x3x5x7", "nchw"))
    el = charbonnier_loss(pred, target, weight, reduction="none")
    assert tuple(el.shape) == tuple(pred.shape) and torch.equal(el, torch.sqrt((pred - target) ** 2 + 1e-12) * weight)
    req = pred.clone().requires_grad_(True)
    with torch.no_grad():
        off = ops.charbonnier(req, target, weight)
    plain, on = ops.charbonnier(pred, target, weight), ops.charbonnier(req, target, weight)
    assert off.grad_fn is None and plain.grad_fn is None and on.grad_fn is not None
    assert torch.equal(off, plain) and torch.equal(on.detach(), plain)


def test_refusal_codes():
    """every argument error comes back as its negative code (before any HIP call: the pointers below are never dereferenced)"""
    from crfp_amd import _lib
    lib = _lib.lib()
    t = torch.zeros(256, device=DEV)
    p, s = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
    fwd, bwd, nbytes = lib.crfp_charbonnier_f32, lib.crfp_charbonnier_backward_f32, lib.crfp_charbonnier_workspace_bytes
    nb = nbytes(1, 3, 4, 4)
    assert nb >= 16 and nbytes(0, 3, 4, 4) == 0 and nbytes(65536, 1, 1, 1) == 0 and nbytes(1, 1, 0, 4) == 0
    ok = (1, 3, 4, 4)
    for args in ((None, p, None, 0, p), (p, None, None, 0, p), (p, p, None, 0, None)):
        assert fwd(*args, *ok, 1e-12, p, nb, s) == BADARG
    for bad in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0)):
        assert fwd(p, p, None, 0, p, *bad, 1e-12, p, nb, s) == BADARG and bwd(p, p, None, 0, p, p, *bad, 1e-12, s) == BADARG, bad
    for wptr, wc in ((None, 1), (p, 0), (p, 2), (None, 3)):
        assert fwd(p, p, wptr, wc, p, *ok, 1e-12, p, nb, s) == BADARG and bwd(p, p, wptr, wc, p, p, *ok, 1e-12, s) == BADARG, wc
    for eps in (-1.0, float("nan"), float("inf")):
        assert fwd(p, p, None, 0, p, *ok, eps, p, nb, s) == BADARG and bwd(p, p, None, 0, p, p, *ok, eps, s) == BADARG
    assert fwd(p, p, None, 0, p, 65536, 1, 1, 1, 1e-12, p, 1 << 30, s) == UNSUPPORTED and bwd(p, p, None, 0, p, p, 65536, 1, 1, 1, 1e-12, s) == UNSUPPORTED
    assert fwd(p, p, None, 0, p, *ok, 1e-12, None, nb, s) == WORKSPACE and fwd(p, p, None, 0, p, *ok, 1e-12, p, nb - 1, s) == WORKSPACE
    for args in ((None, p, None, 0, p, p), (p, None, None, 0, p, p), (p, p, None, 0, None, p), (p, p, None, 0, p, None)):
        assert bwd(*args, *ok, 1e-12, s) == BADARG
    assert b"charbonnier" in lib.crfp_last_error_string()
    torch.cuda.synchronize()
    assert bool((t == 0).all())
