"""GPU: CRFP_DSV trains through the HIP operators -- forward_train and every parameter's gradient against the float64 oracle
(oracle.crfp_oracle.crfp_dsv_forward under autograd), the frozen flow net, Adam steps through crfp_amd.trainrig, the stale-pack check and
the trainable policy.  Gradient pass test per parameter: max|gpu - ref64| <= TOL * max|ref64|, TOL = 8 * max(the float32 CPU graph's
own error, one ulp) from tests/helpers/train_backward_cases.py (no TOL above 0.1: this level looks for wiring mistakes -- a dropped
edge, a detached flow -- which are errors of order one; the per-operator tests are the tight ones).

Measured on an MI355X: case A forward error 2.9e-07, all 118 gradients inside their TOL (largest error 7.8e-03 where the float32 CPU graph
has 7.8e-03 too; worst against its TOL: dcn_3.dcn_mask.bias 1.2e-05 of 4.3e-05); case B all 118 inside, flow-net gradients at 7e-06.  With the
conv epilogue's hardware-exp tanh in the flow head (5e-06 px of flow error, nine times a float32 graph's) case B missed by up to 32x
(spynet.encoder1.0.weight 8.6e-04 against 2.7e-05): forward_train takes that one tanh from ATen."""
import pytest
import torch

from helpers import train_backward_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def build(name, state=None):
    from crfp_amd.model.CRFP import CRFP_DSV
    c = tc.MODEL[name]
    m = CRFP_DSV(torch.device(DEV), mid_channels=c["mid"], y_only=c["y_only"])
    sd = state if state is not None else {k: torch.from_numpy(v) for k, v in tc.model_leaves(name)[0].items()}
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def inputs(name):
    _, lrs, fvs, mks, hr = tc.model_leaves(name)
    return lrs.to(DEV), fvs.to(DEV), mks.to(DEV), hr.to(DEV)


def loss_of(out, hr):
    from crfp_amd.loss import charbonnier_loss
    return charbonnier_loss(out.reshape(-1, *out.shape[2:]), hr.reshape(-1, *hr.shape[2:]))


def grads_of(name, freeze_flow=False):
    m = build(name)
    if freeze_flow:
        for k, p in m.named_parameters():
            if "spynet" in k:
                p.requires_grad_(False)
    lrs, fvs, mks, hr = inputs(name)
    out = m.forward_train(lrs, fvs, mks)
    loss = loss_of(out, hr)
    loss.backward()
    return out.detach(), loss.detach(), {k: p.grad for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(tc.MODEL))
def test_gradients_match_the_float64_oracle(name):
    """forward_train within 2e-4 of the oracle, every parameter's gradient within its TOL of the oracle's float64 autograd"""
    out64, loss64, g64 = tc.model_reference(name)
    tol = tc.model_tol(name)
    out, loss, g = grads_of(name)
    assert out.grad_fn is None and tuple(out.shape) == tuple(out64.shape)
    efwd = float((out.double().cpu() - out64).abs().max())
    assert set(g) == set(g64)
    errs = {}
    for k in g64:
        assert g[k] is not None and bool(torch.isfinite(g[k]).all()) and float(g[k].abs().max()) > 0, k
        errs[k] = tc.rel_err(g[k], g64[k])
    worst = max(errs, key=lambda k: errs[k] / tol[k])
    print(f"train_model {name}: forward error {efwd:.2e}, loss {float(loss):.6f} (float64 {loss64:.6f}); worst gradient error relative to its TOL: "
          f"{worst} {errs[worst]:.2e} (tol {tol[worst]:.2e}); largest error {max(errs.values()):.2e}")
    assert efwd < tc.MODEL_FWD_BOUND
    assert abs(float(loss) - loss64) <= tc.MODEL_FWD_BOUND   # the mean of a 1-Lipschitz function of the output
    over = {k: (f"{errs[k]:.2e}", f"{tol[k]:.2e}") for k in g64 if errs[k] > tol[k]}
    print(f"train_model {name}: {len(over)} of {len(g64)} gradients over their TOL: {over}")
    assert not over, (name, over)


def test_frozen_flow_net_gets_no_gradient_and_changes_no_other():
    """the flow net frozen: its gradients are None, and every other gradient is the one of the run with it unfrozen.  Bit for bit where no
    float atomic sum lies between the loss and the parameter: conv_last, whose gradient is a sum over the frames of grad_out against the
    state.  The gradient of a warp's or a DCN's input is an unordered float atomic sum (ops.flow_warp, ops.dcnv2), the state of every
    frame but the last reaches the loss through one, and the frozen run makes the warps' calls without grad_flow; every other parameter
    is therefore held to its TOL of the cases module (the float32 graph's own noise; a graph that changed with the freeze is an error
    of order one).  Measured: two unfrozen runs already differ in the last bits of most of these tensors."""
    _, _, full = grads_of("B")
    _, _, frozen = grads_of("B", freeze_flow=True)
    tol = tc.model_tol("B")
    exact = 0
    for k in full:
        if "spynet" in k:
            assert frozen[k] is None and full[k] is not None
            continue
        assert frozen[k] is not None
        exact += bool(torch.equal(frozen[k], full[k]))
        if k.startswith("conv_last."):
            assert torch.equal(frozen[k], full[k]), k
        else:
            assert tc.rel_err(frozen[k], full[k]) <= tol[k], k
    print(f"train_model frozen flow: {exact} of {sum('spynet' not in k for k in full)} gradients equal bit for bit to the unfrozen run's")


def _rig_and_batch(name):
    from crfp_amd import option, trainrig
    m = build(name)
    args = option.parse([])
    args.y_only = tc.MODEL[name]["y_only"]
    args.lr_rate, args.lr_rate_flow = 2e-4, 5e-5
    rig = trainrig.TrainRig(args, m)
    c = tc.MODEL[name]
    batch = trainrig.synthetic_batch(7, c["n"], c["t"], c["h"], c["w"], torch.device(DEV), fv_size=c["fv_size"])
    return m, rig, batch


@pytest.mark.parametrize("name", ["B"])
def test_adam_steps_lower_the_loss_and_the_engine_repacks(name):
    """five Adam steps on one fixed batch through trainrig.train_step (y_only: with the colour recombination): every trainable parameter
    gets a finite gradient and the loss falls; afterwards, with trainable = False, the model equals bit for bit a freshly built model
    loaded with the same state_dict (the engine's packed weights were rebuilt)."""
    m, rig, batch = _rig_and_batch(name)
    with torch.no_grad():
        before_engine = m(batch["LR"], batch["Ref"], batch["Ref_sp"])     # packs the weights: the image forward_train must mark stale
    assert m._engine is not None and m._engine_sig is not None
    rig.cur_iter = 5000                                                    # the flow net released (trainer.py:227-229)
    losses = [float(rig.train_step(batch)) for _ in range(5)]
    assert m._engine_sig is None                                           # forward_train marked the packed image stale
    for k, p in m.named_parameters():
        assert p.requires_grad and p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    with torch.no_grad():
        final = float(rig.args.rec_w * rig.loss_all["cb_loss"](*_sr_hr(rig, m.forward_train, batch)))   # the route train_step measured
    print(f"train_model {name}: losses {losses}, after the steps {final:.6f}")
    assert final < losses[0]
    m.trainable = False
    got = m(batch["LR"], batch["Ref"], batch["Ref_sp"])
    fresh = build(name, state={k: v.detach().clone() for k, v in m.state_dict().items()})
    want = fresh(batch["LR"], batch["Ref"], batch["Ref_sp"])
    assert got.grad_fn is None and torch.equal(got, want)
    assert not torch.equal(got, before_engine)


def _sr_hr(rig, forward, batch):
    from crfp_amd import trainrig
    sr = forward(batch["LR"], batch["Ref"], batch["Ref_sp"])
    sr = sr.reshape(-1, *sr.shape[2:])
    hr = batch["HR"].reshape(-1, *batch["HR"].shape[2:])
    if rig.args.y_only:
        yuv = trainrig.rgb2yuv(batch["LR_sr"].reshape(-1, *batch["LR_sr"].shape[2:]))
        sr = trainrig.yuv2rgb(torch.cat((sr[:, 0:1], yuv[:, 1:3]), dim=1))
    return sr, hr


def test_flow_net_is_frozen_before_iteration_5000():
    m, rig, batch = _rig_and_batch("B")
    rig.train_step(batch)
    for k, p in m.named_parameters():
        assert (p.grad is None and not p.requires_grad) if "spynet" in k else (p.grad is not None), k
    rig.cur_iter = 5000
    rig.train_step(batch)
    assert all(p.requires_grad and p.grad is not None for p in m.parameters())


def test_trainable_policy():
    """trainable = False with grad mode on: no grad_fn and bit for bit what torch.no_grad() gives; trainable = True under torch.no_grad():
    the engine path; trainable = True with grad mode on: forward_train; the four other model classes raise NotImplementedError"""
    from crfp_amd.model import CRFP as M
    m = build("A")
    lrs, fvs, mks, _ = inputs("A")
    assert m.trainable is False and m.has_engine()
    on = m(lrs, fvs, mks)
    with torch.no_grad():
        off = m(lrs, fvs, mks)
    assert on.grad_fn is None and not on.requires_grad and torch.equal(on, off)
    m.trainable = True
    with torch.no_grad():
        eng = m(lrs, fvs, mks)
    assert eng.grad_fn is None and torch.equal(eng, off)
    out = m(lrs, fvs, mks)
    assert out.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(out.detach(), m.forward_train(lrs, fvs, mks))
    assert float((out.detach() - off).abs().max()) < tc.MODEL_FWD_BOUND   # the same function through two routes
    for cls in (M.CRFP_DSV_CRA, M.CRFP, M.CRFP_simple, M.MRCF_simple_v18):
        other = cls(torch.device(DEV), mid_channels=16).to(DEV)
        other.trainable = True
        with pytest.raises(NotImplementedError, match="CRFP_DSV"):
            other(lrs, fvs, mks)
        with pytest.raises(NotImplementedError, match="CRFP_DSV"):
            other.forward_train(lrs, fvs, mks)


def test_flow_carries_gradient_into_the_8x_warp():
    """the flow is not detached anywhere: with every parameter but the flow net's frozen, a two-frame clip still gives the flow net a
    gradient, and it is the one of the full run restricted to the flow net up to the atomic sums upstream"""
    m = build("B")
    for k, p in m.named_parameters():
        p.requires_grad_("spynet" in k)
    lrs, fvs, mks, hr = inputs("B")
    loss_of(m.forward_train(lrs, fvs, mks), hr).backward()
    g64 = tc.model_reference("B")[2]
    tol = tc.model_tol("B")
    for k, p in m.named_parameters():
        if "spynet" in k:
            assert p.grad is not None and tc.rel_err(p.grad, g64[k]) <= tol[k], k
        else:
            assert p.grad is None
