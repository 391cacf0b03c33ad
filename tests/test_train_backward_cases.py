"""CPU: pins the cases, references and bounds of tests/helpers/train_backward_cases.py, the gather rule of the resize backward (restated in
numpy, float32 operation for operation), crfp_amd.loss on CPU tensors against the reference's values (tests/golden/charbonnier.npz),
the rig's cosine schedule (tests/golden/cosine_lr.npz), and the trainable policy's refusals."""
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers import train_backward_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_case_tables():
    assert len(tc.RESIZE) == 13 and len(tc.EXACT) == 3 and set(tc.POOL) == {"4x6", "5x7", "2x3", "45x80"}
    for s in (2, 4, 8):
        for hw in ("1x5", "3x1", "5x7"):   # the one-pixel axes exercise the min(i0 + 1, in - 1) clamp
            assert f"s{s}_{hw}" in tc.RESIZE
    assert tc.RESIZE["s2_5x7"]["mul"] == 2.0 and tc.RESIZE["s8_5x7"]["mul"] == 8.0
    assert tc.out_size(tc.RESIZE["size_16x24_20x24"]) == (20, 24) and tc.out_size(tc.RESIZE["down_9x7_5x4"]) == (5, 4)
    assert tc.out_size(tc.RESIZE["identity_6x9"]) == (6, 9) and tc.out_size(tc.RESIZE["size_8x20_11x23"]) == (11, 23)
    assert tc.POOL["45x80"]["h"] // 2 == 22
    assert len(tc.CB_CASES) == 18 and tc.CB_SHAPES["1x3x5x7"] == (1, 3, 5, 7) and (1 * 3 * 5 * 7) % 64 != 0
    assert tc.MODEL["A"]["h"] == 20 and tc.MODEL["B"] == dict(mid=16, y_only=True, weights_seed=3, clip_seed=5, n=2, t=2, h=12, w=16, fv_size=64)


def test_tolerances_come_from_the_float32_cpu_graph():
    for name in tc.RESIZE_ALL:
        t = tc.resize_tol(name)
        assert 8 * tc.ULP <= t < 1e-4, (name, t)
        assert float(tc.resize_reference(name).abs().max()) > 0
    for name in tc.POOL:
        assert 8 * tc.ULP <= tc.pool_tol(name) < 1e-4
    for case in tc.CB_CASES:
        tl, tg = tc.cb_tol(case)
        assert 8 * tc.ULP <= tl < 1e-4 and 8 * tc.ULP <= tg < 1e-4, (case, tl, tg)
    print("resize E32:", {k: f"{tc.resize_e32(k):.1e}" for k in tc.RESIZE_ALL})
    print("pool E32:", {k: f"{tc.pool_e32(k):.1e}" for k in tc.POOL})
    print("charbonnier TOL:", {tc.cb_id(c): tuple(f"{v:.1e}" for v in tc.cb_tol(c)) for c in tc.CB_CASES})


@pytest.mark.parametrize("name", list(tc.EXACT))
def test_exact_cases_float32_aten_equals_float64(name):
    """the condition of the exact cases: dyadic weights, integer grad_out -- float32 autograd is already the float64 gradient"""
    g32 = tc._resize_grad(name, torch.float32)
    g64 = tc.resize_reference(name)
    assert torch.equal(g32.double(), g64)
    assert torch.equal(g64.float().double(), g64) and float(g64.abs().max()) > 0


# ---- the kernel's gather rule in numpy: float32 source index (resample_index.h), the candidate range and the keep rule of train_backward.hip
def _src_index(dst, scale, in_size):
    f = np.float32
    src = f(f(scale) * f(f(dst) + f(0.5))) - f(0.5)
    if src < 0:
        src = f(0)
    i0 = min(int(math.floor(src)), in_size - 1)
    i1 = min(i0 + 1, in_size - 1)
    l1 = f(min(max(f(src - f(i0)), f(0)), f(1)))
    return i0, i1, f(1) - l1, l1


def _candidates(i, scale, in_size, out_size):
    f = np.float32
    last = out_size - 1
    flo = math.floor(f(f(f(i) - f(0.5)) / f(scale)) - f(0.5)) - 1
    fhi = math.ceil(f(f(f(i) + f(1.5)) / f(scale)) - f(0.5)) + 1
    lo = 0 if i == 0 else int(min(max(flo, 0), last))
    hi = last if i == in_size - 1 else int(min(max(fhi, 0), last))
    return lo, hi


def _axis_matrix(in_size, out_size, scale, ranged, edge_both=True):
    """A[o, i] = the forward's weight of input i in output o; ranged: only inside the kernel's candidate range of i"""
    A = np.zeros((out_size, in_size))
    for i in range(in_size):
        lo, hi = _candidates(i, scale, in_size, out_size) if ranged else (0, out_size - 1)
        for o in range(lo, hi + 1):
            i0, i1, l0, l1 = _src_index(o, scale, in_size)
            if i0 == i or i1 == i:
                A[o, i] = (float(l0) if i0 == i else 0.0) + (float(l1) if i1 == i and (edge_both or i0 != i) else 0.0)
    return A


@pytest.mark.parametrize("name", list(tc.RESIZE_ALL))
def test_gather_rule_restated_in_numpy_matches_float64(name):
    """the candidate range loses no contributor (ranged == the walk over every output), and the gathered gradient is ATen's float64 one"""
    c = tc.RESIZE_ALL[name]
    oh, ow = tc.out_size(c)
    sh, sw = tc.src_scales(c)
    Ay, Ax = _axis_matrix(c["h"], oh, sh, True), _axis_matrix(c["w"], ow, sw, True)
    assert np.array_equal(Ay, _axis_matrix(c["h"], oh, sh, False)) and np.array_equal(Ax, _axis_matrix(c["w"], ow, sw, False))
    assert np.allclose(Ay.sum(1), 1.0, atol=1e-6) and np.allclose(Ax.sum(1), 1.0, atol=1e-6)   # every output's weights sum to one
    _, go = tc.resize_leaves(name)
    g = c["mul"] * np.einsum("oi,ncop,pj->ncij", Ay, go.double().numpy(), Ax)
    ref = tc.resize_reference(name).numpy()
    assert np.abs(g - ref).max() <= tc.resize_tol(name) * np.abs(ref).max()
    if c.get("exact"):
        assert np.array_equal(g, ref)
    if "scale" in c:   # dropping the second weight at a clamped edge (i0 == i1) is an error of order one on every upscaling case
        bad = c["mul"] * np.einsum("oi,ncop,pj->ncij", _axis_matrix(c["h"], oh, sh, True, False), go.double().numpy(),
                                   _axis_matrix(c["w"], ow, sw, True, False))
        assert np.abs(bad - ref).max() > 1e-2 * np.abs(ref).max()


@pytest.mark.parametrize("name", list(tc.POOL))
def test_pool_reference_is_a_quarter_inside_and_zero_on_the_dropped_edge(name):
    c = tc.POOL[name]
    _, go = tc.pool_leaves(name)
    ref = tc.pool_reference(name)
    oh, ow = c["h"] // 2, c["w"] // 2
    want = torch.zeros_like(ref)
    want[:, :, :2 * oh, :2 * ow] = 0.25 * go.double().repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert torch.equal(ref, want)


@pytest.mark.parametrize("name", list(tc.MODEL))
def test_model_cases_are_differentiable_end_to_end(name):
    """the oracle carries a gradient to every parameter, the flow net's included, and no tensor's TOL exceeds the cap"""
    _, loss, g64 = tc.model_reference(name)
    assert math.isfinite(loss) and loss > 0
    sd = tc.model_leaves(name)[0]
    assert set(g64) == set(sd)
    for k, g in g64.items():
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    assert max(float(g.abs().max()) for k, g in g64.items() if k.startswith("spynet.")) > 1e-3
    tol = tc.model_tol(name)
    worst = max(tol, key=tol.get)
    print(f"model {name}: loss {loss:.6f}, worst E32 {tc.model_e32(name)[worst]:.2e} on {worst}, worst TOL {tol[worst]:.2e}")
    assert tol[worst] <= tc.MODEL_TOL_CAP, (worst, tol[worst])


def test_loss_on_cpu_tensors_matches_the_reference():
    from crfp_amd import loss as L
    g = np.load(os.path.join(GOLDEN, "charbonnier.npz"))
    for case in tc.CB_CASES:
        shape, wkind, reduction, sample_wise = case
        pred, target, weight = tc.cb_leaves(shape, wkind)
        mod = L.CharbonnierLoss(loss_weight=tc.CB_LOSS_WEIGHT, reduction=reduction, sample_wise=sample_wise, eps=tc.CB_EPS)
        got = mod(pred, target, weight)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), g[tc.cb_id(case)]), tc.cb_id(case)
        # and the cases module's own restatement (the float64 reference of the GPU tests) is that formula
        assert float(tc.CB_LOSS_WEIGHT * tc.cb_formula(pred, target, weight, reduction, sample_wise)) == float(g[tc.cb_id(case)])
    for wkind in tc.CB_WEIGHTS:
        pred, target, weight = tc.cb_leaves("1x3x5x7", wkind)
        assert np.array_equal(L.charbonnier_loss(pred, target, weight, reduction="none").numpy(), g[f"1x3x5x7-{wkind}-none"])
    with pytest.raises(ValueError):
        L.CharbonnierLoss(reduction="median")
    args = type("A", (), {"rec_w": 1.0})()
    d = L.get_loss_dict(args, None)
    assert list(d) == ["cb_loss"] and isinstance(d["cb_loss"], L.CharbonnierLoss) and d["cb_loss"].loss_weight == 1.0
    args.rec_w = 0.0
    with pytest.raises(SystemExit):
        L.get_loss_dict(args, None)


def test_cosine_schedule_matches_the_reference():
    from crfp_amd import trainrig
    g = np.load(os.path.join(GOLDEN, "cosine_lr.npz"))
    for i, it in enumerate(g["iters"]):
        for j, b in enumerate(g["base"]):
            assert trainrig.cosine_lr(float(b), int(it)) == float(g["lr"][i, j]), (it, b)
    with pytest.raises(ValueError):
        trainrig.cosine_lr(1e-4, 600000)
    assert trainrig.PERIODS == (600000,) and trainrig.MIN_LR == 1e-7 and trainrig.FLOW_FREEZE_ITERS == 5000


def test_rig_groups_freeze_and_checkpoint_name():
    """two Adam groups split by 'spynet' in the name, the reference's file name pattern, the colour recombination of y_only"""
    from crfp_amd import option, trainrig
    from crfp_amd.model.CRFP import CRFP_DSV, CRFP_simple
    args = option.parse([])
    model = CRFP_DSV("cpu", mid_channels=16)
    rig = trainrig.TrainRig(args, model)
    assert model.trainable is True
    flow = [p for n, p in model.named_parameters() if "spynet" in n]
    rest = [p for n, p in model.named_parameters() if "spynet" not in n]
    g0, g1 = rig.optimizer.param_groups
    assert len(g0["params"]) == len(rest) and len(g1["params"]) == len(flow) == 28
    assert rig.base_lr == [1e-4, 2.5e-5] and g0["betas"] == (0.9, 0.999) and g0["eps"] == 1e-12
    rig.cur_iter = 300000
    rig.before_train_iter()
    assert [g["lr"] for g in rig.optimizer.param_groups] == [trainrig.cosine_lr(1e-4, 300000), trainrig.cosine_lr(2.5e-5, 300000)]
    rig.cur_iter = 12
    assert rig.checkpoint_name(3) == "save_dir/model/model_00003_000012.pt"
    rgb = torch.rand(2, 3, 4, 5)
    assert float((trainrig.yuv2rgb(trainrig.rgb2yuv(rgb)) - rgb).abs().max()) < 5e-3   # the reference's rounded matrices are near-inverse
    with pytest.raises(NotImplementedError):
        trainrig.TrainRig(args, CRFP_simple("cpu", mid_channels=16))


def test_trainable_policy_refusals():
    """trainable = True on the classes without a training path: forward and forward_train raise NotImplementedError naming CRFP_DSV, before
    any device work"""
    from crfp_amd.model import CRFP as M
    x = torch.zeros(1, 2, 3, 8, 8), torch.zeros(1, 2, 3, 64, 64), torch.zeros(1, 2, 1, 64, 64, dtype=torch.bool)
    assert M.CRFP_DSV("cpu").trainable is False
    for cls in (M.CRFP_DSV_CRA, M.CRFP, M.CRFP_simple, M.MRCF_simple_v18, M.MRCF_simple_v13, M.MRCF_simple_v15, M.MRCF_simple_v18_cra):
        m = cls("cpu", mid_channels=16)
        assert m.trainable is False
        m.trainable = True
        for fn in (m.forward, m.forward_train):
            for grad in (True, False):
                with torch.set_grad_enabled(grad), pytest.raises(NotImplementedError, match="CRFP_DSV"):
                    fn(*x)


def test_synth_exposes_the_hr_scene_without_changing_make_clip():
    from crfp_amd import synth
    a = synth.make_clip(5, 1, 3, 20, 24, fv_size=64)
    b = synth.make_clip_hr(5, 1, 3, 20, 24, fv_size=64)
    assert len(a) == 3 and len(b) == 4 and all(np.array_equal(u, v) for u, v in zip(a, b))
    assert b[3].shape == (1, 3, 3, 160, 192) and b[3].dtype == np.float32
    assert np.array_equal(b[1][b[2].repeat(3, 2)], b[3][b[2].repeat(3, 2)])   # the fovea window shows the HR frame


def test_entry_points_are_declared_and_bound():
    from crfp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "crfp_hip.h")).read()
    for name in ("crfp_upsample_bilinear_backward_f32", "crfp_avgpool2_backward_f32", "crfp_charbonnier_workspace_bytes", "crfp_charbonnier_f32",
                 "crfp_charbonnier_backward_f32"):
        assert name in _lib.SIGNATURES and re.search(r"\b" + name + r"\(", hdr), name
    mk = open(os.path.join(ROOT, "crfp_amd", "csrc", "Makefile")).read()
    assert "train_backward.hip" in mk and "resample_index.h" in mk
