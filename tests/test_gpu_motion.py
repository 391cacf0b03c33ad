"""GPU (-m gpu): the gather kernels and the engines under large, steered motion (tests/helpers/motion_cases.py).

Every other full-path test runs with |flow| < 2 LR pixels, while FNet ends in tanh * 256.  Here the flow network is steered to +-24, +-60 and
saturating (> 200) LR pixels with both signs on both axes, i.e. up to +-2000 pixels at 8x resolution, and every test asserts the regime
conditions on the flow it really used (the engine's own flow).

Engine level.  The engine's flow is injected into the reference: ``orc.dsv_frame`` frame by frame with the flow the engine's FNet kernels gave
(``m.compute_flow`` == the clip's own ``flow_lr``, bit for bit).  The comparison then measures the warps, the DCNs and everything behind them,
not how far two fp32 evaluations of tanh(g z) * 256 drift apart.  Bounds are the ones the suite already holds these comparisons to at small
motion: 1e-4 against the fp32 oracle (test_odd_geometries_vs_oracle), the twin statistics of test_gpu_bf16 for bf16 storage, 2e-4 max(1, |ref|)
against the per-operator composition for the other wirings (test_gpu_ablation_engines), bit equality across schedules.  The fp32 oracle itself
is held within 1e-5 of its float64 run on the same inputs, so the reference sits well inside the bound it is used for.

Operator level.  ``ops.flow_warp`` / ``ops.dcnv2`` / ``ops.dcnv2_shared`` against float64 references that sample at index + displacement
directly, with displacements U(-R, R), R in {9, 64, 2058} (2058 = 8 * 256 + 10 is the largest the model can emit at 8x resolution) and planted
samples exactly on and 2^-10 beside every range check (-1, 0, size - 1, size).  Bound = the existing operator bound (2e-5 warp, 3e-5 DCN:
test_flow_warp_random, test_dcnv2) + the fp32 coordinate-rounding term, computed from the inputs (motion_cases.coord_rounding_term): the
kernel adds index + displacement in fp32 (half an ulp of the coordinate away from the exact sum the reference uses), a bilinear interpolant
moves by at most the largest adjacent-pixel difference per unit of coordinate (the zero frame counts as pixels in zeros mode), and only
samples inside (-1, size) see the image, so term = 1/2 ulp32(max in-frame |coord|) * max |adjacent difference|; for DCN times the largest
sum over taps and input channels of |weight * mask| that one output sees.  NaN, inf and |displacement| > 2^12 are out of scope.

Large-motion performance is not measured here or anywhere else."""
import functools

import numpy as np
import pytest
import torch

import dcn_paper_ref
from helpers import motion_cases as mc

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GEOMS = [(24, 40), (33, 47)]
CLIPS = [(r, h, w) for r in mc.REGIMES for (h, w) in GEOMS] + [("large", 17, 65)]
SHAPES = [(9, 11), (23, 45), (64, 96)]
RANGES = [9.0, 64.0, 2058.0]
FLOW_TOL = 0.05       # pixels: engine flow vs oracle flow, the sanity bound of test_gpu_bf16 for this tensor


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def orc():
    from oracle import crfp_oracle
    return crfp_oracle


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def _case(regime, h, w, y_only=False):
    return mc.steered_case(regime, 3, h, w, y_only=y_only)


def _model(sd_np, cls="CRFP_DSV", y_only=False, storage="f32"):
    from crfp_amd.model import CRFP
    m = getattr(CRFP, cls)(device=dev(), mid_channels=32, y_only=y_only, hr_dcn=True, offset_prop=True)
    m.load_state_dict({k: T(v.copy()) for k, v in sd_np.items()}, strict=True)
    m.storage = storage
    return m.to(dev()).eval()


def _like_model(cls, seed=3, y_only=False, storage="f32"):
    """One of the other wirings with ``make_state_dict_like`` weights and the steered flow network."""
    from crfp_amd import synth
    from crfp_amd.model import CRFP
    m = getattr(CRFP, cls)(dev(), mid_channels=32, y_only=y_only)
    sd = mc.steer_fnet(synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m.storage = storage
    return m.to(dev()).eval()


def _gpu(*arrays):
    return tuple(T(a).to(dev()) for a in arrays)


def _oracle_loop(orc, P, lrs, fvs, mks, flows, cfg, dtype=torch.float32):
    """crfp_dsv_forward with the flow handed in: new_state, then dsv_frame per frame (flows[:, i - 1] belongs to frame i)."""
    L, Fv, M = T(lrs).to(dtype), T(fvs).to(dtype), T(mks)
    n, t, _, h, w = L.shape
    st = orc.new_state(cfg, n, h, w, L)
    outs = []
    for i in range(t):
        out, st = orc.dsv_frame(P, cfg, st, L[:, i], Fv[:, i], M[:, i], flows[:, i - 1].to(dtype) if i > 0 else None)
        outs.append(out)
    return torch.stack(outs, dim=1)


def _engine_flow(orc, m, P, lrs, regime, what):
    """The flow the engine's own FNet kernels give for the clip (cpu tensor), checked for the regime and against the oracle's flow."""
    n, t, _, h, w = lrs.shape
    flows = m.compute_flow(T(lrs).to(dev()))[0].cpu()
    ref = orc.compute_flow(P, T(lrs))
    s = mc.flow_stats(flows, h, w)
    d = float((flows - ref).abs().max())
    print(f"{what}: engine flow {mc.fmt_stats(s)}; max|engine flow - oracle flow| = {d:.2e} px")
    mc.assert_regime(s, regime)
    assert d < FLOW_TOL, d
    return flows


# ----------------------------------------------------------------------------- CRFP_DSV against the oracle with the injected flow
@pytest.mark.parametrize("y_only", [False, True])
@pytest.mark.parametrize("regime,h,w", CLIPS)
def test_dsv_f32_vs_oracle_with_injected_flow(orc, regime, h, w, y_only):
    sd, lrs, fvs, mks = _case(regime, h, w, y_only)
    what = f"{regime} 3x{h}x{w}{' y_only' if y_only else ''}"
    P, cfg = orc.load_numpy_state(sd), orc.DSVConfig(y_only=y_only)
    m = _model(sd, y_only=y_only)
    flows = _engine_flow(orc, m, P, lrs, regime, what)
    out = m(*_gpu(lrs, fvs, mks)).cpu()
    eng = m.engine()
    assert not eng.overflowed()
    assert torch.equal(eng.debug_fetch("flow_lr", 3, h, w)[:, :2].cpu(), flows[0]), "compute_flow is not the clip's own flow"
    ref = _oracle_loop(orc, P, lrs, fvs, mks, flows, cfg)
    ref64 = _oracle_loop(orc, {k: v.double() for k, v in P.items()}, lrs, fvs, mks, flows, cfg, torch.float64)
    d_ref = float((ref.double() - ref64).abs().max())
    d = float((out - ref).abs().max())
    d64 = float((out.double() - ref64).abs().max())
    still = _oracle_loop(orc, P, lrs[:, :2], fvs[:, :2], mks[:, :2], flows[:, :1] * 0, cfg)
    moved = float((ref[:, 1] - still[:, 1]).abs().max())
    print(f"{what}: max|HIP - oracle(engine flow)| = {d:.3e} (bound 1e-4), vs the float64 oracle {d64:.3e}; oracle fp32 vs fp64 = {d_ref:.3e} "
          f"(bound 1e-5); frame 1 with this flow vs with zero flow: {moved:.2f}")
    assert d_ref < 1e-5
    assert moved > 1e-2, "the motion does not reach the output"
    assert torch.isfinite(out).all() and d < 1e-4


@pytest.mark.parametrize("regime,h,w", CLIPS)
def test_dsv_bf16_vs_twin_with_injected_flow(orc, regime, h, w):
    from test_gpu_bf16 import _check_frame_stats
    sd, lrs, fvs, mks = _case(regime, h, w)
    what = f"bf16 {regime} 3x{h}x{w}"
    P, cfg = orc.load_numpy_state(sd), orc.DSVConfig()
    Pb = orc.bf16_weights(P)
    m = _model(sd, storage="bf16")
    with orc.bf16_storage():
        flows = _engine_flow(orc, m, Pb, lrs, regime, what)
    out = m(*_gpu(lrs, fvs, mks)).cpu()
    eng = m.engine()
    assert not eng.overflowed()
    assert torch.equal(eng.debug_fetch("flow_lr", 3, h, w)[:, :2].cpu(), flows[0]), "compute_flow is not the clip's own flow"
    with orc.bf16_storage():
        twin = _oracle_loop(orc, Pb, lrs, fvs, mks, flows, cfg)
    ref32 = _oracle_loop(orc, P, lrs, fvs, mks, flows, cfg)
    _check_frame_stats(out, twin, ref32, what)


# ----------------------------------------------------------------------------- the other one-call wirings against their composition
@pytest.mark.parametrize("cls", ["CRFP_DSV_CRA", "CRFP_simple", "CRFP"])
@pytest.mark.parametrize("regime,h,w", CLIPS)
def test_other_wirings_vs_composition(cls, regime, h, w):
    _, lrs, fvs, mks = _case(regime, h, w)
    m = _like_model(cls)
    L, Fv, M = _gpu(lrs, fvs, mks)
    s = mc.flow_stats(m.compute_flow(L)[0], h, w)
    mc.assert_regime(s, regime)
    out = m(L, Fv, M)
    comp = m.forward_composed(L, Fv, M)
    assert m.has_engine() and not m.engine().overflowed()
    d, scale = float((out - comp).abs().max()), max(1.0, float(comp.abs().max()))
    print(f"{cls} {regime} 3x{h}x{w}: flow {mc.fmt_stats(s)}; max|engine - composed| = {d:.3e} (bound {2e-4 * scale:.1e})")
    assert torch.isfinite(out).all() and d < 2e-4 * scale
    assert float((out[:, 1:] - comp[:, :1]).abs().max()) > 1e-3      # the recurrence is live


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("stream_cls,clip_cls", [("MRCF_simple_v13", "CRFP_simple"), ("MRCF_simple_v15", "CRFP"), ("MRCF_simple_v18", "CRFP_DSV")])
@pytest.mark.parametrize("regime,h,w", [("large", 33, 47), ("saturating", 24, 40), ("moderate", 24, 40), ("large", 17, 65)])
def test_streams_equal_the_clip_engine(stream_cls, clip_cls, storage, regime, h, w):
    """v13 / v15 / v18: the clip streamed one frame per call gives the clip engine's bits."""
    sd, lrs, fvs, mks = _case(regime, h, w)
    if clip_cls == "CRFP_DSV":
        s, c = _model(sd, stream_cls, storage=storage), _model(sd, clip_cls, storage=storage)
    else:
        s, c = _like_model(stream_cls, storage=storage), _like_model(clip_cls, storage=storage)
    L, Fv, M = _gpu(lrs, fvs, mks)
    mc.assert_regime(mc.flow_stats(c.compute_flow(L)[0], h, w), regime)
    clip = c(L, Fv, M)
    s.clear_states()
    got = torch.cat([s(L[:, i:i + 1].contiguous(), Fv[:, i:i + 1].contiguous(), M[:, i:i + 1].contiguous()).clone() for i in range(3)], dim=1)
    assert torch.isfinite(clip).all() and torch.equal(got, clip)


# ----------------------------------------------------------------------------- schedule invariance, bit for bit
MOTION_ENV = {"CRFP_CHECK_GEOM": "33,47,3", "CRFP_CHECK_MOTION": "60"}
BIG_ENV = {"CRFP_CHECK_GEOM": "101,170,3", "CRFP_CHECK_MOTION": "120"}
_digests = {}


def _digest(env, lab=False):
    from test_gpu_parity import _golden_check
    key = (tuple(sorted(env.items())), lab)
    if key not in _digests:
        _digests[key] = _golden_check(env, lab=lab, want="DIGEST")
    return _digests[key]


def _storage_env(storage):
    return {"CRFP_CHECK_STORAGE": "bf16"} if storage == "bf16" else {}


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("env,lab", [({"CRFP_DCN_FUSED": "0"}, False), ({"CRFP_MASK_GATE": "0"}, False), ({"CRFP_SIDE_STREAM": "0"}, False),
                                     ({"CRFP_CONV_PAIR": "0"}, False), ({}, True), ({"CRFP_NARROW_SEQ": "0", "CRFP_NARROW_CHAIN": "0"}, True),
                                     ({"CRFP_STATE_FROM_EPILOGUE": "0"}, True)])
def test_schedules_are_bit_identical_under_large_motion(env, lab, storage):
    """3 x 33 x 47 with M = 60: the two-kernel DCN path, dense fovea-side launches, one stream, unpaired convs, the lab library and its
    round-6 switches all give the product default's bits (the regime of this clip: test_motion_cases.py and the engine tests above)."""
    base = dict(MOTION_ENV, **_storage_env(storage))
    want = _digest(base)
    got = _digest(dict(base, **env), lab=lab)
    assert want.startswith("DIGEST ") and len(want) == 7 + 64
    assert got == want, (env, lab, storage)


def test_persistent_and_banded_dcn_under_large_motion(orc):
    """3 x 101 x 170 with M = 120 (202 x 340 at 2x: the XCD-banded, persistent dcn_fused_kernel): product == two-kernel path == the lab library's
    non-persistent form."""
    from crfp_amd import synth
    sd = mc.steer_fnet(synth.make_state_dict(7))
    lrs = mc.steered_frames(mc.CLIP_SEED, 3, 101, 170, 120.0)[0]
    s = mc.flow_stats(orc.compute_flow(orc.load_numpy_state(sd), T(lrs)), 101, 170)
    print(f"3x101x170, M = 120: oracle flow {mc.fmt_stats(s)}")
    mc.assert_regime(s, "large")
    assert s["over16"] >= 0.5
    want = _digest(BIG_ENV)
    assert _digest(dict(BIG_ENV, CRFP_DCN_FUSED="0")) == want
    assert _digest(dict(BIG_ENV, CRFP_DF_PS_MIN_TILES="257"), lab=True) == want


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_lockstep_batch_and_used_workspace(storage):
    """n = 2 (the large and the moderate clip in one lock-step call) == two one-clip calls, and an engine whose workspace the moderate clip has
    used gives the same bits on the large clip as a freshly built engine."""
    h, w = 33, 47
    sd, big = _case("large", h, w)[0], _case("large", h, w)[1:]
    small = _case("moderate", h, w)[1:]
    fresh = _model(sd, storage=storage)(*_gpu(*big)).clone()
    m = _model(sd, storage=storage)
    first = m(*_gpu(*small)).clone()
    again = m(*_gpu(*big)).clone()
    assert torch.isfinite(fresh).all() and torch.equal(again, fresh), "a used workspace changes the result"
    both = m(*_gpu(*(np.concatenate([a, b], 0) for a, b in zip(big, small))))
    assert not m.engine().overflowed()
    assert torch.equal(both[:1], fresh) and torch.equal(both[1:], first), "lock-step batch differs from the one-clip calls"
    assert float((fresh - first).abs().max()) > 1e-2


# ----------------------------------------------------------------------------- operators against float64
def _report(what, got, ref, base, term, share, R):
    d = float(np.abs(got.detach().cpu().double().numpy() - ref).max())
    print(f"{what}: max|HIP - float64| = {d:.3e}, bound {base:.0e} + {term:.2e} (coordinate rounding); {share:.2f} of the samples in the frame")
    if R <= 64:
        assert share >= 0.2, share
    assert np.isfinite(d) and d < base + term, (d, base + term)


@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("c", [4, 24, 32])
@pytest.mark.parametrize("mode", ["zeros", "border"])
def test_flow_warp_vs_float64(mode, c, h, w, R):
    from crfp_amd import ops
    rs = np.random.RandomState(c * 1000 + h)
    x = rs.standard_normal((2, c, h, w)).astype(np.float32)
    flow = mc.planted_flow(int(R) + h, 2, h, w, R)
    ref = mc.warp_ref64(x, flow, mode)
    px = np.arange(w) + flow[..., 0].astype(np.float64)
    py = np.arange(h).reshape(h, 1) + flow[..., 1].astype(np.float64)
    term, share = mc.coord_rounding_term(x, px, py, zero_pad=(mode == "zeros"))
    got = ops.flow_warp(T(x).to(dev()), T(flow).to(dev()), padding_mode=mode)
    _report(f"flow_warp {mode} c={c} {h}x{w} R={R:g}", got, ref, 2e-5, term, share, R)
    assert np.abs(ref).max() > 0.5


def _dcn_inputs(seed, C, O, groups, h, w, R):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((1, C, h, w)).astype(np.float32)
    off = mc.planted_offsets(seed + 1, 1, groups, h, w, R)
    msk = rs.uniform(0, 1, (1, groups, h, w)).astype(np.float32)
    wt = (rs.standard_normal((O, C, 3, 3)) * 0.2).astype(np.float32)
    b = rs.standard_normal(O).astype(np.float32)
    return x, off, msk, wt, b


def _dcn_check(what, got, x, off, msk, wt, b, dg, R):
    """off / msk in ``ops.dcnv2`` layout [1, 2 * dg * 9, h, w] / [1, dg * 9, h, w]."""
    h, w = x.shape[-2:]
    C, O = x.shape[1], wt.shape[0]
    # tests/dcn_paper_ref.py (the paper's equations, dense hat matrices) where it is affordable; on 64 x 96 its corner-sampling restatement,
    # which test_motion_cases.py holds to the paper form within 1e-12
    fn = dcn_paper_ref.dcnv2_paper if h * w <= 23 * 45 else mc.dcn_ref64
    ref = fn(x, off, msk, wt, b, dg)
    k = np.arange(dg * 9) % 9
    py = np.arange(h).reshape(1, h, 1) + (k // 3 - 1).reshape(-1, 1, 1) + off[0, 0::2].astype(np.float64)
    px = np.arange(w).reshape(1, 1, w) + (k % 3 - 1).reshape(-1, 1, 1) + off[0, 1::2].astype(np.float64)
    term, share = mc.coord_rounding_term(x, px, py)
    gain = np.abs(wt.astype(np.float64)).reshape(O, dg, C // dg, 9).sum(2).reshape(O, dg * 9)       # sum over the channels of a group
    gain = float(np.einsum("oj,jyx->oyx", gain, msk[0].astype(np.float64)).max())
    _report(f"{what} {h}x{w} R={R:g} (sum|w mask| = {gain:.1f})", got, ref, 3e-5, term * gain, share, R)
    assert np.abs(ref - b.reshape(1, -1, 1, 1)).max() > 0.5


@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("C,O,dg", [(32, 32, 8), (8, 12, 2)])
def test_dcnv2_vs_float64(C, O, dg, h, w, R):
    from crfp_amd import ops
    x, off, msk, wt, b = _dcn_inputs(C + h + int(R), C, O, dg * 9, h, w, R)
    got = ops.dcnv2(*[T(a).to(dev()) for a in (x, off, msk, wt, b)], 3, 1, 1, dg)
    _dcn_check(f"dcnv2 {C}/{O}/{dg}", got, x, off, msk, wt, b, dg, R)


@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_dcnv2_shared_vs_float64(h, w, R):
    from crfp_amd import ops
    x, off, msk, wt, b = _dcn_inputs(77 + h + int(R), 4, 4, 1, h, w, R)
    got = ops.dcnv2_shared(*[T(a).to(dev()) for a in (x, off, msk, wt, b)])
    _dcn_check("dcnv2_shared 4/4", got, x, np.tile(off, (1, 9, 1, 1)), np.tile(msk, (1, 9, 1, 1)), wt, b, 1, R)
