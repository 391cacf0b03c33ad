"""GPU (-m gpu): the regional runtime engine (``crfp_rt_forward_clip``, csrc/engine_rt.hip) under steered motion, stage by stage.

Every other test of this engine runs ``make_state_dict_like`` weights, whose flow stays below 2 LR pixels.  Here the flow network is steered
(tests/helpers/motion_cases.py, ``window_case``) to +-24, +-60 and saturating LR pixels on windows that can hold such motion, and to the `edge`
regime (+-5 px, both signs on both axes) on windows of 8 to 13 LR pixels; all statistics are in-window, because FNet sees the top-left LR
window only.  The engine's own flow is read out of its workspace (``RuntimeEngine.debug_fetch("flow_lr")``, ``crfp_rt_debug_fetch``) and
injected into the float64 oracle (``oracle.runtime_oracle.runtime_forward(flows=, taps=)``), so a comparison measures the warps, the DCNs, the
crop / paste kernels and everything behind them, not the drift between two fp32 evaluations of tanh * 256.

Bounds.  Output: max |HIP - oracle64| < 2e-4, the bound test_runtime_engine_one_call_vs_reference_golden_and_oracle holds this engine to at
small motion.  Stages: 2e-4 * max(1, max |tap|) per tensor.  Flow: FLOW_TOL = 0.05 px against the oracle's flow (test_gpu_motion.py).
Schedules, batches and used or dirty workspaces: bit equality.

Measured on an MI355X (max |HIP - oracle64| over the clip; the fp32 oracle against its float64 run with the same flow; whether the engine's
flow equals ``m.compute_flow(window crop)`` bit for bit):

    case / regime              HIP vs oracle64   oracle fp32 vs fp64   engine flow vs oracle flow   == m.compute_flow
    inside / moderate            1.04e-05           1.67e-05              1.50e-04 px               no
    inside / large               1.61e-05           1.92e-05              1.51e-04 px               no
    inside / saturating          7.10e-06           4.66e-06              1.14e-04 px               no
    full-width / moderate        1.22e-05           1.30e-05              1.52e-04 px               no
    full-width / large           7.69e-06           1.06e-05              1.51e-04 px               no
    full-width / saturating      9.15e-07           1.46e-06              9.35e-05 px               no
    whole-ragged / moderate      4.88e-06           8.13e-06              1.16e-04 px               no
    whole-ragged / saturating    7.10e-07           9.06e-07              7.63e-05 px               no
    ragged-window / edge         9.90e-07           8.71e-07              3.36e-05 px               no
    smallest / edge              5.72e-07           1.03e-06              5.84e-05 px               no
    y_only full-width / large    7.75e-06           1.06e-05              1.51e-04 px               no
    y_only, the batch's clip 1   6.84e-06           5.79e-06              1.26e-04 px               no

(``m.compute_flow`` of the regional model is the per-operator FNet module, another launch sequence than the engine's FNet pass: close, not equal
bits, which is why the fetched flow is the one injected.)  The engine sits as close to float64 as the fp32 oracle does; no case came near the
bound and no defect was found.  full-width/large, frame 1: the window-warp oracle and one that warps the full frame and crops are 1.41e-2
apart; the engine is 7.5e-6 from the first and 1.41e-2 from the second.

Stage by stage, frame 1 of the two clips cut to t = 2: max |HIP - tap64| (max |tap64|), bound 2e-4 * max(1, max |tap64|):

    buffer      inside / large            ragged-window / edge
    state_w     1.16e-05 (0.49)           2.18e-06 (0.40)
    carryw      4.30e-06 (0.95)           7.55e-07 (0.71)
    prev2w      5.10e-06 (0.38)           1.53e-06 (0.43)
    prev2       4.00e-07 (0.46)           3.97e-07 (0.57)
    aligned0    6.48e-06 (0.40)           1.08e-06 (0.26)
    aligned1    1.01e-05 (0.39)           1.83e-06 (0.39)
    aligned2    9.17e-06 (0.29)           1.75e-06 (0.30)
    poff        4.60e-05 (79.4)           2.65e-06 (3.42)
    al3         1.79e-05 (0.56)           2.04e-06 (0.23)
    state       7.16e-06 (1.10)           7.64e-07 (1.32)
    feat2       7.16e-06 (1.32)           7.64e-07 (1.32)
    x_lr        1.09e-06 (1.99)           8.28e-07 (1.99)
    x_hr        3.34e-07 (1.02)           3.22e-07 (1.03)
    flow2       1.14e-05 (116)            0        (6.39)
    flow8       5.39e-05 (465)            0        (25.6)
    win         6.56e-07 (1.37)           7.34e-07 (1.55)
    upw         7.91e-07 (1.46)           6.96e-07 (1.74)
    offfeat0    1.68e-05 (44.4)           1.33e-06 (2.42)
    offfeat1    2.94e-05 (51.2)           1.76e-06 (1.95)
    offfeat2    2.53e-05 (31.7)           1.68e-06 (1.77)
    carry       2.62e-06 (1.01)           9.08e-07 (1.02)

ragged-window: the carried state inside the fovea's 56 columns is 7.6e-7 from the pasted conv_tttf crop and 1.20 from the LeakyReLU branch.

Large-motion timing of this engine is not measured here or anywhere else."""
import functools

import numpy as np
import pytest
import torch

from helpers import motion_cases as mc

pytestmark = pytest.mark.gpu

T = torch.from_numpy
BOUND = 2e-4          # the bound this engine is held to against the oracle at small motion (test_gpu_round3.py)
FLOW_TOL = 0.05       # pixels: engine flow vs oracle flow (test_gpu_motion.py)
STAGES = ["state_w", "carryw", "prev2w", "prev2", "aligned0", "aligned1", "aligned2", "poff", "al3", "state", "feat2"]
# the other names of the fetch, held to the same per-tensor bound
MORE = ["x_lr", "x_hr", "flow_lr", "flow2", "flow8", "win", "upw", "offfeat0", "offfeat1", "offfeat2", "carry"]


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
def _case(name, regime=None, t=3, seed=None, y_only=False):
    sd, lrs, fvs, warp = mc.window_case(name, regime, seed=seed, y_only=y_only)
    return sd, lrs[:, :t], fvs[:, :t], warp


@functools.lru_cache(maxsize=None)
def _model(y_only=False):
    """One model per output form: every window case carries the same weights (``window_case``'s weights_seed)."""
    from crfp_amd.model import MRCF_runtime
    sd = _case("smallest", y_only=y_only)[0]
    m = MRCF_runtime.MRCF_simple_v18(mid_channels=32, y_only=y_only, hr_dcn=True, offset_prop=True, split_ratio=3, device=dev())
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev()).eval()
    m.print_timings = False       # -> crfp_rt_forward_clip
    return m


@functools.lru_cache(maxsize=None)
def _params(y_only=False, double=False):
    from oracle import crfp_oracle
    P = crfp_oracle.load_numpy_state(_case("smallest", y_only=y_only)[0])
    return {k: v.double() for k, v in P.items()} if double else P


def _forward(m, lrs, fvs, warp):
    return m(T(lrs).to(dev()), T(fvs).to(dev()), warp_size=warp)


@functools.lru_cache(maxsize=None)
def _engine_run(name, regime=None, t=3, seed=None, y_only=False):
    """One clip through the engine: the output and every fetchable buffer, on the CPU (fetched before another geometry takes the workspace)."""
    _, lrs, fvs, warp = _case(name, regime, t, seed, y_only)
    m = _model(y_only)
    out = _forward(m, lrs, fvs, warp)
    eng = m.engine()
    assert m._engine_takes(T(lrs), T(fvs), warp), "the clip would take the per-operator composition"
    got = {n: eng.debug_fetch(n).cpu() for n in STAGES + MORE}
    got["out"], got["overflowed"] = out.cpu(), eng.overflowed()
    return got


def _flows(run):
    return run["flow_lr"][:, :2].unsqueeze(0).contiguous()       # [1, t-1, 2, whl, wwl]: channels 2, 3 of the quad are padding


@functools.lru_cache(maxsize=None)
def _oracle64(name, regime=None, t=3, seed=None, y_only=False):
    """The float64 oracle with the engine's flow, once per case: (output, taps of the last frame)."""
    from oracle import runtime_oracle as ro
    _, lrs, fvs, warp = _case(name, regime, t, seed, y_only)
    taps = {}
    ref = ro.runtime_forward(_params(y_only, True), T(lrs).double(), T(fvs).double(), warp, y_only=y_only,
                             flows=_flows(_engine_run(name, regime, t, seed, y_only)), taps=taps)
    return ref, taps


def _check_against_oracle(orc, what, name, regime, seed=None, y_only=False):
    """(a): regime and flow checks on the fetched flow, then the engine against the float64 oracle with that flow."""
    from oracle import runtime_oracle as ro
    _, lrs, fvs, warp = _case(name, regime, 3, seed, y_only)
    whl, wwl = warp[0] // 8, warp[1] // 8
    run = _engine_run(name, regime, 3, seed, y_only)
    flows, out = _flows(run), run["out"]
    P = _params(y_only)
    crop = T(lrs)[:, :, :, :whl, :wwl].contiguous()
    s = mc.flow_stats(flows, whl, wwl)
    d_flow = float((flows - orc.compute_flow(P, crop)).abs().max())
    same = torch.equal(_model(y_only).compute_flow(crop.to(dev()))[0].cpu(), flows)
    print(f"{what}: engine flow {mc.fmt_stats(s)}; max|engine flow - oracle flow| = {d_flow:.2e} px; bit-equal to m.compute_flow(window crop): {same}")
    if regime is not None:
        mc.assert_regime(s, regime)
    assert d_flow < FLOW_TOL, d_flow
    ref64, _ = _oracle64(name, regime, 3, seed, y_only)
    ref32 = ro.runtime_forward(P, T(lrs), T(fvs), warp, y_only=y_only, flows=flows)
    still = ro.runtime_forward(P, T(lrs)[:, :2], T(fvs)[:, :2], warp, y_only=y_only, flows=flows[:, :1] * 0)
    d64 = float((out.double() - ref64).abs().max())
    d_ref = float((ref32.double() - ref64).abs().max())
    moved = float((ref32[:, 1] - still[:, 1]).abs().max())
    print(f"{what}: max|HIP - oracle64(engine flow)| = {d64:.3e} (bound {BOUND:.0e}); oracle fp32 vs fp64 = {d_ref:.3e}; "
          f"frame 1 with this flow vs with zero flow: {moved:.3f}")
    assert tuple(out.shape) == tuple(ref64.shape)
    assert not run["overflowed"]
    assert moved > 1e-2, "the motion does not reach the output"
    assert torch.isfinite(out).all() and d64 < BOUND, d64


# ----------------------------------------------------------------------------- (a) engine against the float64 oracle with the engine's flow
@pytest.mark.parametrize("name,regime", mc.WINDOW_ROWS)
def test_rt_vs_oracle64_with_the_engines_flow(orc, name, regime):
    _check_against_oracle(orc, f"{name}/{regime}", name, regime)


# ----------------------------------------------------------------------------- (b) stage by stage
@pytest.mark.parametrize("name,regime", [("inside", "large"), ("ragged-window", "edge")])
def test_rt_stage_by_stage(name, regime):
    """Frame 1 of the clip cut to t = 2: every fetched buffer against the float64 oracle's tap (the P4 pad is stripped by the fetch)."""
    _, lrs, fvs, warp = _case(name, regime, 2)
    run, (_, taps) = _engine_run(name, regime, 2), _oracle64(name, regime, 2)
    mc_stats = mc.flow_stats(_flows(run), warp[0] // 8, warp[1] // 8)
    assert mc_stats["absmax"] >= 2.5, mc_stats
    worst = []
    for n in STAGES + MORE:
        got, want = run[n].double(), taps[n]
        if n == "flow_lr":
            got = got[:, :2]
        assert tuple(got.shape) == tuple(want.shape), (n, tuple(got.shape), tuple(want.shape))
        d, scale = float((got - want).abs().max()), max(1.0, float(want.abs().max()))
        print(f"{name}/{regime} t=2 {n:9s}: max|HIP - tap64| = {d:.3e}, max|tap64| = {float(want.abs().max()):.3e} (bound {BOUND * scale:.1e})")
        if not (np.isfinite(d) and d < BOUND * scale):
            worst.append((n, d, BOUND * scale))
    assert not worst, f"first stage that departs: {worst[0]}; all: {worst}"
    assert torch.equal(run["state"], run["feat2"][:, :, :warp[0], :warp[1]]), "the carried state is not the window of the frame's features"
    if name == "ragged-window":
        fh, fw = fvs.shape[-2:]
        assert fh > warp[0] and fw < warp[1]
        state, pasted, branch = run["state"][:, :, :, :fw].double(), taps["tttf"][:, :, :warp[0]], taps["feat_pre"][:, :, :warp[0], :fw]
        apart = float((pasted - branch).abs().max())
        d_paste, d_branch = float((state - pasted).abs().max()), float((state - branch).abs().max())
        print(f"{name}: state inside the fovea's {fw} columns: vs the pasted conv_tttf {d_paste:.3e}, vs the LeakyReLU branch {d_branch:.3e} "
              f"(the two are {apart:.3f} apart)")
        assert apart > 1e-2 and d_paste < BOUND * max(1.0, float(pasted.abs().max())) and d_branch > 1e-2


# ----------------------------------------------------------------------------- (c) out-of-window samples read zero, not the frame
def test_rt_case_tells_window_warp_from_frame_warp(orc):
    """full-width/large cut to t = 2.  The reference warps the window-sized state, so a sample that leaves the window reads zero even where the
    frame has pixels.  An oracle that warps the full-frame features and crops afterwards moves frame 1 by far more than the bound, and the
    engine sits with the window semantics: passing (a) on this case means something."""
    from oracle import runtime_oracle as ro
    name, regime = "full-width", "large"
    _, lrs, fvs, warp = _case(name, regime, 2)
    h, w = lrs.shape[-2:]
    assert warp[0] < 8 * h and warp[1] == 8 * w           # rows of the frame below the window
    P64, L, Fv = _params(False, True), T(lrs).double(), T(fvs).double()
    flows = _flows(_engine_run(name, regime, 3))[:, :1]    # frames 0 and 1 of the t = 3 run
    window = ro.runtime_forward(P64, L, Fv, warp, flows=flows)
    taps0 = {}
    ro.runtime_forward(P64, L[:, :1], Fv[:, :1], warp, taps=taps0)
    frame0 = taps0["feat2"]
    real = orc.flow_warp

    def frame_warp(x, flow, padding_mode="zeros"):
        if x.shape[1] != 4:                                # the carried 2x features are window tensors under either reading
            return real(x, flow, padding_mode)
        assert torch.equal(x, frame0[:, :, :warp[0], :warp[1]])
        full = torch.zeros(1, 8 * h, 8 * w, 2, dtype=flow.dtype)
        full[:, :warp[0], :warp[1]] = flow
        return real(frame0, full, padding_mode)[:, :, :warp[0], :warp[1]]

    orc.flow_warp = frame_warp
    try:
        frame = ro.runtime_forward(P64, L, Fv, warp, flows=flows)
    finally:
        orc.flow_warp = real
    apart = float((window[:, 1] - frame[:, 1]).abs().max())
    out = _engine_run(name, regime, 3)["out"][:, :2].double()
    d_window, d_frame = float((out - window).abs().max()), float((out - frame).abs().max())
    print(f"{name}/{regime}: window warp vs frame warp, frame 1: {apart:.3f}; engine vs window {d_window:.3e}, vs frame {d_frame:.3e}")
    assert torch.equal(window[:, 0], frame[:, 0]) and apart > 1e-2
    assert d_window < BOUND and d_frame > 1e-2


# ----------------------------------------------------------------------------- (d) dirty workspace
@pytest.mark.parametrize("name,regime,other", [("inside", "large", ("saturating", None)), ("smallest", "edge", ("edge", 4))])
def test_rt_dirty_and_used_workspace(name, regime, other):
    """Every byte the engine reads is first written or cleared by the call: a workspace of 0xFF bytes (every float a NaN) gives the bits of
    a zeroed one, and a clip that follows another clip in the same workspace gives them too (state and carry are reset per call)."""
    _, lrs, fvs, warp = _case(name, regime)
    m = _model()
    eng = m.engine()
    key = (3,) + tuple(lrs.shape[-2:]) + tuple(fvs.shape[-2:]) + tuple(warp)
    ws = eng._workspace(key)
    ws.zero_()
    clean = _forward(m, lrs, fvs, warp).clone()
    assert eng._workspace(key) is ws and torch.isfinite(clean).all() and not eng.overflowed()
    ws.fill_(0xFF)
    assert torch.isnan(ws[-64:].view(torch.float32)).all()
    dirty = _forward(m, lrs, fvs, warp).clone()
    assert not eng.overflowed()
    assert torch.equal(dirty, clean), f"a dirty workspace changes the result: max|delta| = {float((dirty - clean).abs().max()):.3e}"
    _, lrs2, fvs2, warp2 = _case(name, other[0], 3, other[1])
    assert warp2 == warp and lrs2.shape == lrs.shape and not np.array_equal(lrs2, lrs)
    first = _forward(m, lrs2, fvs2, warp2).clone()
    again = _forward(m, lrs, fvs, warp)
    assert eng._workspace(key) is ws and not eng.overflowed()
    assert torch.equal(again, clean), "a used workspace changes the result"
    assert float((first - clean).abs().max()) > 1e-2
    assert torch.equal(clean.cpu(), _engine_run(name, regime)["out"])


# ----------------------------------------------------------------------------- (e) schedules
@pytest.mark.parametrize("name,regime", [("inside", "large"), ("ragged-window", "edge")])
def test_rt_single_stream_gives_the_four_stream_bits(name, regime):
    _, lrs, fvs, warp = _case(name, regime)
    m = _model()
    eng = m.engine()
    assert not eng.single_stream
    four = _forward(m, lrs, fvs, warp).clone()
    eng.single_stream = True
    try:
        one = _forward(m, lrs, fvs, warp).clone()
    finally:
        eng.single_stream = False
    assert torch.isfinite(four).all() and torch.equal(one, four)
    assert torch.equal(four.cpu(), _engine_run(name, regime)["out"])


# ----------------------------------------------------------------------------- (f) y_only and a batch of two
def test_rt_y_only_batch_of_two(orc):
    """Clip 0 is full-width/large, clip 1 the same geometry with another seed (WINDOW_BATCH_SEED, in the large regime as well): each clip of the n = 2 call equals its n = 1 call bit for bit,
    and both y_only outputs hold (a)'s bound."""
    name, regime = "full-width", "large"
    clips = [_case(name, regime, 3, seed, True) for seed in (None, mc.WINDOW_BATCH_SEED)]
    warp = clips[0][3]
    assert not np.array_equal(clips[0][1], clips[1][1])
    m = _model(True)
    singles = [_engine_run(name, regime, 3, seed, True)["out"] for seed in (None, mc.WINDOW_BATCH_SEED)]
    both = _forward(m, np.concatenate([c[1] for c in clips], 0), np.concatenate([c[2] for c in clips], 0), warp)
    assert not m.engine().overflowed()
    assert tuple(both.shape) == (2, 3, 1, 8 * clips[0][1].shape[-2], 8 * clips[0][1].shape[-1])
    assert torch.equal(both[:1].cpu(), singles[0]) and torch.equal(both[1:].cpu(), singles[1]), "a clip of the batch differs from its one-clip call"
    assert float((singles[0] - singles[1]).abs().max()) > 1e-2
    _check_against_oracle(orc, f"y_only {name}/{regime}", name, regime, None, True)
    _check_against_oracle(orc, f"y_only {name}/{regime} seed {mc.WINDOW_BATCH_SEED}", name, regime, mc.WINDOW_BATCH_SEED, True)


# ----------------------------------------------------------------------------- (g) refusals
def test_rt_debug_fetch_refusals():
    from crfp_amd import engine
    m = _model()
    _, lrs, fvs, warp = _case("smallest", "edge")
    _forward(m, lrs, fvs, warp)
    eng = m.engine()
    with pytest.raises(RuntimeError, match="unknown buffer 'no_such_buffer'"):
        eng.debug_fetch("no_such_buffer")
    assert tuple(eng.debug_fetch("state").shape) == (1, 4, 64, 64)
    _forward(m, lrs[:, :1], fvs[:, :1], warp)                 # one frame: nothing is warped
    with pytest.raises(RuntimeError, match="frames >= 1"):
        eng.debug_fetch("state_w")
    assert tuple(eng.debug_fetch("feat2").shape) == (1, 4, 8 * lrs.shape[-2], 8 * lrs.shape[-1])
    fresh = engine.RuntimeEngine(m.state_dict(), dev())
    with pytest.raises(RuntimeError, match="before any forward"):   # it raises rather than reading a stale workspace
        fresh.debug_fetch("state")
