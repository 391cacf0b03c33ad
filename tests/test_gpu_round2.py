"""GPU (-m gpu), round 2: longer recurrences, BASELINE-size clips, the numerics guard, graph capture and the boundary
conventions of DCNv2 against a third, independent restatement.  Everything goes through the C-ABI."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import golden_io  # noqa: E402
from conftest import GOLDEN  # noqa: E402

T = torch.from_numpy


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def maxdiff(a, b):
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else T(np.asarray(a))
    b = b.detach().cpu() if isinstance(b, torch.Tensor) else T(np.asarray(b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


@pytest.fixture(scope="module")
def orc():
    from oracle import crfp_oracle
    return crfp_oracle


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


def _model(sd_np, y_only=False, cls="CRFP_DSV"):
    from crfp_amd.model import CRFP
    m = getattr(CRFP, cls)(device=dev(), mid_channels=32, y_only=y_only, hr_dcn=True, offset_prop=True)
    m.load_state_dict({k: T(v.copy()) for k, v in sd_np.items()}, strict=True)
    return m.to(dev()).eval()


# ------------------------------------------------------------------------------------------------ streaming
def test_streaming_through_one_reused_input_buffer():
    """A caller that refills ONE device buffer per input in place: the previous LR frame the engine hands to
    FNet must be its own copy (model/CRFP_test.py:2234-2238 clones it)."""
    from crfp_amd import synth
    g = golden_io.load("stream_16x24_t7")
    sd = synth.make_state_dict(int(g["weights_seed"]))
    t, h, w = int(g["t"]), int(g["h"]), int(g["w"])
    lrs, fvs, mks = synth.make_clip(int(g["clip_seed"]), 1, t, h, w, fv_size=int(g["fv_size"]), sigma_t=10.0)
    m = _model(sd, cls="MRCF_simple_v18")
    d = dev()
    L = torch.empty((1, 1, 3, h, w), device=d)
    Fv = torch.empty((1, 1, 3, 8 * h, 8 * w), device=d)
    M = torch.empty((1, 1, 1, 8 * h, 8 * w), device=d, dtype=torch.bool)
    Fg = torch.empty((1, 1, 1, 8 * h, 8 * w), device=d, dtype=T(g["fgs"]).dtype)
    outs = []
    for i in range(t):
        if i == int(g["clear_at"]):
            m.clear_states()
        L.copy_(T(lrs[:, i:i + 1])); Fv.copy_(T(fvs[:, i:i + 1])); M.copy_(T(mks[:, i:i + 1])); Fg.copy_(T(g["fgs"][:, i:i + 1]))
        outs.append(m(L, Fv, M, Fg).clone())
    assert maxdiff(torch.cat(outs, dim=1), g["out"]) < 2e-4


def _gaze_stream(orc, h, w, n_frames, sigma, fv_size, seed, hip_model, P):
    """Drive the HIP streaming model and StreamOracle with the video rig's gaze trajectory and fovea masks
    (test_video.py:303-379) and return the per-call max |HIP - oracle|."""
    from crfp_amd import gaze, synth
    chunk = 10
    lrs = np.concatenate([synth.make_clip(seed + i, 1, min(chunk, n_frames - i), h, w, fv_size=fv_size)[0][0]
                          for i in range(0, n_frames, chunk)], 0)
    lr = T(lrs)
    rs = np.random.RandomState(seed)
    gt = torch.clamp(F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False) +
                     T(rs.normal(0, 0.03, (n_frames, 3, 8 * h, 8 * w)).astype(np.float32)), 0, 1)
    H, W = 8 * h, 8 * w
    xs, ys = gaze.gaze_trajectory(n_frames, H, W, sigma, np.random.RandomState(seed))
    masks = gaze.RegionMasks(H, W, fv_size, torch.device("cpu"))
    so = orc.StreamOracle(P)
    hip_model.clear_states()
    d = dev()
    diffs = []
    for n in range(n_frames):
        cy, cx = gaze.window_origin(xs[n], ys[n], fv_size, H, W)
        mk = masks.frame(n, cy, cx)["mk"]
        fv = gt[n:n + 1] * mk
        ref = so(lr[n:n + 1].unsqueeze(0), fv.unsqueeze(0), mk.unsqueeze(0))
        got = hip_model(lrs=lr[n:n + 1].unsqueeze(0).to(d), fvs=fv.unsqueeze(0).to(d), mks=mk.unsqueeze(0).to(d))
        diffs.append(maxdiff(got, ref))
    return diffs


def test_stream_100_calls_sigma50_vs_oracle(orc):
    """BASELINE config 3's call pattern: 100 calls of the one-frame-per-call model under a sigma^T = 50 px gaussian gaze
    trajectory, against StreamOracle -- drift of the recurrent state over a long sequence.  45x80 -> 360x640 keeps the
    oracle at ~0.3 s per call; the first 10 calls are repeated at the real 180x320 -> 1440x2560 size."""
    from crfp_amd import synth
    sd = synth.make_state_dict(7)
    P = orc.load_numpy_state(sd)
    m = _model(sd, cls="MRCF_simple_v18")
    diffs = _gaze_stream(orc, 45, 80, 100, 50.0, 96, 1234, m, P)
    curve = [max(diffs[i:i + 10]) for i in range(0, 100, 10)]
    print("drift curve, max|HIP - oracle| per 10 calls @45x80:", " ".join(f"{v:.2e}" for v in curve))
    assert max(diffs) < 1e-3                                   # the north-star tolerance, held over the whole sequence
    assert max(diffs[50:]) < 4 * max(max(diffs[:50]), 1e-6)    # and no run-away growth
    big = _gaze_stream(orc, 180, 320, 10, 50.0, 96, 4321, m, P)
    print("first 10 calls @180x320:", " ".join(f"{v:.2e}" for v in big))
    assert max(big) < 1e-3


# ------------------------------------------------------------------------------------------------ BASELINE sizes
def test_config_a_seven_frames_vs_oracle(orc):
    """BASELINE configs[1] in full: 7 frames 180x320 -> 1440x2560, fp32 semantics, sigma^T = 10, against the oracle
    (the 7-frame comparison used to live only behind a bench.py flag)."""
    from crfp_amd import synth
    sd = synth.make_state_dict(7)
    P = orc.load_numpy_state(sd)
    lrs, fvs, mks = synth.make_clip(1234, 1, 7, 180, 320, fv_size=96, sigma_t=10.0)
    m = _model(sd)
    d = dev()
    out = m(lrs=T(lrs).to(d), fvs=T(fvs).to(d), mks=T(mks).to(d))
    assert not m.engine().overflowed()
    ref = orc.crfp_dsv_forward(P, T(lrs), T(fvs), T(mks))
    per_frame = [maxdiff(out[:, i], ref[:, i]) for i in range(7)]
    print("config A per-frame max|HIP - oracle|:", " ".join(f"{v:.2e}" for v in per_frame))
    assert max(per_frame) < 1e-3
    assert max(per_frame) < 1e-4   # what the split-fp16 scheme actually holds


# ------------------------------------------------------------------------------------------------ numerics guard
def test_fp16_operand_overflow_is_never_silent(orc):
    """Activations scaled past the fp16 operand range of the split-fp16 scheme (|v| >= 65504): the default policy fills
    the output with NaN and raises the status word; 'raise' raises; 'fallback' reruns in strict fp32 and is CORRECT;
    precision='f32' is correct from the start.  Never a finite-but-wrong frame."""
    from crfp_amd import synth
    sd = synth.make_state_dict(7)
    h, w, t = 16, 24, 3
    lrs, fvs, mks = synth.make_clip(5, 1, t, h, w, fv_size=48)
    scale = 1.0e5
    lrs, fvs = lrs * scale, fvs * scale
    P = orc.load_numpy_state(sd)
    ref = orc.crfp_dsv_forward(P, T(lrs), T(fvs), T(mks))
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 65504
    d = dev()
    args = dict(lrs=T(lrs).to(d), fvs=T(fvs).to(d), mks=T(mks).to(d))
    m = _model(sd)
    out = m(**args)
    assert m.engine().overflowed()
    assert torch.isnan(out).all(), "an overflowed clip must not return finite frames"
    m.on_overflow = "raise"
    with pytest.raises(FloatingPointError, match="65504"):
        m(**args)
    tol = 2e-5 * float(ref.abs().max())
    m.on_overflow = "fallback"
    assert maxdiff(m(**args), ref) < tol
    m.on_overflow, m.precision = "poison", "f32"
    assert maxdiff(m(**args), ref) < tol
    # in-range inputs leave the word clear and the two precisions agree
    lrs2, fvs2, mks2 = synth.make_clip(5, 1, t, h, w, fv_size=48)
    a2 = dict(lrs=T(lrs2).to(d), fvs=T(fvs2).to(d), mks=T(mks2).to(d))
    strict = m(**a2)
    m.precision = "split"
    fast = m(**a2)
    assert not m.engine().overflowed() and maxdiff(fast, strict) < 1e-4
    # streaming: the word is sticky over the sequence and cleared by clear_states()
    ms = _model(sd, cls="MRCF_simple_v18")
    ms.clear_states()
    for i in range(2):
        o = ms(args["lrs"][:, i:i + 1], args["fvs"][:, i:i + 1], args["mks"][:, i:i + 1])
    assert ms.engine().overflowed(stream=True) and torch.isnan(o).all()
    ms.clear_states()
    o = ms(a2["lrs"][:, :1], a2["fvs"][:, :1], a2["mks"][:, :1])
    assert not ms.engine().overflowed(stream=True) and torch.isfinite(o).all()


# ------------------------------------------------------------------------------------------------ DCNv2 conventions
@pytest.mark.parametrize("C,O,dg,H,W", [(32, 32, 8, 9, 37), (4, 4, 1, 11, 70), (8, 12, 2, 6, 5)])
def test_dcnv2_vs_paper_equations(C, O, dg, H, W):
    """All three HIP DCN kernels (dcn_g8 MFMA, shared-offset c4, generic) against the float64 restatement written from
    the DCN papers' equations (tests/dcn_paper_ref.py), with sampling positions straddling -1, 0, H-1 and H."""
    from crfp_amd import ops
    from dcn_paper_ref import boundary_offsets, dcnv2_paper
    rs = np.random.RandomState(C + H)
    x = rs.standard_normal((2, C, H, W)).astype(np.float32)
    off = boundary_offsets(rs, 2, dg, H, W)
    m = rs.uniform(0, 1, (2, dg * 9, H, W)).astype(np.float32)
    w = (rs.standard_normal((O, C, 3, 3)) * 0.2).astype(np.float32)
    b = rs.standard_normal(O).astype(np.float32)
    ref = dcnv2_paper(x, off, m, w, b, dg)
    got = ops.dcnv2(*[T(a).to(dev()) for a in (x, off, m, w, b)], 3, 1, 1, dg).cpu().numpy().astype(np.float64)
    assert np.abs(got - ref).max() < 3e-5


def test_dcn_module_shared_offsets_vs_paper_equations(orc):
    """dcn_3's wiring (one (dy,dx,mask) per pixel tiled over the 9 taps, model/CRFP.py:341-347) on the engine's compact
    dcn3 kernel, through DCN_module, vs the paper-equation restatement fed the TILED tensors."""
    from crfp_amd.model import CRFP
    from dcn_paper_ref import dcnv2_paper
    rs = np.random.RandomState(3)
    H, W = 13, 70
    mod = CRFP.DCN_module(4, 1, 3, 10, repeat=True).to(dev())
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(T((rs.standard_normal(tuple(p.shape)) * 0.3).astype(np.float32)))
    cur, pre, prew = (T(rs.standard_normal((1, 4, H, W)).astype(np.float32)) for _ in range(3))
    flow = T(rs.uniform(-3, 3, (1, 2, H, W)).astype(np.float32))
    flow[0, :, 0, :] = -4.0          # push the first row's samples across the top border
    flow[0, 0, :, -1] = 3.5          # and the last column across the right border
    got, feat = mod(cur.to(dev()), pre.to(dev()), prew.to(dev()), flow.to(dev()))
    P = {"m." + k: v.detach().cpu() for k, v in mod.state_dict().items()}
    f = torch.cat([cur, prew, flow], 1)
    f = orc.lrelu(orc.conv(P, "m.dcn_block.2", orc.lrelu(orc.conv(P, "m.dcn_block.0", f))))
    off = 10 * torch.tanh(orc.conv(P, "m.dcn_offset", f)) + flow.flip(1)
    msk = torch.sigmoid(orc.conv(P, "m.dcn_mask", f))
    ref = dcnv2_paper(pre.numpy(), off.repeat(1, 9, 1, 1).numpy(), msk.repeat(1, 9, 1, 1).numpy(),
                      P["m.dcn.weight"].numpy(), P["m.dcn.bias"].numpy(), 1)
    assert np.abs(got.cpu().numpy() - ref).max() < 1e-4


# ------------------------------------------------------------------------------------------------ graph capture
def test_clip_forward_is_graph_capturable_and_replays_bit_exact():
    """crfp_dsv_forward_clip (two-stream schedule: fork / join through events) captured into a HIP graph once and
    replayed on new inputs equals the eager call bit for bit."""
    from crfp_amd import synth
    sd = synth.make_state_dict(7)
    h, w, t = 24, 40, 3
    d = dev()
    clips = [synth.make_clip(s, 1, t, h, w, fv_size=64) for s in (31, 32)]
    m = _model(sd)
    eng = m.engine()
    eager = [m(lrs=T(c[0]).to(d), fvs=T(c[1]).to(d), mks=T(c[2]).to(d)).clone() for c in clips]   # also warms up side stream + events
    L, Fv, M = (T(a).to(d).clone() for a in clips[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.forward(L, Fv, M)
    for i in (0, 1, 0):
        L.copy_(T(clips[i][0])); Fv.copy_(T(clips[i][1])); M.copy_(T(clips[i][2]))
        g.replay()
        torch.cuda.synchronize()
        assert maxdiff(out, eager[i]) == 0.0


# ------------------------------------------------------------------------------------------------ SPyNet (a-4)
def test_spynet_vs_reference_golden(orc):
    """crfp_spynet_forward (one native call: resize + normalise, 5-level avg-pool pyramid, align_corners=True flow
    upsampling, border warp, 30 ReLU-before-conv 7x7 convs) against the flow of the imported reference SPyNet, for a size
    that is resized up to a multiple of 32 and one that is not; the per-operator route (SPyNet.compute_flow) agrees."""
    from crfp_amd import synth
    from crfp_amd.model import CRFP
    g = dict(np.load(os.path.join(GOLDEN, "spynet_small.npz")))
    sd = synth.make_spynet_state_dict(int(g["weights_seed"]))
    m = CRFP.SPyNet(None, dev())
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev()).eval()
    for tag in "ab":
        ref, supp = T(g[tag + "_ref"]).to(dev()), T(g[tag + "_supp"]).to(dev())
        flow = m(ref, supp)
        assert maxdiff(flow, g[tag + "_flow"]) < 2e-4, tag          # pixels; flows reach ~2 px
    ref, supp = T(g["b_ref"]).to(dev()), T(g["b_supp"]).to(dev())   # 64 x 96: forward == compute_flow (no resize)
    assert maxdiff(m.compute_flow(ref, supp), g["b_flow"]) < 2e-4
    # SPyNetBasicModule alone, signed input: the ReLU sits in front of every conv, the first included (model/CRFP.py:152)
    assert maxdiff(m.basic_module[3](T(g["bm_x"]).to(dev())), g["bm_y"]) < 1e-4
    x = T(g["bm_x"]).to(dev())
    w, b = m.basic_module[3].basic_module[0].conv.weight, m.basic_module[3].basic_module[0].conv.bias
    from crfp_amd import ops
    assert maxdiff(ops.convkxk(x, w, b, pre_relu=True), F.conv2d(F.relu(x.cpu()), w.cpu(), b.cpu(), padding=3)) < 2e-5
    assert maxdiff(ops.convkxk(x, w, b, pre_relu=False), F.conv2d(x.cpu(), w.cpu(), b.cpu(), padding=3)) < 2e-5
    up = ops.upsample_bilinear_ac(x, 2, mul=2.0)
    assert maxdiff(up, F.interpolate(x.cpu(), scale_factor=2, mode="bilinear", align_corners=True) * 2.0) < 1e-5


# ------------------------------------------------------------------------------------------------ regional-DCN runtime wiring (a-20 / f4)
def test_runtime_variant_vs_reference_golden(orc, capsys):
    """``MRCF_runtime.MRCF_simple_v18(...)(lr, fv, warp_size=)`` -- the call test_runtime.py:41,142 makes -- on the HIP
    operators against the output of the reference class (tests/golden/runtime_small.npz) and, at another geometry, against
    the oracle twin; it prints the reference's six per-stage lines."""
    from crfp_amd import synth
    from crfp_amd.model import MRCF_runtime
    from oracle import runtime_oracle as ro
    g = golden_io.load("runtime_small")
    m = MRCF_runtime.MRCF_simple_v18(mid_channels=32, y_only=False, hr_dcn=True, offset_prop=True, split_ratio=3,
                                     spynet_pretrained='pretrained_models/fnet.pth', device=dev())
    sd = synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["weights_seed"]))
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev()).eval()
    m.print_timings = True         # per-operator composition with the reference's stage prints; the default is the one-call engine (round 3)
    out = m(T(g["lrs"]).to(dev()), T(g["fvs"]).to(dev()), warp_size=tuple(int(v) for v in g["warp"]))
    assert maxdiff(out, g["out"]) < 2e-4
    printed = capsys.readouterr().out.split()
    assert printed[1::2] == ["flow", "enc", "dcn", "res", "last", "total"]
    # another geometry: window = whole frame in y, partial in x; 2 frames
    lrs = T(synth.make_clip(9, 1, 2, 16, 40, fv_size=32)[0])
    fvs = torch.rand(1, 2, 3, 48, 48, generator=torch.Generator().manual_seed(1))
    m.print_timings = False
    got = m(lrs.to(dev()), fvs.to(dev()), warp_size=(128, 192))
    ref = ro.runtime_forward(orc.load_numpy_state(sd), lrs, fvs, (128, 192))
    assert tuple(got.shape) == (1, 2, 3, 128, 320) and maxdiff(got, ref) < 2e-4


# ------------------------------------------------------------------------------------------------ pre-packed operator variants
def test_packed_operator_variants_and_weight_updates(orc):
    """crfp_conv3x3_packed_f32 / crfp_dcnv2_g8_packed_f32 (weights packed by the caller) equal the one-call forms, and the
    per-operator wrappers see EVERY kind of weight update -- in place, and through ``.data`` the way the reference writes
    weights (``m.weight.data *= scale``, conv_identify, model/CRFP.py:359-370), which moves no version counter."""
    from crfp_amd import ops
    rs = np.random.RandomState(2)
    x = T(rs.standard_normal((1, 32, 20, 36)).astype(np.float32)).to(dev())
    w = T((rs.standard_normal((32, 32, 3, 3)) * 0.1).astype(np.float32)).to(dev())
    b = T(rs.standard_normal(32).astype(np.float32)).to(dev())
    ref = lambda: F.leaky_relu(F.conv2d(x.cpu(), w.cpu(), b.cpu(), padding=1), 0.1)   # noqa: E731
    a1 = ops.conv3x3(x, w, b, "lrelu")
    assert maxdiff(a1, ops.conv3x3_unpacked(x, w, b, "lrelu")) == 0.0
    pk = ops.pack_conv3x3(w, b)
    assert maxdiff(ops.conv3x3_packed(x, pk, "lrelu"), a1) == 0.0                  # caller-hoisted pack == per-call pack
    w.mul_(2.0)                                                                    # in-place update
    a2 = ops.conv3x3(x, w, b, "lrelu")
    assert maxdiff(a2, ref()) < 3e-5 and maxdiff(a2, a1) > 1e-3
    v = w._version
    w.data *= 0.25                                                                 # .data update: the version counter stays
    w.data[3] = 1.0
    assert w._version == v
    a3 = ops.conv3x3(x, w, b, "lrelu")
    assert maxdiff(a3, ref()) < 3e-5 and maxdiff(a3, a2) > 1e-3
    assert maxdiff(ops.conv3x3(x, w, None, "none"), F.conv2d(x.cpu(), w.cpu(), None, padding=1)) < 3e-5   # bias=None
    off = T(rs.uniform(-4, 4, (1, 144, 20, 36)).astype(np.float32)).to(dev())
    msk = T(rs.uniform(0, 1, (1, 72, 20, 36)).astype(np.float32)).to(dev())
    d1 = ops.dcnv2(x, off, msk, w, b, 3, 1, 1, 8)
    assert maxdiff(d1, orc.dcnv2(x.cpu(), off.cpu(), msk.cpu(), w.cpu(), b.cpu(), 8)) < 5e-5
    assert maxdiff(ops.dcnv2_g8_packed(x, off, msk, ops.pack_dcnv2_g8(w), b), d1) == 0.0
    w.data.zero_()
    assert maxdiff(ops.dcnv2(x, off, msk, w, b, 3, 1, 1, 8), b.cpu().view(1, 32, 1, 1).expand(1, 32, 20, 36)) < 1e-6


def test_module_sees_data_writes_after_invalidate_and_checked_mode_catches_stale_weights():
    """CRFP_DSV keeps one packed-weight image per engine, keyed by (address, version) of every parameter.  A write through
    ``.data`` moves neither: ``invalidate_packed()`` is the documented way to publish it, and CRFP_CHECK_PACKED=1 turns a
    forgotten one into an error instead of a silently stale result."""
    from crfp_amd import synth
    sd = synth.make_state_dict(7)
    m = _model(sd)
    lrs, fvs, mks = synth.make_clip(5, 1, 2, 16, 24, fv_size=48)
    d = dev()
    a = dict(lrs=T(lrs).to(d), fvs=T(fvs).to(d), mks=T(mks).to(d))
    ref = m(**a).clone()
    m.conv_last.weight.data *= 0.5
    m.invalidate_packed()
    out = m(**a).clone()
    assert maxdiff(out, ref) > 1e-4
    m.conv_last.weight.mul_(2.0)                      # in place on the parameter: picked up by itself
    assert maxdiff(m(**a), ref) < 1e-6
    os.environ["CRFP_CHECK_PACKED"] = "1"
    try:
        m.invalidate_packed()
        m(**a)                                        # packs and records the checksum
        m.conv_last.bias.data += 1.0
        with pytest.raises(RuntimeError, match="invalidate_packed"):
            m(**a)
        m.invalidate_packed()
        assert maxdiff(m(**a), ref) > 0.5
    finally:
        os.environ.pop("CRFP_CHECK_PACKED")


@pytest.mark.parametrize("case", ["cat_resid", "slice", "shuffle2", "shuffle4", "unshuffle4"])
def test_conv3x3_ex_operator_vs_torch(case):
    """crfp_conv3x3_ex_f32 (the conv operator with everything SURVEY 8b lists: two inputs = fused cat, residual, channel-slice store,
    pixel_shuffle store, pixel_unshuffle load) against the ATen ops the reference composes (model/CRFP.py:28-50,184-193)."""
    from crfp_amd import ops
    g = torch.Generator().manual_seed(5)
    d = dev()
    R = lambda *s: (torch.rand(*s, generator=g) - 0.5)
    n, h, w = 2, 19, 37
    if case == "cat_resid":
        x, x2 = R(n, 24, h, w), R(n, 10, h, w)
        wt, b, res = R(20, 34, 3, 3) * 0.2, R(20), R(n, 20, h, w)
        ref = F.leaky_relu(F.conv2d(torch.cat([x, x2], 1), wt, b, padding=1), 0.1) * 0.5 + res
        got = ops.conv3x3_ex(x.to(d), wt.to(d), b.to(d), x2=x2.to(d), residual=res.to(d), act="lrelu", post_scale=0.5)
    elif case == "slice":
        x = R(n, 12, h, w)
        wt, b = R(6, 12, 3, 3) * 0.2, R(6)
        base = R(n, 16, h, w)
        ref = base.clone(); ref[:, 5:11] = F.relu(F.conv2d(x, wt, b, padding=1))
        got = ops.conv3x3_ex(x.to(d), wt.to(d), b.to(d), act="relu", out=base.to(d).clone(), out_c0=5)
    elif case in ("shuffle2", "shuffle4"):
        r = int(case[-1])
        x = R(n, 16, h, w)
        wt, b = R(3 * r * r, 16, 3, 3) * 0.2, R(3 * r * r)
        ref = F.pixel_shuffle(F.conv2d(x, wt, b, padding=1), r)
        got = ops.conv3x3_ex(x.to(d), wt.to(d), b.to(d), shuffle=r)
    else:
        x = R(n, 2, 4 * h, 4 * w)
        wt, b = R(9, 32, 3, 3) * 0.2, R(9)
        ref = F.conv2d(F.pixel_unshuffle(x, 4), wt, b, padding=1)
        got = ops.conv3x3_ex(x.to(d), wt.to(d), b.to(d), unshuffle=4)
    assert tuple(got.shape) == tuple(ref.shape)
    assert maxdiff(got, ref) < 3e-5


def test_conv3x3_ex_rejects_unsupported_combinations():
    from crfp_amd import ops
    d = dev()
    x = torch.zeros(1, 8, 8, 8, device=d)
    with pytest.raises(RuntimeError):
        ops.conv3x3_ex(x, torch.zeros(6, 8, 3, 3, device=d), shuffle=2)                 # cout not a multiple of r^2
    with pytest.raises(RuntimeError):
        ops.conv3x3_ex(x, torch.zeros(8, 8, 3, 3, device=d), shuffle=2, act="tanh")    # transcendental activation with a shuffle store
    with pytest.raises(RuntimeError):
        ops.conv3x3_ex(x, torch.zeros(8, 8, 3, 3, device=d), unshuffle=3)               # only r = 4


def test_dcnv2_shared_offsets_operator(orc):
    """crfp_dcnv2_shared_f32 (one (dy, dx) and mask per pixel for all 9 taps, SURVEY 8b's offset_mask_shared_across_taps) equals the
    general DCNv2 on the 9x-tiled tensors the reference builds (model/CRFP.py:341-350): against the oracle and against our own
    general operator."""
    from crfp_amd import ops
    g = torch.Generator().manual_seed(9)
    n, h, w = 2, 21, 45
    x = torch.rand(n, 4, h, w, generator=g) - 0.5
    off = (torch.rand(n, 2, h, w, generator=g) - 0.5) * 9.0
    mk = torch.rand(n, 1, h, w, generator=g)
    wt = (torch.rand(4, 4, 3, 3, generator=g) - 0.5) * 0.5
    b = torch.rand(4, generator=g) - 0.5
    ref = orc.dcnv2(x, off.repeat(1, 9, 1, 1), mk.repeat(1, 9, 1, 1), wt, b, 1)
    d = dev()
    got = ops.dcnv2_shared(x.to(d), off.to(d), mk.to(d), wt.to(d), b.to(d))
    gen = ops.dcnv2(x.to(d), off.repeat(1, 9, 1, 1).to(d), mk.repeat(1, 9, 1, 1).to(d), wt.to(d), b.to(d), deformable_groups=1)
    assert maxdiff(got, ref) < 3e-5 and maxdiff(gen, ref) < 3e-5
    with pytest.raises(RuntimeError):
        ops.dcnv2_shared(torch.zeros(1, 8, 8, 8, device=d), torch.zeros(1, 2, 8, 8, device=d), torch.zeros(1, 1, 8, 8, device=d),
                         torch.zeros(8, 8, 3, 3, device=d), torch.zeros(8, device=d))
