"""The one-frame-per-call forms of the CRFP_simple / CRFP wirings -- the reference's MRCF_simple_v13 / MRCF_simple_v15 (model/CRFP_test.py:
1184-1486, 1805-2113) -- on the GPU: against the reference's own streamed outputs (tests/golden/stream_ablation), against the clip engine of
the same wiring (bit for bit), and against themselves across the schedules that must not change a bit (lock-step sequences, resident inputs,
the ignored regional mask)."""
import ast

import numpy as np
import pytest
import torch

import golden_io

pytestmark = pytest.mark.gpu

T = torch.from_numpy
WIRINGS = [("MRCF_simple_v13", "CRFP_simple"), ("MRCF_simple_v15", "CRFP")]


@pytest.fixture(scope="module")
def golden():
    return golden_io.load("stream_ablation")


def _dev():
    return torch.device("cuda:0")


def _load(m, seed):
    from crfp_amd import synth
    sd = synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    return m.to(_dev()).eval()


def _models(stream_cls, clip_cls, y_only=False, seed=3, storage="f32"):
    """The stream model and the clip model of one wiring with the same weights."""
    from crfp_amd.model import CRFP
    s = _load(getattr(CRFP, stream_cls)(_dev(), mid_channels=32, y_only=y_only), seed)
    c = _load(getattr(CRFP, clip_cls)(_dev(), mid_channels=32, y_only=y_only), seed)
    s.storage = c.storage = storage
    return s, c


def _clip(seed, n, t, h=24, w=40, fv=96):
    from crfp_amd import synth
    return tuple(T(a).to(_dev()) for a in synth.make_clip(seed, n, t, h, w, fv_size=fv, sigma_t=10.0))


def _boxes(n, t, h, w, seed=5):
    rs = np.random.RandomState(seed)
    fgs = torch.zeros(n, t, 1, 8 * h, 8 * w, dtype=torch.bool)
    for b in range(n):
        for i in range(t):
            y0, x0 = rs.randint(0, 4 * h), rs.randint(0, 4 * w)
            fgs[b, i, 0, y0:y0 + 4 * h, x0:x0 + 4 * w] = True
    return fgs.to(_dev())


def _stream(m, lrs, fvs, mks, fgs=None, clear_at=()):
    outs = []
    for i in range(lrs.shape[1]):
        if i in clear_at:
            m.clear_states()
        outs.append(m(lrs[:, i:i + 1], fvs[:, i:i + 1], mks[:, i:i + 1], None if fgs is None else fgs[:, i:i + 1]).clone())
    return torch.cat(outs, dim=1)


def _golden_run(g, name, path):
    from crfp_amd import synth
    from crfp_amd.model import CRFP
    kw = dict(ast.literal_eval(str(g[f"{name}.kwargs"])))
    m = getattr(CRFP, str(g[f"{name}.class"]))(_dev(), **kw)
    table = {s.rsplit(":", 1)[0]: tuple(int(v) for v in s.rsplit(":", 1)[1].split(",")) for s in map(str, g[f"{name}.keys"])}
    sd = synth.make_state_dict_like(table, int(g["weights_seed"]))
    assert synth.state_dict_digest(sd) == str(g[f"{name}.weights_sha256"])
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(_dev()).eval()
    if path == "composed":
        m.has_engine = lambda: False     # the per-operator composition with the state carried between calls
    elif path == "f32":
        m.precision = "f32"
    h, w, t = int(g["h"]), int(g["w"]), int(g[f"{name}.t"])
    lrs, fvs, mks = (T(a).to(_dev()) for a in synth.make_clip(int(g[f"{name}.clip_seed"]), 1, t, h, w, fv_size=int(g["fv"]), sigma_t=10.0))
    fgs = T(g[f"{name}.fgs"]).to(_dev())
    outs = []
    for c, (a, b) in enumerate(g[f"{name}.calls"]):
        if c == int(g[f"{name}.clear_at"]):
            m.clear_states()
        outs.append(m(lrs[:, a:b], fvs[:, a:b], mks[:, a:b], fgs[:, a:b]))
    return m, torch.cat(outs, dim=1)


GOLDEN_RUNS = [(name, path) for name in ("v13_mid32", "v15_mid32", "v15_yonly") for path in ("engine", "f32", "composed")] + \
              [("v13_nohrdcn", "composed"), ("v15_noprop", "composed")]   # no one-call engine for these two: the composition is their path


@pytest.mark.parametrize("name,path", GOLDEN_RUNS)
def test_stream_matches_the_reference_golden(golden, name, path):
    """Within 2e-4 of the reference's streamed output (the tolerance of test_streaming_variant_golden): one frame per call, a two-frame call,
    clear_states() in the middle, a regional box per frame."""
    m, got = _golden_run(golden, name, path)
    assert m.has_engine() == (path != "composed")
    ref = T(golden[f"{name}.out"])
    assert got.shape == ref.shape
    assert float((got.cpu() - ref).abs().max()) < 2e-4
    if path != "composed":
        assert not m.engine().overflowed(stream=True)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("y_only", [False, True])
@pytest.mark.parametrize("stream_cls,clip_cls", WIRINGS)
def test_stream_equals_the_clip_engine(stream_cls, clip_cls, y_only, storage):
    """Streaming a clip one frame per call gives the clip engine's bits (the same kernels on the same buffer sets)."""
    s, c = _models(stream_cls, clip_cls, y_only, storage=storage)
    lrs, fvs, mks = _clip(31, 1, 5)
    with torch.no_grad():
        clip = c(lrs, fvs, mks)
        got = _stream(s, lrs, fvs, mks)
    assert type(s.engine()).__name__.endswith("StreamEngine")
    assert torch.isfinite(clip).all() and torch.equal(got, clip)
    # the recurrence is live: frame 4 of the stream is not its first-frame arithmetic
    s.clear_states()
    with torch.no_grad():
        alone = _stream(s, lrs[:, 4:], fvs[:, 4:], mks[:, 4:])
    assert float((alone[:, 0] - got[:, 4]).abs().max()) > 1e-3


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("stream_cls,clip_cls", WIRINGS)
def test_lockstep_sequences_equal_single_chains(stream_cls, clip_cls, storage):
    """n = 3 sequences in one call per frame == three one-sequence chains, bit for bit, across a clear_states()."""
    s, _ = _models(stream_cls, clip_cls, storage=storage)
    lrs, fvs, mks = _clip(32, 3, 6)
    with torch.no_grad():
        both = _stream(s, lrs, fvs, mks, clear_at=(3,))
        singles = [_stream(s, lrs[b:b + 1], fvs[b:b + 1], mks[b:b + 1], clear_at=(0, 3)) for b in range(3)]
    assert torch.isfinite(both).all()
    for b in range(3):
        assert torch.equal(both[b:b + 1], singles[b]), b


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("stream_cls,clip_cls", WIRINGS)
def test_resident_inputs_are_bit_identical(stream_cls, clip_cls, storage):
    """inputs_resident (CRFP_DSV_INPUTS_RESIDENT): the same bits as the plain call, across a clear_states(), on two streams and on one; n = 2 too."""
    s, _ = _models(stream_cls, clip_cls, storage=storage)
    lrs, fvs, mks = _clip(33, 2, 7)
    mks = mks.bool()
    torch.cuda.synchronize()   # the resident calls read the inputs on the library's side stream: they must be complete
    with torch.no_grad():
        base = _stream(s, lrs, fvs, mks, clear_at=(4,))
        s.clear_states()
        s.inputs_resident = True
        res = _stream(s, lrs, fvs, mks, clear_at=(4,))
        one = _stream(s, lrs[:1], fvs[:1], mks[:1], clear_at=(0, 4))
        s.engine().single_stream = True
        single = _stream(s, lrs[:1], fvs[:1], mks[:1], clear_at=(0, 4))
    assert torch.isfinite(base).all() and torch.equal(base, res)
    assert torch.equal(one, base[:1]) and torch.equal(single, base[:1])


@pytest.mark.parametrize("stream_cls,clip_cls", WIRINGS)
def test_regional_mask_changes_nothing(stream_cls, clip_cls):
    """v13 / v15 never read fg_lv0 (model/CRFP_test.py:1357-1359, 1978-1980): a regional box leaves every output bit as it is, for n = 1 and
    n = 2 (where CRFP_DSV's stream refuses `fg`), on the engine and on the composition."""
    s, _ = _models(stream_cls, clip_cls)
    lrs, fvs, mks = _clip(34, 2, 4)
    fgs = _boxes(2, 4, 24, 40)
    with torch.no_grad():
        plain = _stream(s, lrs, fvs, mks, clear_at=(0,))
        boxed = _stream(s, lrs, fvs, mks, fgs, clear_at=(0,))
        one = _stream(s, lrs[:1], fvs[:1], mks[:1], fgs[:1], clear_at=(0,))
        s.has_engine = lambda: False
        comp_plain = _stream(s, lrs, fvs, mks, clear_at=(0,))
        comp_boxed = _stream(s, lrs, fvs, mks, fgs, clear_at=(0,))
    assert torch.equal(plain, boxed) and torch.equal(one, plain[:1])
    assert torch.equal(comp_plain, comp_boxed)


@pytest.mark.parametrize("stream_cls,clip_cls", WIRINGS)
def test_full_size_stream_against_the_composition(stream_cls, clip_cls):
    """180 x 320 -> 1440 x 2560, 12 calls: no range-guard overflow, within 2e-4 * max(1, |ref|) of the composed stream."""
    s, _ = _models(stream_cls, clip_cls, seed=9)
    lrs, fvs, mks = _clip(35, 1, 12, 180, 320, 384)
    with torch.no_grad():
        got = _stream(s, lrs, fvs, mks)
        assert not s.engine().overflowed(stream=True)
        s.clear_states()
        s.has_engine = lambda: False
        ref = _stream(s, lrs, fvs, mks)
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max()) < 2e-4 * max(1.0, float(ref.abs().max()))


def test_stream_engine_refuses_what_the_dsv_stream_refuses():
    from crfp_amd import _lib
    s, _ = _models("MRCF_simple_v15", "CRFP")
    lrs, fvs, mks = _clip(36, 1, 2)
    eng = s.engine()
    eng.on_overflow = "fallback"
    with pytest.raises(NotImplementedError):
        eng.stream_frame(lrs[0, 0], fvs[0, 0], mks[0, 0])
    eng.on_overflow = "poison"
    # a workspace sized for CRFP_DSV is too small for this wiring's stream
    h, w = 24, 40
    nb = _lib.lib().crfp_dsv_batch_workspace_bytes(1, 1, h, w)
    assert nb < _lib.lib().crfp_dense_batch_workspace_bytes(1, 1, h, w)
    ws = torch.zeros(nb, dtype=torch.uint8, device=_dev())
    out = torch.empty(3, 8 * h, 8 * w, device=_dev())
    rc = _lib.lib().crfp_dense_stream_batch(eng.packed.data_ptr(), 0, lrs[0, 0].data_ptr(), None, fvs[0, 0].data_ptr(),
                                            mks[0, 0].to(torch.uint8).data_ptr(), None, out.data_ptr(), 1, 1, h, w, ws.data_ptr(), nb,
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == -2   # CRFP_E_WORKSPACE


def test_gaze_rig_runs_the_v15_stream():
    """crfp_amd.gaze.run_gaze_video (test_video.py's loop: one frame per call with a regional mask) with MRCF_simple_v15: finite region metrics."""
    import torch.nn.functional as F
    from crfp_amd import gaze, synth
    from crfp_amd.model import CRFP
    h, w, N, fv = 16, 24, 5, 32
    lr = T(synth.make_clip(21, 1, N, h, w, fv_size=fv)[0][0]).to(_dev())
    gt = torch.clamp(F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False), 0, 1)
    m = _load(CRFP.MRCF_simple_v15(_dev(), mid_channels=32), 4)
    res = gaze.run_gaze_video(m, lr, gt, sigma=6.0, fv_size=fv, seed=11, fv_start=1, regional_dcn=True, rg=96)
    assert res["frames"] == N
    for r in ("whole", "fovea", "outskirt", "past"):
        assert np.isfinite(res[f"psnr_{r}"]) and np.isfinite(res[f"ssim_{r}"]), r
