"""The one-frame-per-call form of the CRFP_DSV_CRA wiring -- the reference's MRCF_simple_v18_cra (model/CRFP_test.py:2480-2861) -- on the GPU:
against the reference's own streamed outputs (tests/golden/stream_cra), against the clip engine of the wiring (bit for bit), and against
itself across everything that must not change a bit: lock-step sequences, several frames per call, the four schedules of
crfp_cra_stream_batch (one or two streams, resident inputs or not) and the regional mask the model never reads."""
import ast

import numpy as np
import pytest
import torch

import golden_io

pytestmark = pytest.mark.gpu

T = torch.from_numpy
STREAM, CLIP = "MRCF_simple_v18_cra", "CRFP_DSV_CRA"


@pytest.fixture(scope="module")
def golden():
    return golden_io.load("stream_cra")


def _dev():
    return torch.device("cuda:0")


def _load(m, seed):
    from crfp_amd import synth
    sd = synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    return m.to(_dev()).eval()


def _model(cls=STREAM, y_only=False, seed=3, storage="f32"):
    from crfp_amd.model import CRFP
    m = _load(getattr(CRFP, cls)(_dev(), mid_channels=32, y_only=y_only), seed)
    m.storage = storage
    return m


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
    with torch.no_grad():
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


@pytest.mark.parametrize("path", ["engine", "f32", "composed"])
@pytest.mark.parametrize("name", ["cra_mid32", "cra_yonly", "cra_mid16"])
def test_stream_matches_the_reference_golden(golden, name, path):
    """Within 2e-4 of the reference's streamed output (the tolerance of the v13 / v15 / v18 stream goldens): one frame per call, a two-frame
    call, clear_states() in the middle, a regional box per frame; mid_channels 16 runs embedded in the 32-channel schedule."""
    m, got = _golden_run(golden, name, path)
    assert m.has_engine() and type(m.engine()).__name__ == "CRAStreamEngine" if path != "composed" else not m.has_engine()
    ref = T(golden[f"{name}.out"])
    assert got.shape == ref.shape
    d = float((got.cpu() - ref).abs().max())
    print(f"{name} {path}: max |stream - reference| = {d:.3e}")
    assert d < 2e-4
    if path != "composed":
        assert not m.engine().overflowed(stream=True)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("y_only", [False, True])
@pytest.mark.parametrize("h,w,t", [(24, 40, 5), (33, 47, 4)])
def test_stream_equals_the_clip_engine(h, w, t, y_only, storage):
    """Streaming a clip one frame per call gives crfp_cra_forward_batch's bits (the same kernels on the same buffer sets); 33 x 47 has ragged
    tiles at every resolution, t >= 4 reuses both parity sets of the clip schedule."""
    s, c = _model(STREAM, y_only, storage=storage), _model(CLIP, y_only, storage=storage)
    lrs, fvs, mks = _clip(41, 1, t, h, w)
    with torch.no_grad():
        clip = c(lrs, fvs, mks)
    got = _stream(s, lrs, fvs, mks)
    assert type(s.engine()).__name__ == "CRAStreamEngine" and type(c.engine()).__name__ == "CRAEngine" and s.engine().storage == storage
    assert clip.shape == (1, t, 1 if y_only else 3, 8 * h, 8 * w)
    assert torch.isfinite(clip).all() and torch.equal(got, clip)
    # the recurrence is live: the last frame of the stream is not its first-frame arithmetic
    s.clear_states()
    alone = _stream(s, lrs[:, t - 1:], fvs[:, t - 1:], mks[:, t - 1:])
    assert float((alone[:, 0] - got[:, t - 1]).abs().max()) > 1e-3


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_lockstep_sequences_and_multi_frame_calls(storage):
    """n = 3 sequences in one call per frame == three one-sequence chains; one call on four frames == four one-frame calls; clear_states()
    in the middle restarts every sequence.  Bit for bit."""
    s = _model(storage=storage)
    lrs, fvs, mks = _clip(42, 3, 6)
    both = _stream(s, lrs, fvs, mks, clear_at=(3,))
    singles = [_stream(s, lrs[b:b + 1], fvs[b:b + 1], mks[b:b + 1], clear_at=(0, 3)) for b in range(3)]
    assert torch.isfinite(both).all()
    for b in range(3):
        assert torch.equal(both[b:b + 1], singles[b]), b
    # after the clear, frame 3 is first-frame arithmetic again: the same bits as a fresh sequence started there
    s.clear_states()
    fresh = _stream(s, lrs[:, 3:], fvs[:, 3:], mks[:, 3:])
    assert torch.equal(fresh, both[:, 3:])
    s.clear_states()
    with torch.no_grad():
        four = s(lrs[:, 0:4], fvs[:, 0:4], mks[:, 0:4]).clone()
    s.clear_states()
    assert torch.equal(four, _stream(s, lrs[:, 0:4], fvs[:, 0:4], mks[:, 0:4]))
    assert torch.equal(four[:, :3], both[:, :3])


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 2])
def test_the_four_schedules_give_the_same_bits(n, storage):
    """inputs_resident (CRFP_DSV_INPUTS_RESIDENT) x single_stream (CRFP_DSV_SINGLE_STREAM): seven calls with a clear_states() in front of the
    fifth, so calls 2 and 3 start early behind a chained call, call 4 restarts on one stream and call 6 starts early again."""
    s = _model(storage=storage)
    lrs, fvs, mks = _clip(43, n, 7)
    mks = mks.bool()
    torch.cuda.synchronize()   # the resident calls read the inputs on the library's side stream: they must be complete
    runs = {}
    for resident in (False, True):
        for single in (False, True):
            s.clear_states()
            s.inputs_resident = resident
            s.engine().single_stream = single
            runs[resident, single] = _stream(s, lrs, fvs, mks, clear_at=(4,))
            torch.cuda.synchronize()
    base = runs[False, False]
    assert torch.isfinite(base).all() and float((base[:, 3] - base[:, 4]).abs().max()) > 1e-3
    for key, got in runs.items():
        assert torch.equal(got, base), key


def test_regional_mask_changes_nothing():
    """MRCF_simple_v18_cra.forward takes `fgs` and never reads it: a regional box leaves every output bit as it is, for n = 1 and n = 2
    (where CRFP_DSV's stream refuses `fg`), on the engine and on the composition."""
    s = _model()
    lrs, fvs, mks = _clip(44, 2, 4)
    fgs = _boxes(2, 4, 24, 40)
    plain = _stream(s, lrs, fvs, mks, clear_at=(0,))
    boxed = _stream(s, lrs, fvs, mks, fgs, clear_at=(0,))
    one = _stream(s, lrs[:1], fvs[:1], mks[:1], fgs[:1], clear_at=(0,))
    s.has_engine = lambda: False
    comp_plain = _stream(s, lrs, fvs, mks, clear_at=(0,))
    comp_boxed = _stream(s, lrs, fvs, mks, fgs, clear_at=(0,))
    comp_one = _stream(s, lrs[:1], fvs[:1], mks[:1], fgs[:1], clear_at=(0,))
    assert torch.isfinite(plain).all() and torch.equal(plain, boxed) and torch.equal(one, plain[:1])
    assert torch.equal(comp_plain, comp_boxed) and torch.equal(comp_one, comp_plain[:1])
    assert float((plain - comp_plain).abs().max()) < 2e-4 * max(1.0, float(comp_plain.abs().max()))


def test_full_size_stream_against_the_composition():
    """180 x 320 -> 1440 x 2560, 6 calls: finite, no range-guard overflow, within 2e-4 * max(1, |ref|) of the composed stream."""
    s = _model(seed=9)
    lrs, fvs, mks = _clip(45, 1, 6, 180, 320, 384)
    got = _stream(s, lrs, fvs, mks)
    assert not s.engine().overflowed(stream=True)
    s.clear_states()
    s.has_engine = lambda: False
    ref = _stream(s, lrs, fvs, mks)
    assert torch.isfinite(got).all()
    d, bound = float((got - ref).abs().max()), 2e-4 * max(1.0, float(ref.abs().max()))
    print(f"full size: max |engine stream - composed stream| = {d:.3e} (bound {bound:.3e})")
    assert d < bound


def test_stream_refuses_what_the_dsv_stream_refuses():
    """Argument checks of the handle and of the two entry points: none of them launches anything."""
    from crfp_amd import _lib
    L = _lib.lib()
    s = _model()
    lrs, fvs, mks = _clip(46, 1, 2)
    eng = s.engine()
    eng.on_overflow = "fallback"
    with pytest.raises(NotImplementedError):
        eng.stream_frame(lrs[0, 0], fvs[0, 0], mks[0, 0])
    eng.on_overflow = "poison"
    h, w = 24, 40
    mk8 = mks[0, 0].to(torch.uint8)
    out = torch.empty(3, 8 * h, 8 * w, device=_dev())
    stream = torch.cuda.current_stream().cuda_stream

    def call(fn, packed, flags, n, ws):
        return fn(packed.data_ptr(), flags, lrs[0, 0].data_ptr(), None, fvs[0, 0].data_ptr(), mk8.data_ptr(), None, out.data_ptr(), 1, n, h, w,
                  ws.data_ptr(), ws.numel(), stream)

    # a workspace sized for CRFP_DSV is too small for this wiring's stream
    nb, need = L.crfp_dsv_batch_workspace_bytes(1, 1, h, w), L.crfp_cra_batch_workspace_bytes(1, 1, h, w)
    assert 0 < nb < need
    small, full = torch.zeros(nb, dtype=torch.uint8, device=_dev()), torch.zeros(need, dtype=torch.uint8, device=_dev())
    assert call(L.crfp_cra_stream_batch, eng.packed, 0, 1, small) == -2          # CRFP_E_WORKSPACE
    assert call(L.crfp_cra_stream_batch, eng.packed, 0, 33, full) == -3          # CRFP_E_UNSUPPORTED: n <= 32
    assert b"32" in L.crfp_last_error_string()
    assert call(L.crfp_cra_stream_batch, eng.packed, 0, 0, full) == -1           # CRFP_E_BADARG
    # strict fp32 belongs to the fp32 entry point
    s.storage = "bf16"
    eng16 = s.engine()
    need16 = L.crfp_cra_batch_workspace_bytes_bf16(1, 1, h, w)
    full16 = torch.zeros(need16, dtype=torch.uint8, device=_dev())
    assert eng16.storage == "bf16" and call(L.crfp_cra_stream_batch_bf16, eng16.packed, _lib.DSV_STRICT_F32, 1, full16) == -3
    assert b"STRICT_F32" in L.crfp_last_error_string()
    with pytest.raises(ValueError):
        type(eng16)(s.state_dict(), _dev(), storage="bf16", precision="f32")
    # the clip model and its handle keep refusing to stream
    c = _model(CLIP)
    with pytest.raises(NotImplementedError):
        c.forward_stream(lrs, fvs, mks)
    with pytest.raises(NotImplementedError, match="CRFP_DSV_CRA"):
        c.engine().stream_frame(lrs[0, 0], fvs[0, 0], mks[0, 0])


def test_gaze_rig_runs_the_cra_stream():
    """crfp_amd.gaze.run_gaze_video (test_video.py's loop: one frame per call with a regional mask) with MRCF_simple_v18_cra, 8 frames at
    24 x 40: finite region metrics, and the fused metrics table gives the per-region calls' numbers (1e-4 dB / 2e-6 SSIM, the bound of
    test_gaze_rig_fused_metrics_equal_the_per_region_calls)."""
    import torch.nn.functional as F
    from crfp_amd import gaze, synth
    h, w, N, fv = 24, 40, 8, 48
    lr = T(synth.make_clip(21, 1, N, h, w, fv_size=fv)[0][0]).to(_dev())
    rs = np.random.RandomState(4)
    gt = torch.clamp(F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False) +
                     T(rs.normal(0, 0.02, (N, 3, 8 * h, 8 * w)).astype(np.float32)).to(_dev()), 0, 1)
    m = _model(seed=4)
    run = lambda fused: gaze.run_gaze_video(m, lr, gt, sigma=6.0, fv_size=fv, seed=11, fv_start=1, regional_dcn=True, rg=96,   # noqa: E731
                                            fused_metrics=fused)
    ref, got = run(False), run(True)
    assert ref["frames"] == got["frames"] == N and got["trajectory"] == ref["trajectory"]
    for r in ("whole", "fovea", "outskirt", "past"):
        assert np.isfinite(ref[f"psnr_{r}"]) and np.isfinite(ref[f"ssim_{r}"]), r
        assert len(got["per_frame"][r]) == len(ref["per_frame"][r]) == (N - 1 if r == "past" else N), r
        assert abs(got[f"psnr_{r}"] - ref[f"psnr_{r}"]) < 1e-4 and abs(got[f"ssim_{r}"] - ref[f"ssim_{r}"]) < 2e-6, r
