"""CPU: the oracle's restatement of the other three clip wirings (``cra_frame`` / ``ablation_frame`` / ``WiringConfig`` / the generalised
``StreamOracle``, oracle/crfp_oracle.py) pinned to the reference's goldens, and the stage tables of tests/helpers/wiring_stage_cases.py against
the oracle alone.

* fp32 oracle vs tests/golden/dsv_flags cases cra_mid32, simple_mid32, dense_mid32, cra_mid16_yonly (the narrow case natively at mid = 16) and,
  with state carried from call to call, vs the streamed goldens stream_ablation (v13_mid32, v15_mid32, v15_yonly) and stream_cra (cra_mid32,
  cra_yonly): <= 2e-5, the project's oracle-vs-golden bound (weights ``make_state_dict_like``, clips ``make_clip``, as tests/test_flags.py and
  the streaming GPU tests build them);
* every tap a table names exists with the shape the wiring's ``debug_fetch`` reports; every fetchable buffer of the wiring's Layout is a row,
  listed as never written, or carries no model tensor;
* fp32 oracle vs its float64 run with the same injected flow <= 0.25 of the stage bound for every tap the tables name, on frames 1 and 2 of the
  two steered clips (and cra's L-mask variant); the measured shares stand in the helper's docstring;
* the masks: the stock fovea masks resample to {0, 1/2, 1}, the L-shaped variant to all of {0, 1/4, 1/2, 3/4, 1};
* guards: dense with its third source zeroed is simple's function of the same weights; a cra oracle run with the nearest-pixel x0.25 mask is
  far outside the bound on the `res<k>` taps; a stale frame or a stale level cannot pass for a row."""
import ast
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import golden_io
from helpers import motion_cases as mc
from helpers import wiring_stage_cases as wc

T = torch.from_numpy
CLIPS = [("large", 3, 33, 47), ("moderate", 3, 24, 40)]
CASES = [(w, "stock") for w in wc.WIRINGS] + [("cra", "L")]
GOLDEN_BOUND = 2e-5
STREAM_CLASS = {"MRCF_simple_v13": "simple", "MRCF_simple_v15": "dense", "MRCF_simple_v18_cra": "cra"}


@pytest.fixture(scope="module")
def orc():
    from oracle import crfp_oracle
    return crfp_oracle


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


def _table(g, name):
    return {s.rsplit(":", 1)[0]: tuple(int(v) for v in s.rsplit(":", 1)[1].split(",")) for s in map(str, g[f"{name}.keys"])}


def _weights(orc, g, name):
    from crfp_amd import synth
    sd = synth.make_state_dict_like(_table(g, name), int(g["weights_seed"]))
    assert synth.state_dict_digest(sd) == str(g[f"{name}.weights_sha256"])
    return orc.load_numpy_state(sd)


# ----------------------------------------------------------------------------- the oracle against the reference's goldens
@pytest.mark.parametrize("name", ["cra_mid32", "simple_mid32", "dense_mid32", "cra_mid16_yonly"])
def test_clip_oracle_matches_the_reference_golden(orc, name):
    from crfp_amd import synth
    g = golden_io.load("dsv_flags")
    kw = dict(ast.literal_eval(str(g[f"{name}.kwargs"])))
    cfg = orc.WiringConfig(name.split("_")[0], kw.get("mid_channels", 16), kw.get("y_only", False))
    assert (cfg.mid, cfg.y_only) == ((16, True) if name == "cra_mid16_yonly" else (32, False))
    lrs, fvs, mks = (T(a) for a in synth.make_clip(int(g[f"{name}.clip_seed"]), 1, int(g[f"{name}.t"]), int(g["h"]), int(g["w"]), fv_size=int(g["fv"])))
    out = orc.wiring_forward(_weights(orc, g, name), lrs, fvs, mks, cfg)
    ref = T(g[f"{name}.out"])
    assert out.shape == ref.shape
    d = float((out - ref).abs().max())
    print(f"{name}: max |oracle - reference| = {d:.3e}")
    assert d <= GOLDEN_BOUND


@pytest.mark.parametrize("gname,name", [("stream_ablation", "v13_mid32"), ("stream_ablation", "v15_mid32"), ("stream_ablation", "v15_yonly"),
                                        ("stream_cra", "cra_mid32"), ("stream_cra", "cra_yonly")])
def test_stream_oracle_carries_the_state_like_the_reference(orc, gname, name):
    from crfp_amd import synth
    g = golden_io.load(gname)
    kw = dict(ast.literal_eval(str(g[f"{name}.kwargs"])))
    cfg = orc.WiringConfig(STREAM_CLASS[str(g[f"{name}.class"])], kw.get("mid_channels", 16), kw.get("y_only", False))
    t, h, w = int(g[f"{name}.t"]), int(g["h"]), int(g["w"])
    lrs, fvs, mks = (T(a) for a in synth.make_clip(int(g[f"{name}.clip_seed"]), 1, t, h, w, fv_size=int(g["fv"]), sigma_t=10.0))
    fgs = T(g[f"{name}.fgs"])
    so = orc.StreamOracle(_weights(orc, g, name), cfg)
    outs = []
    for c, (a, b) in enumerate(g[f"{name}.calls"]):
        if c == int(g[f"{name}.clear_at"]):
            so.clear_states()
        outs.append(so(lrs[:, a:b], fvs[:, a:b], mks[:, a:b], fgs[:, a:b]))       # these three models never read fgs
    out, ref = torch.cat(outs, 1), T(g[f"{name}.out"])
    assert out.shape == ref.shape
    d = float((out - ref).abs().max())
    print(f"{gname} {name}: max |stream oracle - reference| = {d:.3e}")
    assert d <= GOLDEN_BOUND
    # and the carry is live: a sequence restarted at every call is a different function
    cold = orc.wiring_forward(so.P, lrs[:, 1:2], fvs[:, 1:2], mks[:, 1:2], cfg)
    assert float((cold[:, 0] - ref[:, 1]).abs().max()) > 100 * GOLDEN_BOUND


def test_dsv_config_through_the_generalised_stream_oracle_is_unchanged(orc):
    """StreamOracle with a DSVConfig still runs dsv_frame (fgs included), and WiringConfig("dsv") is DSVConfig."""
    a, b = orc.DSVConfig(), orc.WiringConfig("dsv")
    assert (a.mid, a.last, a.carry, a.prop, a.dg) == (b.mid, b.last, b.carry, b.prop, b.dg) and orc.frame_fn(a) is orc.dsv_frame is orc.frame_fn(b)
    s = orc.WiringConfig("simple", 16)
    assert (s.carry, s.prop, s.last, s.dense, s.abl, s.cra) == (0, 16, 2, False, True, False) and orc.WiringConfig("dense").dense
    assert orc.frame_fn(orc.WiringConfig("cra")) is orc.cra_frame and orc.frame_fn(s) is orc.ablation_frame
    with pytest.raises(ValueError):
        orc.WiringConfig("v13")


# ----------------------------------------------------------------------------- the stage tables
@functools.lru_cache(maxsize=None)
def _taps(wiring, mask, regime, t, h, w, double, **kw):
    """Frame-by-frame taps with the fp32 oracle's own flow injected into both precisions."""
    from oracle import crfp_oracle
    sd, lrs, fvs, mks = wc.case(wiring, regime, t, h, w, mask=mask)
    flows = crfp_oracle.compute_flow(crfp_oracle.load_numpy_state(sd), T(lrs))
    return wc.oracle_taps(crfp_oracle, wiring, sd, lrs, fvs, mks, flows=flows, double=double, **kw)


def _fetch_shape(wiring, name, t, h, w, storage="f32"):
    from crfp_amd import _lib
    fn = getattr(_lib.lib(), _lib.symbol(wiring, "debug_fetch", storage))
    dummy = C.create_string_buffer(8)
    c, hh, ww = C.c_int(), C.c_int(), C.c_int()
    n = fn(name.encode(), t, h, w, C.cast(dummy, C.c_void_p), None, C.byref(c), C.byref(hh), C.byref(ww), None)
    return (n, c.value, hh.value, ww.value) if n >= 0 else None


@pytest.mark.parametrize("wiring", wc.WIRINGS)
def test_tables_are_well_formed(wiring):
    rows = wc.ROWS[wiring]
    keys = [r.key for r in rows]
    assert len(set(keys)) == len(keys)
    w = lambda b, s, t=3: set(wc.written_names(wiring, b, s, t))      # noqa: E731
    for build in wc.BUILDS:
        prod, unf = w(build, "product"), w(build, "unfused")
        assert unf - prod == {"dcn.fa", "res.y1", "offmask"} | ({"om3"} if build == "f32" else set()), (build, unf - prod)
        assert prod <= unf
        assert {"poff", "state_hr"} <= {r.key for r in wc.rows_for(wiring, build, "product") if r.state}
        assert not set(wc.NEVER_WRITTEN[wiring] + wc.CLEARED[wiring]) & unf
    if wiring == "cra":
        assert {"cra.s1", "cra.a", "cra.b", "cra.y", "cra.fused", "cra.lv0", "cra.lv0.1", "cra.lv2", "carry", "carryw"} <= w("f32", "product")
        assert [r.gated for r in rows if r.key in ("xin8", "enc_hr0", "cra.s1", "x_hr")] == [0, 0, 0, 1]
        assert "res3.z0" not in w("bf16", "product") and "res3.z0" not in w("f32", "product")
    else:
        assert not {"carry", "carryw"} & set(keys) and wc.NEVER_WRITTEN[wiring] == ("carryw",) and wc.CLEARED[wiring] == ("carry",)
        assert ("res3.z0" in w("bf16", "product")) == ("res3.z1" in w("bf16", "product")) == (wiring == "dense")
        assert "res3.z0" not in w("f32", "product") and "res3.z0" not in w("f32", "unfused")
        assert [r.gated for r in rows if r.key in ("xin8", "enc_hr0", "x_hr")] == [3, 2, 1]
    assert "flow2" not in w("f32", "product", 2) and "flow2.1" in w("f32", "product", 2) and "flow2" in w("f32", "product", 3)
    assert wc.SCHEDULES["unfused"] == {"CRFP_DCN_FUSED": "0", "CRFP_CONV_PAIR": "0"} and wc.SCHEDULES["product"] == {}


@pytest.mark.parametrize("storage", wc.BUILDS)
@pytest.mark.parametrize("wiring", wc.WIRINGS)
def test_every_layout_buffer_is_a_row_or_listed(wiring, storage, t=3, h=33, w=47):
    names = wc.fetch_names(wiring, t)
    layout = ["status", "state_hr", "carry", "flow_lr", "lr_q4", "enc_lr0", "x_lr"] + ["fnet." + n for n, _ in wc.sc._FNET] + ["fnet.g1"]
    for p in ("", ".1"):
        layout += [b + p for b in ("xin8", "enc_hr0", "x_hr", "prop0", "flow2", "flow8", "gate")]
    layout += ["prop_a", "prop_b", "prev2", "prev2w", "prevhrw", "carryw", "dcn.fa", "dcn.fb", "offfeat0", "offfeat1", "offfeat2", "offmask", "aligned",
               "res.y0", "res.y1", "up", "poff", "dcn3.g0", "dcn3.g1", "dcn3.g2", "om3", "aligned3", "res3.z0", "res3.z1", "feat"]
    cra = ["cra.s1", "cra.a", "cra.b", "cra.y", "cra.fused"] + [f"cra.lv{k}{p}" for k in range(3) for p in ("", ".1")]
    for n in layout + (cra if wiring == "cra" else []):
        assert _fetch_shape(wiring, n, t, h, w, storage) is not None, n
        assert (n in names) != (n in wc.NOT_MODEL), n
    assert set(names) <= set(layout + cra)
    for n in ([] if wiring == "cra" else cra) + ["fg2", "no_such_buffer"]:
        assert _fetch_shape(wiring, n, t, h, w, storage) is None, n
    # the layouts differ where the issue says: 32-channel prop*, 128-channel upsample
    for n in ("prop0", "prop0.1", "prop_a", "prop_b"):
        assert _fetch_shape(wiring, n, t, h, w, storage)[1] == (24 if wiring == "cra" else 32), n
    assert _fetch_shape("dsv", "prop_a", t, h, w, storage)[1] == 24 and _fetch_shape("dsv", "cra.s1", t, h, w, storage) is None


@pytest.mark.parametrize("wiring,mask", CASES)
@pytest.mark.parametrize("regime,t,h,w", [("large", 2, 33, 47), ("moderate", 3, 24, 40)])
def test_taps_exist_with_the_fetched_shapes(wiring, mask, regime, t, h, w):
    per = _taps(wiring, mask, regime, 3, h, w, False)[:t]
    for r in wc.ROWS[wiring]:
        for name, idx, frame in wc.slots(r, t):
            assert r.tap[0] in per[frame], (r.key, frame)
            tap = wc.tap_of(per[frame], r.tap)
            n, c, hh, ww = _fetch_shape(wiring, name, t, h, w)
            assert 0 <= idx < n, (r.key, name, idx, n)
            if name.startswith("flow2") or name.startswith("flow8"):
                assert c == 2 and tuple(tap.shape) == (1, hh, ww, 2), (r.key, tuple(tap.shape))
                continue
            got_c = len(range(c)[r.sel]) if isinstance(r.sel, slice) else (len(r.sel) if r.sel is not None else c)
            assert tuple(tap.shape) == (1, got_c, hh, ww), (r.key, name, tuple(tap.shape), (got_c, hh, ww))
            if r.other is not None:
                assert tuple(wc.tap_of(per[frame], r.other).shape) == tuple(tap.shape), r.key


@pytest.mark.parametrize("wiring,mask", CASES)
@pytest.mark.parametrize("regime,t,h,w", CLIPS)
def test_bound_is_safe_on_the_reference_alone(wiring, mask, regime, t, h, w):
    p32, p64 = _taps(wiring, mask, regime, t, h, w, False), _taps(wiring, mask, regime, t, h, w, True)
    mc.assert_regime(mc.flow_stats(torch.cat([p32[i]["flow_lr"] for i in (1, 2)]), h, w), regime)
    shares = {}
    for r in wc.ROWS[wiring]:
        for frame in (1, 2):
            a, b = wc.tap_of(p32[frame], r.tap).double(), wc.tap_of(p64[frame], r.tap)
            shares[r.key] = max(shares.get(r.key, 0.0), float((a - b).abs().max()) / wc.bound_of(wiring, r, b))
    d_out = max(float((p32[i]["out"].double() - p64[i]["out"]).abs().max()) for i in range(t))
    top = sorted(shares.items(), key=lambda kv: -kv[1])[:8]
    print(f"SHARES {wiring}/{mask} {regime}: out fp32 vs float64 {d_out:.2e}; " + "  ".join(f"{k} {v:.3f}" for k, v in top))
    assert d_out < 1e-5
    bad = {k: v for k, v in shares.items() if v > 0.25}
    assert not bad, bad


def test_masks_take_the_values_the_blend_must_handle():
    for regime, t, h, w in CLIPS + [("large", 2, 33, 47), ("moderate", 2, 24, 40)]:
        stock = wc.mk2_values(wc.case("cra", regime, t, h, w)[3])
        assert stock == [0.0, 0.5, 1.0], (regime, t, stock)
        lm = wc.case("cra", regime, t, h, w, mask="L")[3]
        assert wc.mk2_values(lm) == [0.0, 0.25, 0.5, 0.75, 1.0]
        assert lm.shape == (1, t, 1, 8 * h, 8 * w) and all(wc.mk2_values(lm[:, i:i + 1]) == [0.0, 0.25, 0.5, 0.75, 1.0] for i in range(t))
        assert all((lm[0, i] != lm[0, i - 1]).any() for i in range(1, t))


@pytest.mark.parametrize("wiring", ("dsv",) + wc.WIRINGS)
def test_embedded_channel_map_is_embed_mid32s(orc, wiring):
    """The narrow (mid_channels = 16) oracle against the 32-channel oracle on ``embed_mid32``'s weights: every tap of the table sits at
    ``embedded_channels``' positions, and every other channel is exactly zero -- the map the GPU test reads the engine's buffers with."""
    from crfp_amd import engine
    regime, t, h, w = CLIPS[1]
    sd, lrs, fvs, mks = wc.case(wiring, regime, t, h, w, mid=16)
    flows = orc.compute_flow(orc.load_numpy_state(sd), T(lrs))
    narrow = wc.oracle_taps(orc, wiring, sd, lrs, fvs, mks, flows=flows, mid=16)
    wide_sd = {k: v.numpy() for k, v in engine.embed_mid32({k: T(v) for k, v in sd.items()}, 16, wiring).items()}
    assert {k: v.shape for k, v in wide_sd.items()} == {k: tuple(v) for k, v in wc.shapes(wiring).items()}
    wide = wc.oracle_taps(orc, wiring, wide_sd, lrs, fvs, mks, flows=flows, mid=32)
    embedded = 0
    for r in wc.ROWS[wiring]:
        e = wc.embedded_channels(wiring, r)
        for frame in (1, 2):
            x = wc.tap_of(wide[frame], r.tap)
            assert float((wide[frame]["out"] - narrow[frame]["out"]).abs().max()) < 1e-5
            if e is None:
                assert float((x - wc.tap_of(narrow[frame], r.tap)).abs().max()) <= 1e-5 * max(1.0, float(x.abs().max())), r.key
                continue
            pos, nsel = e
            nt = narrow[frame][r.tap[0]]
            nt = nt if nsel is None else nt[:, nsel]
            assert nt.shape[1] == len(pos) and len(set(pos)) == len(pos) and max(pos) < x.shape[1], (r.key, nt.shape, pos)
            assert float((x[:, pos] - nt).abs().max()) <= 1e-5 * max(1.0, float(nt.abs().max())), r.key
            rest = [c for c in range(x.shape[1]) if c not in pos]
            assert rest and not x[:, rest].any(), r.key
            embedded += 1
    assert embedded >= 2 * 25


# ----------------------------------------------------------------------------- guards
def test_dense_with_a_zero_third_source_is_simple(orc):
    """On dense weights: dropping the third source == the simple wiring run on those weights with the third input block cut off."""
    regime, t, h, w = CLIPS[1]
    sd, lrs, fvs, mks = wc.case("dense", regime, t, h, w)
    dropped = _taps("dense", "stock", regime, t, h, w, False, drop_third=True)
    cut = {k: (v[:, :2 * v.shape[1] // 3] if k.endswith("main.0.weight") and k.startswith("forward_resblocks") else v) for k, v in sd.items()}
    assert {k: v.shape for k, v in cut.items()} == {k: tuple(v) for k, v in wc.shapes("simple").items()}
    flows = orc.compute_flow(orc.load_numpy_state(sd), T(lrs))
    simple = wc.oracle_taps(orc, "simple", cut, lrs, fvs, mks, flows=flows)
    full = _taps("dense", "stock", regime, t, h, w, False)
    for i in range(t):
        assert float((dropped[i]["out"] - simple[i]["out"]).abs().max()) <= 1e-6, i
        for k in ("res0", "res2", "feat", "state_hr"):
            assert float((dropped[i][k] - simple[i][k]).abs().max()) <= 1e-6, (i, k)
    # ... and the third source matters from the first moving frame on (frame 0 multiplies it by a zero state)
    assert torch.equal(full[0]["out"], dropped[0]["out"])
    for i in (1, 2):
        for k in ("res0", "feat"):
            assert float((full[i][k] - dropped[i][k]).abs().max()) > 100 * wc.sc.bound_of(full[i][k]), (i, k)


@pytest.mark.parametrize("mask", ["stock", "L"])
def test_cra_with_the_nearest_pixel_mask_is_far_outside_the_bound(mask):
    regime, t, h, w = CLIPS[0]
    good, bad = _taps("cra", mask, regime, t, h, w, True), _taps("cra", mask, regime, t, h, w, True, mk2_mode="nearest")
    for i in range(t):
        for k in range(3):
            d = float((good[i][f"res{k}"] - bad[i][f"res{k}"]).abs().max())
            assert d > 100 * wc.sc.bound_of(good[i][f"res{k}"]), (i, k, d)


@pytest.mark.parametrize("wiring,mask", CASES)
def test_a_wrong_buffer_cannot_pass(wiring, mask):
    regime, t, h, w = CLIPS[0]
    p64 = _taps(wiring, mask, regime, t, h, w, True)
    for r in wc.ROWS[wiring]:
        for i, j in [(2, 1)] + ([(1, 0)] if not r.moving else []):
            a, b = wc.tap_of(p64[i], r.tap), wc.tap_of(p64[j], r.tap)
            assert float((a - b).abs().max()) >= 50 * wc.bound_of(wiring, r, a), (r.key, "frame", i, j)
        if r.other is not None:
            for i in (1, 2):
                a, b = wc.tap_of(p64[i], r.tap), wc.tap_of(p64[i], r.other)
                assert float((a - b).abs().max()) >= 50 * wc.bound_of(wiring, r, a), (r.key, "level", i)
