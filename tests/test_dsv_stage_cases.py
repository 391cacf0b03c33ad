"""CPU: the stage table of the CRFP_DSV clip engine (tests/helpers/dsv_stage_cases.py) against the oracle alone.

* every tap the table names exists, and has the shape ``crfp_dsv_debug_fetch`` reports for the buffer (its size query touches no device memory)
  after the table's channel selection;
* every fetchable buffer of ``Layout`` is a row, or listed in NOT_MODEL;
* the bound 1e-4 * max(1, max |tap64|) is safe on the reference alone: max |oracle fp32 - oracle float64| with the same injected flow stays
  within a quarter of it for every tap (the measured shares: the helper's docstring);
* a right buffer can be told from a plausible wrong one: a tap at frame i is at least 50 bounds away from the same tap at frame i - 1 (a stale
  buffer, a swapped parity set), and a reused buffer's level-2 tap at least 50 bounds from the level a stale launch would have left.  The rows
  that cannot be told apart this way are listed in INDISTINCT with their reasons, and nothing else may fall short."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import dsv_stage_cases as sc
from helpers import motion_cases as mc

T = torch.from_numpy
CLIPS = [("large", 3, 33, 47), ("moderate", 3, 24, 40)]
# rows whose tap at frame i may be closer than 50 bounds to frame i - 1's: (row key) -> reason
INDISTINCT = {}      # none: the closest pair of the two clips is more than 200 bounds apart


@pytest.fixture(scope="module")
def orc():
    from oracle import crfp_oracle
    return crfp_oracle


@functools.lru_cache(maxsize=None)
def _taps(regime, t, h, w, double):
    """Frame-by-frame taps with the fp32 oracle's own flow injected into both precisions."""
    from oracle import crfp_oracle
    sd, lrs, fvs, mks = mc.steered_case(regime, t, h, w)
    flows = crfp_oracle.compute_flow(crfp_oracle.load_numpy_state(sd), T(lrs))
    return sc.oracle_taps(crfp_oracle, sd, lrs, fvs, mks, flows=flows, double=double)


def _fetch_shape(name, t, h, w):
    """(N, C, H, W) of a fetch, from the library's own Layout (out_nchw = NULL: nothing is read or written)."""
    from crfp_amd import _lib
    fn = _lib.lib().crfp_dsv_debug_fetch
    dummy = C.create_string_buffer(8)
    c, hh, ww = C.c_int(), C.c_int(), C.c_int()
    n = fn(name.encode(), t, h, w, C.cast(dummy, C.c_void_p), None, C.byref(c), C.byref(hh), C.byref(ww), None)
    return (n, c.value, hh.value, ww.value) if n >= 0 else None


def test_table_is_well_formed():
    keys = [r.key for r in sc.ROWS]
    assert len(set(keys)) == len(keys)
    for build in sc.BUILDS:
        for sched in sc.SCHEDULES:
            assert sc.rows_for(build, sched), (build, sched)
    # per build every row is compared under some schedule or listed as unreachable with a reason; only res3.z1 is out of reach in both builds
    for r in sc.ROWS:
        per_build = {b: any(r in sc.rows_for(b, s) for s in sc.SCHEDULES) for b in sc.BUILDS}
        assert any(per_build.values()) or r.key == "res3.z1", r.key
        for b, ok in per_build.items():
            assert ok or len(sc.UNREACHABLE[(b, r.key)]) > 20, (b, r.key)
    for (b, k) in sc.UNREACHABLE:
        r = next(r for r in sc.ROWS if r.key == k)
        assert not any(r in sc.rows_for(b, s) for s in sc.SCHEDULES), (b, k)
    # the buffers only an alternate schedule writes are not in the product's set; each alternate schedule adds something, except the dense launches
    # (same buffers, whole frame) and the lab library in the bf16 build (its bf16 objects are the product's)
    for build in sc.BUILDS:
        prod = set(sc.written_names(build, "product", 3))
        for sched in list(sc.SCHEDULES)[1:]:
            adds = set(sc.written_names(build, sched, 3)) - prod
            assert bool(adds) == (sched != "mask_gate0" and (build, sched) != ("bf16", "lab_unfused")), (build, sched, adds)
    assert "offmask" not in sc.written_names("f32", "product", 3) and "om3" not in sc.written_names("f32", "product", 3)
    assert "om3" in sc.written_names("bf16", "product", 3) and "dcn3.g0" in sc.written_names("f32", "product", 3)
    assert "dcn3.g0" not in sc.written_names("bf16", "product", 3) and "dcn3.g0" not in sc.written_names("bf16", "lab_unfused", 3)
    assert "res3.z0" in sc.written_names("f32", "lab_unfused", 3) and "res3.z0" not in sc.written_names("bf16", "lab_unfused", 3)
    # what only the next frame reads is in the product's compared set of both builds; the buffers Layout keeps fp32 in the bf16 build (f32 = true / kind 1)
    for build in sc.BUILDS:
        assert {"poff", "state_hr", "carry"} == {r.key for r in sc.rows_for(build, "product") if r.state}
    assert {r.buf for r in sc.ROWS if r.f32} == {"flow_lr", "fnet.g1", "flow2", "flow8", "offmask", "om3"}
    assert "flow2" not in sc.written_names("f32", "product", 2) and "flow2.1" in sc.written_names("f32", "product", 2)
    assert "flow2" in sc.written_names("f32", "product", 3)


@pytest.mark.parametrize("t,h,w", [(2, 33, 47), (3, 24, 40)])
def test_every_layout_buffer_is_a_row_or_listed(t, h, w):
    names = sc.fetch_names(t)
    for n in names:
        assert _fetch_shape(n, t, h, w) is not None, n
    # Layout's frame-level and clip-level names (engine.hip:317-383, W_DSV, t > 1): nothing fetchable is missing from the table
    layout = ["status", "state_hr", "carry", "flow_lr", "lr_q4", "enc_lr0", "x_lr"] + ["fnet." + n for n, _ in sc._FNET] + ["fnet.g1"]
    for p in ("", ".1"):
        layout += [b + p for b in ("xin8", "enc_hr0", "x_hr", "prop0", "flow2", "flow8", "gate")]
    layout += ["prop_a", "prop_b", "prev2", "prev2w", "prevhrw", "carryw", "dcn.fa", "dcn.fb", "offfeat0", "offfeat1", "offfeat2", "offmask", "aligned",
               "res.y0", "res.y1", "up", "poff", "dcn3.g0", "dcn3.g1", "dcn3.g2", "om3", "aligned3", "res3.z0", "res3.z1", "feat"]
    for n in layout:
        assert _fetch_shape(n, t, h, w) is not None, n
        assert (n in names) != (n in sc.NOT_MODEL), n
    assert set(names) <= set(layout)
    for n in ("cra.s1", "fg2", "lr_keep", "fnet.part", "no_such_buffer"):        # other wirings' and the one-frame-per-call layout's buffers are not in this Layout
        assert _fetch_shape(n, t, h, w) is None, n


@pytest.mark.parametrize("regime,t,h,w", [("large", 2, 33, 47), ("moderate", 3, 24, 40)])
def test_taps_exist_with_the_fetched_shapes(regime, t, h, w):
    per = _taps(regime, 3, h, w, False)[:t]
    for r in sc.ROWS:
        for name, idx, frame in sc.slots(r, t):
            assert r.tap[0] in per[frame], (r.key, frame)
            tap = sc.tap_of(per[frame], r.tap)
            n, c, hh, ww = _fetch_shape(name, t, h, w)
            assert 0 <= idx < n, (r.key, name, idx, n)
            if name.startswith("flow2") or name.startswith("flow8"):     # fetched as [n, H, W, 2]
                assert c == 2 and tuple(tap.shape) == (1, hh, ww, 2), (r.key, tuple(tap.shape))
                continue
            got_c = len(range(c)[r.sel]) if isinstance(r.sel, slice) else (len(r.sel) if r.sel is not None else c)
            assert tuple(tap.shape) == (1, got_c, hh, ww), (r.key, name, tuple(tap.shape), (got_c, hh, ww))
            if r.other is not None:
                assert tuple(sc.tap_of(per[frame], r.other).shape) == tuple(tap.shape), r.key
    # a 2-frame clip leaves frame 1 in set .1 and frame 0 in set 0; a 3-frame clip frame 2 in set 0 and frame 1 in set .1
    x_hr = next(r for r in sc.ROWS if r.key == "x_hr")
    assert sc.slots(x_hr, 2) == [("x_hr.1", 0, 1), ("x_hr", 0, 0)] and sc.slots(x_hr, 3) == [("x_hr", 0, 2), ("x_hr.1", 0, 1)]
    flow2 = next(r for r in sc.ROWS if r.key == "flow2")
    assert sc.slots(flow2, 2) == [("flow2.1", 0, 1)]


@pytest.mark.parametrize("regime,t,h,w", CLIPS)
def test_bound_is_safe_on_the_reference_alone(regime, t, h, w):
    p32, p64 = _taps(regime, t, h, w, False), _taps(regime, t, h, w, True)
    s = mc.flow_stats(p32[1]["flow_lr"], h, w)
    mc.assert_regime(mc.flow_stats(torch.cat([p32[i]["flow_lr"] for i in (1, 2)]), h, w), regime)
    worst = (0.0, None)
    for r in sc.ROWS:
        for frame in (1, 2):
            a, b = sc.tap_of(p32[frame], r.tap).double(), sc.tap_of(p64[frame], r.tap)
            share = float((a - b).abs().max()) / sc.bound_of(b)
            worst = max(worst, (share, f"{r.key} frame {frame}"))
            assert share <= 0.25, (r.key, frame, share)
    print(f"{regime} {t}x{h}x{w} (flow max {s['absmax']:.1f} px): worst oracle fp32 vs float64 = {worst[0]:.3f} of the bound ({worst[1]})")


def test_dilate():
    m = np.zeros((7, 9), bool)
    m[3, 4] = True
    assert sc.dilate(m, 0).sum() == 1 and sc.dilate(m, 1).sum() == 9 and sc.dilate(m, 3).sum() == 49
    m[0, 0] = True
    assert sc.dilate(m, 2)[:3, :3].all() and not sc.dilate(m, 2)[3, 0]


@pytest.mark.parametrize("regime,t,h,w", CLIPS)
def test_a_wrong_buffer_cannot_pass(regime, t, h, w):
    p64 = _taps(regime, t, h, w, True)
    short = []
    for r in sc.ROWS:
        frames = [(2, 1)] + ([(1, 0)] if not r.moving else [])
        for i, j in frames:
            a, b = sc.tap_of(p64[i], r.tap), sc.tap_of(p64[j], r.tap)
            if float((a - b).abs().max()) < 50 * sc.bound_of(a):
                short.append(r.key)
        if r.other is not None:
            for i in (1, 2):
                a, b = sc.tap_of(p64[i], r.tap), sc.tap_of(p64[i], r.other)
                assert float((a - b).abs().max()) >= 50 * sc.bound_of(a), (r.key, "level 2 against the other level", i)
    assert set(short) <= set(INDISTINCT), sorted(set(short) - set(INDISTINCT))
