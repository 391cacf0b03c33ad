"""GPU (-m gpu): every stage of the CRFP_DSV_CRA, CRFP_simple and CRFP clip engines (``crfp_cra_`` / ``crfp_simple_`` / ``crfp_dense_forward_batch``,
csrc/engine.hip: the W_CRA, W_SIMPLE and W_DENSE wirings) against the float64 oracle.

What test_gpu_dsv_stages.py does for CRFP_DSV, for the other three wirings: every workspace buffer that carries a model tensor is read back
through the wiring's own ``debug_fetch`` and compared with the oracle's tap (``cra_frame`` / ``ablation_frame``, oracle/crfp_oracle.py, pinned to
the reference's goldens by tests/test_wiring_oracle.py), following the tables of tests/helpers/wiring_stage_cases.py.  Clips:
``steered_frames`` "large" at 33 x 47 and "moderate" at 24 x 40, t = 2 and 3 (both parities of the frame slots), weights
``steer_fnet(make_state_dict_like(...))``; cra also with the L-shaped mask whose x0.25 resample takes all of 0, 1/4, 1/2, 3/4, 1.  The flow is the
engine's own (`flow_lr`, bit-equal to the engine's ``compute_flow`` of the clip: ``crfp_fnet_forward`` with the same flow network), asserted for the
regime and injected into the oracle.

(a) output frames: fp32 build < 1e-4 of the float64 oracle (the fp32 oracle itself < 1e-5 of it; frame 1 with the flow differs from frame 1
    with zero flow by > 1e-2); bf16 build by ``test_gpu_bf16._check_frame_stats`` against the storage twin.
(b) stages on a 0xFF workspace: every live row within ``1e-4 * max(1, max |tap64|)`` (bf16 build: mean <= 0.75 x and max <= 1.5 x the twin's own
    distance to the fp32 oracle), the next frame's state (`state_hr`, `poff`, cra: `carry`) included, both frame-slot sets, gated rows inside
    their dilated mask; the set of buffers holding a non-NaN value equals the table's written set (simple / dense: `carryw` stays
    prefill, `carry` holds the exact zeros the clip's state reset leaves and nothing else).
(c) the `unfused` schedule (CRFP_DCN_FUSED=0 CRFP_CONV_PAIR=0, one child process): the buffers only it writes under the same bounds, the output
    and every fetch both runs share bit-equal.
(d) a 0xFF workspace and a used one give a fresh workspace's bits; n = 2 lock-step == one-clip calls.
(e) y_only: output and `state_hr`.
(f) mid_channels = 16 embedded in the 32-channel schedule, all four wirings: output against the narrow model's oracle / twin, in every fetched
    stage the channels ``embed_mid32`` leaves empty exactly 0.0, the occupied ones within the row's bound of the narrow oracle's tap.

Measured on an MI355X (63 tests, 56 s).  Output frames: 1.8e-6 (cra), 2.0e-6 (simple), 1.1e-6 (dense) from the float64 oracle, whose fp32 run
sits 0.7e-6 .. 2.9e-6 from it; embedded mid 16: 0.9e-6 (dsv), 0.8e-6 (cra), 1.3e-6 (simple), 6.4e-6 (dense), and 2.8 .. 4.1 million values of
empty channels per wiring and build are exactly 0.0.  Worst fp32 share of the stage bound, product schedule: cra 0.046 (`aligned3`, large t = 2),
simple 0.092 (`aligned3`, moderate t = 3), dense 0.046 (`flow_lr`); unfused schedule: 0.224 / 0.209 / 0.166, all on `om3:mask` (large t = 3, 2.2e-5
of 1e-4; the fp32 oracle itself is 0.14 .. 0.19 there).  bf16 build, worst mean / max ratio to the twin's own distance (asserted <= 0.75 / 1.5):
cra 0.63 (`prev2`) / 1.09 (`offfeat0`, L mask), simple 0.64 (`om3:mask`) / 1.32 (`offfeat1`), dense 0.62 (`prev2`) / 1.10 (`aligned`); unfused
rows 0.34 / 0.70 at most (`res.y1`).  One row misses the default max factor without a defect: cra `xin8` (BF16_FACTORS above).  The unfused run
gives the product run's output bits and the bits of every shared fetch; a 0xFF or used workspace and the n = 2 lock-step call never changed a bit.

Census (t = 3; buffers of the table left untouched on a 0xFF workspace), as the tables say:
    cra      fp32: dcn.fa offmask res.y1 om3 res3.z0 res3.z1                 bf16: dcn.fa offmask res.y1 dcn3.g0 dcn3.g1 res3.z0 res3.z1
    simple   fp32: the same + carryw                                         bf16: the same + carryw
    dense    fp32: as simple                                                 bf16: dcn.fa offmask res.y1 dcn3.g0 dcn3.g1 carryw
                                                                                   (`res3.z0` AND `res3.z1` are written: three single launches)
    unfused: `dcn.fa`, `res.y1`, `offmask` (fp32 build: and `om3`) leave these lists; nothing else moves.
Two disagreements with the tables as first written, both in the tables: the bf16 dense path of forward_resblocks_3 is main.0 -> conv1 -> conv2 as
three launches, not main.0 -> pair (``res3_pair`` is an fp32-build constant), so `res3.z1` is live there too; and `carry` of simple / dense is not
prefill but exact zeros: ``reset_state`` clears it with the recurrent state although these wirings never read it.  No defect in a kernel.

Mutation guard (four one-line changes, each built as a scratch library and run through this file; tests failed of 63): cra_blend_kernel reading the
block's corner pixel 23 (every cra test that compares values), the dense third source of res3.main0 bound to another tensor 13 (every such dense
test), prev2w = flow_warp(prev2, flow2) in simple / dense 26, cra.tttf_level's two sources swapped in the bind 27 (the workspace- and
batch-invariance tests included: the swapped bind reads past the level tensor)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import motion_cases as mc
from helpers import wiring_stage_cases as wc

pytestmark = pytest.mark.gpu

T = torch.from_numpy
RUNS = [("large", 2, 33, 47), ("large", 3, 33, 47), ("moderate", 2, 24, 40), ("moderate", 3, 24, 40)]
CHILD = ("large", 3, 33, 47)
CASES = [(w, "stock") for w in wc.WIRINGS] + [("cra", "L")]
BF16_DEFAULT = (0.75, 1.5)        # test_gpu_bf16's factors, applied per stage as test_gpu_dsv_stages.py applies them
# (wiring, row key) -> (mean factor, max rule) where the default is missed without a defect (test_gpu_dsv_stages.BF16_FACTORS' mechanism).
# cra / xin8: the tensor is the fp32 blend fv * mk + up8(lr) * (1 - mk) rounded ONCE to bf16, so the twin's distance to the fp32 oracle is the
# rounding itself, below half a bf16 ulp.  The kernel and ATen evaluate the x8 bilinear sum in different fp32 orders; where the fp32 value sits
# next to a rounding tie the two round to neighbouring bf16 values, one whole ulp apart -- just over 2.0 x the twin's maximum, and no
# rounded-once tensor can be further off.  CRFP_DSV compares this buffer inside the dilated fovea mask only; W_CRA writes and compares the whole
# frame (595 584 values), and frame 0 of the large clips has one such element (max 3.906e-03 = 2^-8 against the twin's 1.953e-03, mean ratio
# 0.000).  The max rule for it is therefore the project's own for tensors next to the inputs (test_gpu_bf16.
# test_bf16_intermediates_round_where_the_twin_rounds): every element within one bf16 ulp, max(|twin|, 1e-3) * 2^-7.  The mean factor stays.
BF16_FACTORS = {("cra", "xin8"): (0.75, "ulp")}
ALL_MK2 = [0.0, 0.25, 0.5, 0.75, 1.0]


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


def _gpu(*arrays):
    return tuple(T(np.ascontiguousarray(a)).to("cuda:0") for a in arrays)


@functools.lru_cache(maxsize=None)
def _run(wiring, mask, regime, t, h, w, storage="f32", y_only=False, mid=32):
    """The product schedule in this process, on a 0xFF workspace: the output and every buffer of the wiring's table."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    got = wc.run_case(wiring, regime, t, h, w, storage, y_only, mask, mid=mid)
    assert not bool(got["overflowed"])
    return got


def _flows(got):
    return T(got["flow_lr"][:, :2].copy())[None]        # [1, t - 1, 2, h, w]


@functools.lru_cache(maxsize=None)
def _ref(wiring, mask, regime, t, h, w, kind, storage="f32", y_only=False, mid=32, still=False):
    """Oracle taps per frame with the flow the `storage` engine fetched: kind "f64" / "f32" / "twin" (still: that flow times zero)."""
    from oracle import crfp_oracle
    sd, lrs, fvs, mks = wc.case(wiring, regime, t, h, w, y_only, mask, mid)
    flows = _flows(_run(wiring, mask, regime, t, h, w, storage, y_only, mid))
    return wc.oracle_taps(crfp_oracle, wiring, sd, lrs, fvs, mks, flows=flows * 0 if still else flows, double=kind == "f64", bf16=kind == "twin",
                          y_only=y_only, mid=mid)


def _outs(refs):
    return torch.stack([p["out"] for p in refs], 1)


def _assert_inputs(got, wiring, mask, regime, t, h, w, storage, what):
    """The regime on the flow the engine used; that flow is the engine's compute_flow (crfp_fnet_forward) of the clip, bit for bit; the L mask's condition."""
    s = mc.flow_stats(_flows(got), h, w)
    print(f"{what}: engine flow {mc.fmt_stats(s)}")
    mc.assert_regime(s, regime)
    assert np.array_equal(got["flow_engine"][0], got["flow_lr"][:, :2]), "compute_flow is not the clip's own flow"
    if mask == "L":
        assert wc.mk2_values(wc.case(wiring, regime, t, h, w, mask=mask)[3]) == ALL_MK2


def _pick(got, row, name, idx, reg):
    x = got[name][idx:idx + 1]
    if row.sel is not None:
        x = x[:, row.sel]
    x = x.astype(np.float64)
    where = np.ones(x.shape, bool) if reg is None else np.broadcast_to(reg[None, None], x.shape)
    return x, where


def _compare(got, wiring, build, sched, t, refs, mks, rows, what, refs32=None):
    """Every slot of `rows`: fp32 build against the float64 taps under the row's bound; bf16 build against the twin's taps by the per-stage
    yardstick (refs = twin, refs32 = fp32 oracle).  Prints every figure, then asserts."""
    f = wc.flags(wiring, build, sched)
    bad = []
    for r in rows:
        for name, idx, frame in wc.slots(r, t):
            tap = wc.tap_of(refs[frame], r.tap).double().numpy()
            x, where = _pick(got, r, name, idx, wc.region(r, f, mks[0, frame, 0]))
            assert x.shape == tap.shape, (r.key, x.shape, tap.shape)
            d = np.abs(x - tap)[where]
            finite = bool(np.isfinite(x[where]).all())
            tag = f"STAGE {wiring} {what} {build} {sched} {r.key} [{name} frame {frame}]"
            if refs32 is None:
                bound = wc.bound_of(wiring, r, tap)
                print(f"{tag} max|HIP-tap64| {d.max():.3e} max|tap64| {np.abs(tap).max():.3e} bound {bound:.1e} share {d.max() / bound:.3f}")
                ok = finite and float(d.max()) < bound
            else:
                td = np.abs(tap - wc.tap_of(refs32[frame], r.tap).double().numpy())[where]
                fm, fx = BF16_FACTORS.get((wiring, r.key), BF16_DEFAULT)
                if td.max() == 0.0:      # a tensor the storage does not touch: the fp32 bound
                    bound = wc.bound_of(wiring, r, tap)
                    print(f"{tag} max|HIP-twin| {d.max():.3e} max|twin| {np.abs(tap).max():.3e} twin == fp32 oracle: bound {bound:.1e}")
                    ok = finite and float(d.max()) < bound
                else:
                    print(f"{tag} mean|HIP-twin| {d.mean():.3e} max {d.max():.3e} | twin vs fp32 oracle mean {td.mean():.3e} max {td.max():.3e} | "
                          f"ratios {d.mean() / td.mean():.3f} {d.max() / td.max():.3f} (factors {fm} {fx})")
                    within = bool((d <= np.maximum(np.abs(tap[where]), 1e-3) * 2.0 ** -7).all()) if fx == "ulp" else float(d.max()) <= fx * float(td.max())
                    ok = finite and float(d.mean()) <= fm * float(td.mean()) and within
            if not ok:
                bad.append((r.key, name, frame))
    assert not bad, bad


def _census(got, wiring, build, sched, t, mks, what):
    f = wc.flags(wiring, build, sched)
    names = wc.fetch_names(wiring, t)
    holds = sorted(n for n in names if not np.isnan(got[n]).all())
    want = wc.written_names(wiring, build, sched, t)
    print(f"CENSUS {wiring} {what} {build} {sched} t={t}: written {' '.join(holds)} | untouched {' '.join(n for n in names if n not in holds)}")
    assert holds == sorted(want + list(wc.CLEARED[wiring])), (sorted(set(holds) - set(want)), sorted(set(want) - set(holds)))
    for n in wc.NEVER_WRITTEN[wiring]:
        assert np.isnan(got[n]).all(), n
    for n in wc.CLEARED[wiring]:          # zeroed with the recurrent state, written by no launch
        assert not got[n].any(), n
    for r in wc.rows_for(wiring, build, sched):
        for name, idx, frame in wc.slots(r, t):
            x, where = _pick(got, r, name, idx, wc.region(r, f, mks[0, frame, 0]))
            assert not np.isnan(x[where]).any(), (r.key, name)
    assert np.isfinite(got["out"]).all()


# ----------------------------------------------------------------------------- (a), (b): the product schedule, in this process
@pytest.mark.parametrize("regime,t,h,w", RUNS)
@pytest.mark.parametrize("wiring,mask", CASES)
def test_f32_stages_vs_float64(wiring, mask, regime, t, h, w):
    got, mks = _run(wiring, mask, regime, t, h, w), wc.case(wiring, regime, t, h, w, mask=mask)[3]
    what = f"{mask}/{regime}/t{t}"
    _assert_inputs(got, wiring, mask, regime, t, h, w, "f32", f"{wiring} {what}")
    refs, refs32 = _ref(wiring, mask, regime, t, h, w, "f64"), _ref(wiring, mask, regime, t, h, w, "f32")
    d = float(np.abs(got["out"].astype(np.float64) - _outs(refs).numpy()).max())
    d_ref = float((_outs(refs32).double() - _outs(refs)).abs().max())
    moved = float((refs32[1]["out"] - _ref(wiring, mask, regime, t, h, w, "f32", still=True)[1]["out"]).abs().max())
    print(f"STAGE {wiring} {what} f32 product out max|HIP-oracle64| {d:.3e}; oracle fp32 vs float64 {d_ref:.3e}; frame 1 with this flow vs zero flow {moved:.2f}")
    assert d_ref < 1e-5
    assert moved > 1e-2, "the motion does not reach the output"
    assert d < 1e-4
    _compare(got, wiring, "f32", "product", t, refs, mks, wc.rows_for(wiring, "f32", "product"), what)
    _census(got, wiring, "f32", "product", t, mks, what)


@pytest.mark.parametrize("regime,t,h,w", RUNS)
@pytest.mark.parametrize("wiring,mask", CASES)
def test_bf16_stages_vs_twin(wiring, mask, regime, t, h, w):
    from test_gpu_bf16 import _check_frame_stats
    got, mks = _run(wiring, mask, regime, t, h, w, "bf16"), wc.case(wiring, regime, t, h, w, mask=mask)[3]
    what = f"{mask}/{regime}/t{t}"
    _assert_inputs(got, wiring, mask, regime, t, h, w, "bf16", f"{wiring} {what} bf16")
    twin, refs32 = _ref(wiring, mask, regime, t, h, w, "twin", "bf16"), _ref(wiring, mask, regime, t, h, w, "f32", "bf16")
    _check_frame_stats(T(got["out"]), _outs(twin), _outs(refs32), f"{wiring} {what} bf16")
    _compare(got, wiring, "bf16", "product", t, twin, mks, wc.rows_for(wiring, "bf16", "product"), what, refs32=refs32)
    _census(got, wiring, "bf16", "product", t, mks, what)


# ----------------------------------------------------------------------------- (c): the unfused schedule, one child process for all
@functools.lru_cache(maxsize=None)
def _child(tmp):
    env = dict(os.environ, **wc.SCHEDULES["unfused"])
    regime, t, h, w = CHILD
    res = {}
    for mask in ("stock", "L"):
        path = os.path.join(tmp, f"unfused_{mask}.npz")
        p = subprocess.run([sys.executable, os.path.abspath(wc.__file__), path, "--wiring", ",".join(wc.WIRINGS) if mask == "stock" else "cra", "--regime", regime,
                            "--t", str(t), "--h", str(h), "--w", str(w), "--storage", "f32,bf16", "--mask", mask], capture_output=True, text=True, env=env,
                           timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        with np.load(path) as z:
            res.update({f"{mask}:{k}": z[k] for k in z.files})
    return res


@pytest.fixture(scope="module")
def child_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("wiring_stages"))


@pytest.mark.parametrize("build", wc.BUILDS)
@pytest.mark.parametrize("wiring,mask", CASES)
def test_unfused_schedule_stages_and_bits(wiring, mask, build, child_dir):
    regime, t, h, w = CHILD
    pre = f"{mask}:{wiring}:{build}:"
    got = {k[len(pre):]: v for k, v in _child(child_dir).items() if k.startswith(pre)}
    prod, mks = _run(wiring, mask, regime, t, h, w, build), wc.case(wiring, regime, t, h, w, mask=mask)[3]
    assert not bool(got["overflowed"])
    what = f"{mask}/large/t3"
    _census(got, wiring, build, "unfused", t, mks, what)
    mine = [r for r in wc.rows_for(wiring, build, "unfused") if r not in wc.rows_for(wiring, build, "product")]
    assert {r.buf for r in mine} == {"dcn.fa", "res.y1", "offmask"} | ({"om3"} if build == "f32" else set())
    if build == "f32":
        _compare(got, wiring, build, "unfused", t, _ref(wiring, mask, regime, t, h, w, "f64"), mks, mine, what)
    else:
        _compare(got, wiring, build, "unfused", t, _ref(wiring, mask, regime, t, h, w, "twin", "bf16"), mks, mine, what,
                 refs32=_ref(wiring, mask, regime, t, h, w, "f32", "bf16"))
    assert np.array_equal(got["out"].view(np.uint32), prod["out"].view(np.uint32)), "output"
    fp = wc.flags(wiring, build, "product")
    shared = [r for r in wc.rows_for(wiring, build, "unfused", compared_only=False) if r in wc.rows_for(wiring, build, "product", compared_only=False)]
    n = 0
    for r in shared:
        for name, idx, frame in wc.slots(r, t):
            a, where = _pick(got, r._replace(sel=None), name, idx, wc.region(r, fp, mks[0, frame, 0]))
            b, _ = _pick(prod, r._replace(sel=None), name, idx, None)
            assert np.array_equal(np.where(where, a, 0.0).astype(np.float32).view(np.uint32), np.where(where, b, 0.0).astype(np.float32).view(np.uint32)), \
                (wiring, build, name)
            n += 1
    print(f"BITS {wiring} {what} {build} unfused: {n} buffers bit-equal to the product run; compared on their own: {' '.join(r.key for r in mine)}")


# ----------------------------------------------------------------------------- (d): workspace and batch invariance
STATE_NAMES = {"cra": ["state_hr", "carry", "poff", "feat", "x_lr", "flow_lr", "cra.y", "cra.fused"], "simple": ["state_hr", "poff", "feat", "x_lr", "flow_lr", "prev2w"],
               "dense": ["state_hr", "poff", "feat", "x_lr", "flow_lr", "prev2w"]}


@pytest.mark.parametrize("storage", wc.BUILDS)
@pytest.mark.parametrize("wiring", wc.WIRINGS)
def test_dirty_and_used_workspace_give_a_fresh_ones_bits(wiring, storage):
    regime, t, h, w = CHILD
    sd, lrs, fvs, mks = wc.case(wiring, regime, t, h, w)
    other = wc.case(wiring, "moderate", t, h, w)
    names = STATE_NAMES[wiring]
    res = []
    for how in ("fresh", "dirty", "used"):
        m = wc.make_model(wiring, sd, storage)
        eng = m.engine()
        if how == "dirty":
            wc.sc.dirty_workspace(eng, t, h, w)
        elif how == "used":
            m(*_gpu(*other[1:]))               # another clip of the same geometry went through this workspace first
        out = m(*_gpu(lrs, fvs, mks))
        assert not eng.overflowed()
        res.append([out.cpu()] + [eng.debug_fetch(n, t, h, w).cpu() for n in names])
    assert torch.isfinite(res[0][0]).all()
    for how, other_res in zip(("dirty", "used"), res[1:]):
        for n, a, b in zip(["out"] + names, res[0], other_res):
            assert torch.equal(a, b), f"{wiring} {storage} {n}: a {how} workspace changes the bits"
    assert np.array_equal(res[0][0].numpy(), _run(wiring, "stock", regime, t, h, w, storage)["out"])


@pytest.mark.parametrize("storage", wc.BUILDS)
@pytest.mark.parametrize("wiring", wc.WIRINGS)
def test_lockstep_batch_is_the_one_clip_calls(wiring, storage):
    t, h, w = 3, 33, 47
    sd, big = wc.case(wiring, "large", t, h, w)[0], wc.case(wiring, "large", t, h, w)[1:]
    small = wc.case(wiring, "moderate", t, h, w)[1:]
    m = wc.make_model(wiring, sd, storage)
    wc.sc.dirty_workspace(m.engine(), t, h, w, 2)
    two = m(*_gpu(*(np.concatenate([a, b], 0) for a, b in zip(big, small)))).cpu()
    assert not m.engine().overflowed() and torch.isfinite(two).all()
    one = wc.make_model(wiring, sd, storage)
    assert torch.equal(two[:1], one(*_gpu(*big)).cpu()) and torch.equal(two[1:], one(*_gpu(*small)).cpu())
    assert np.array_equal(two[:1].numpy(), _run(wiring, "stock", "large", t, h, w, storage)["out"])


# ----------------------------------------------------------------------------- (e): y_only
@pytest.mark.parametrize("wiring", wc.WIRINGS)
def test_y_only_output_and_state(wiring):
    regime, t, h, w = CHILD
    got, mks = _run(wiring, "stock", regime, t, h, w, "f32", True), wc.case(wiring, regime, t, h, w, True)[3]
    _assert_inputs(got, wiring, "stock", regime, t, h, w, "f32", f"{wiring} y_only")
    refs = _ref(wiring, "stock", regime, t, h, w, "f64", "f32", True)
    assert got["out"].shape[2] == 1
    d = float(np.abs(got["out"].astype(np.float64) - _outs(refs).numpy()).max())
    print(f"STAGE {wiring} y_only out max|HIP-oracle64| {d:.3e}")
    assert d < 1e-4
    _compare(got, wiring, "f32", "product", t, refs, mks, [r for r in wc.rows_for(wiring, "f32", "product") if r.key in ("state_hr", "feat")], "large/t3/y_only")


# ----------------------------------------------------------------------------- (f): mid_channels = 16 embedded in the 32-channel schedule
@pytest.mark.parametrize("storage", wc.BUILDS)
@pytest.mark.parametrize("wiring", ("dsv",) + wc.WIRINGS)
def test_embedded_mid16_output_empty_and_occupied_channels(wiring, storage):
    from test_gpu_bf16 import _check_frame_stats
    regime, t, h, w = CHILD
    got, mks = _run(wiring, "stock", regime, t, h, w, storage, False, 16), wc.case(wiring, regime, t, h, w, mid=16)[3]
    what = f"{wiring} mid16 {storage}"
    mc.assert_regime(mc.flow_stats(_flows(got), h, w), regime)
    f = wc.flags(wiring, storage, "product")
    bf16 = storage == "bf16"
    refs = _ref(wiring, "stock", regime, t, h, w, "twin" if bf16 else "f64", storage, False, 16)
    refs32 = _ref(wiring, "stock", regime, t, h, w, "f32", storage, False, 16)
    if bf16:
        _check_frame_stats(T(got["out"]), _outs(refs), _outs(refs32), what)
    else:
        d = float(np.abs(got["out"].astype(np.float64) - _outs(refs).numpy()).max())
        print(f"STAGE {what} out max|HIP-narrow oracle64| {d:.3e}")
        assert d < 1e-4
    bad, n_empty = [], 0
    for r in wc.rows_for(wiring, storage, "product"):
        e = wc.embedded_channels(wiring, r)
        if e is None:
            continue
        pos, nsel = e
        for name, idx, frame in wc.slots(r, t):
            x, where = _pick(got, r, name, idx, wc.region(r, f, mks[0, frame, 0]))
            rest = [c for c in range(x.shape[1]) if c not in pos]
            empty = x[:, rest][where[:, rest]]
            n_empty += empty.size
            if not (empty == 0.0).all():
                bad.append((r.key, name, "empty channels", float(np.abs(np.nan_to_num(empty, nan=np.inf)).max())))
            pick = lambda taps: (taps[frame][r.tap[0]] if nsel is None else taps[frame][r.tap[0]][:, nsel]).double().numpy()      # noqa: E731
            tap, occ = pick(refs), x[:, pos]
            d = np.abs(occ - tap)[where[:, pos]]
            if not bf16:
                bound = wc.bound_of(wiring, r, tap)
                print(f"STAGE {what} {r.key} [{name} frame {frame}] occupied max|HIP-tap64| {d.max():.3e} bound {bound:.1e}")
                ok = float(d.max()) < bound
            else:
                td = np.abs(tap - pick(refs32))[where[:, pos]]
                print(f"STAGE {what} {r.key} [{name} frame {frame}] occupied mean|HIP-twin| {d.mean():.3e} max {d.max():.3e} | twin vs fp32 oracle {td.mean():.3e} {td.max():.3e}")
                ok = (float(d.max()) < wc.bound_of(wiring, r, tap)) if td.max() == 0.0 else \
                    (float(d.mean()) <= BF16_DEFAULT[0] * float(td.mean()) and float(d.max()) <= BF16_DEFAULT[1] * float(td.max()))
            if not (ok and np.isfinite(occ[where[:, pos]]).all()):
                bad.append((r.key, name, frame))
    print(f"EMBEDDED {what}: {n_empty} values of empty channels are exactly 0.0")
    assert n_empty > 0 and not bad, bad
