"""The stage tables of the other three wirings of the one-call clip engine (csrc/engine.hip): ``W_CRA`` (CRFP_DSV_CRA), ``W_SIMPLE``
(CRFP_simple) and ``W_DENSE`` (CRFP) -- one row per fetchable workspace buffer of the wiring's own ``Layout`` (``crfp_cra_`` / ``crfp_simple_`` /
``crfp_dense_debug_fetch``) that carries a model tensor, in the row format of tests/helpers/dsv_stage_cases.py.  A row is CRFP_DSV's where the
wiring runs the same launch into the same buffer; the rows that differ are spelled out below with their engine.hip lines.
tests/test_wiring_oracle.py (CPU), tests/test_gpu_wiring_stages.py (GPU) and tools/bisect_engine.py --wiring read these tables.

simple / dense (``Layout::pq == 8``): `prop0` / `prop_a` / `prop_b` hold all 32 features of a level (no [24 | 8] split); the state is warped at
8x first and `prev2w` = downsample(`prevhrw`), an unpadded tensor (engine.hip:939-942); `carry` / `carryw` exist in the Layout and no launch
writes them (`carry` is zeroed with the state at the start of a clip, CLEARED); dcn_block.0 reads (32 | 32 | flow), res.main0 two (dense: three) 32-channel sources; the bf16 build of the dense wiring runs
forward_resblocks_3 of frames >= 1 as three launches (engine.hip:933,1037,1058-1059), so `res3.z0` and `res3.z1` reach memory there and only there.

cra: `hr_prep` and slice1 of the fovea encoder are not gated, only conv_lv3 is (engine.hip:879-887): `xin8` / `enc_hr0` / `cra.s1` hold the whole
frame, `x_hr` (= lv3) its dilated mask.  `cra.s1`, `cra.a`, `cra.b` are temporaries of a pre-work launch: item 0 holds the first frame of the
last launch, which is frame t - 1 for the t <= 3 clips used here (one clip: frames 0, 1 and then two at a time, engine.hip:1221-1228); `cra.a` /
`cra.b` end as slice4's two convs (the last of the eight ping-ponged convs, engine.hip:893-901).  `cra.lv0..2` are frame-slot tensors like
`x_hr`.  `cra.y` / `cra.fused` hold level 2's residual-block output and its conv_tttf_2 twin; the blend writes `prop_a` / `prop_b` / `carry`
(resample.hip:401).

Schedules: `product`, and `unfused` = CRFP_DCN_FUSED=0 CRFP_CONV_PAIR=0 together in one child process, which makes `dcn.fa`, `res.y1`, `offmask`
(and the fp32 build's `om3`) reach memory.  The per-switch matrix is CRFP_DSV's (test_gpu_dsv_stages.py).

Bounds.  fp32 build: ``1e-4 * max(1, max |tap64|)`` per tensor (dsv_stage_cases.bound_of).  The bound is safe on the reference alone: max |oracle
fp32 - oracle float64| with the same injected flow as a share of it, worst over frames 1 and 2 of steered ("large", 3, 33, 47) and ("moderate",
3, 24, 40) with ``case()``'s weights (tests/test_wiring_oracle.py asserts <= 0.25 for every tap these tables name; the L-mask variant of
cra included):

    cra     om3:mask 0.138   aligned3 0.103   offmask:masks 0.053   carryw 0.035   feat 0.033   state_hr 0.033   res3.z0 0.033   prevhrw 0.030
    simple  om3:mask 0.150   aligned3 0.094   offmask:masks 0.056   prevhrw 0.034   res3.z0 0.032   feat 0.031   state_hr 0.031   aligned 0.028
    dense   om3:mask 0.187   aligned3 0.051   offmask:masks 0.042   prevhrw 0.020   feat 0.018   state_hr 0.018   res3.z0 0.017   aligned 0.014
    flow_lr / fnet.g1 0.028 in every wiring (the flow network is the same); every other row below these.  No row needs a bound of its own
    (ROW_BOUNDS is empty); the output frames of the fp32 oracle sit 1.0e-6 .. 2.3e-6 from its float64 run.

Run as a script it runs one case on the GPU on a 0xFF-filled workspace and writes the output and every fetchable buffer of the wiring's table,
for each wiring and storage asked for, to an .npz (keys ``<wiring>:<storage>:<fetch name>``):
    python tests/helpers/wiring_stage_cases.py out.npz --wiring cra [--regime large --t 3 --h 33 --w 47 --storage f32,bf16 --mask L --y-only]
"""
import collections
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from helpers import dsv_stage_cases as sc      # noqa: E402
from helpers import motion_cases as mc         # noqa: E402

WIRINGS = ("cra", "simple", "dense")
CLASSES = {"dsv": "CRFP_DSV", "cra": "CRFP_DSV_CRA", "simple": "CRFP_simple", "dense": "CRFP"}
BUILDS = sc.BUILDS
SCHEDULES = collections.OrderedDict([("product", {}), ("unfused", {"CRFP_DCN_FUSED": "0", "CRFP_CONV_PAIR": "0"})])
WEIGHTS_SEED = 3          # test_gpu_motion._like_model's

Flags = collections.namedtuple("Flags", "bf16 pair fused gate chain wiring")
_row = sc._row


def flags(wiring, build, sched):
    """Runner::frame's switches (dsv_stage_cases.flags) plus the wiring.  `unfused` turns both pair sites and both fused DCN kernels off."""
    assert wiring in CLASSES and build in BUILDS and sched in SCHEDULES, (wiring, build, sched)
    bf16 = build == "bf16"
    return Flags(bf16, sched == "product", sched == "product", True, 3 if bf16 else 2, wiring)


def _build_rows(wiring):
    rows = []
    if wiring == "cra":
        for r in sc.ROWS:
            if r.key == "xin8":
                rows.append(r._replace(gated=0, line="880 (hr_prep without the gate, :879)"))
            elif r.key == "enc_hr0":
                rows.append(r._replace(gated=0, line="884 (gp = -1, :879)"))
            elif r.key == "x_hr":
                rows += [_row("cra.s1", "cra.s1", "885 (ungated; read by cra.slice2a's SRC_UNSHUF4 loader, :893)", moving=False),
                         r._replace(tap=("cra.lv3", None), line="887 (the one gated launch of the fovea encoder)")]
                rows += [_row(f"cra.lv{k}", f"cra.lv{k}", f"{901 - 3 * k} (frame slot, :889-892)", frames="set", moving=False) for k in (2, 1, 0)]
                rows += [_row("cra.a", "cra.s4a", "899 (slice4.0; ping-pong :893-900)", moving=False, other="cra.s3a"),
                         _row("cra.b", "cra.s4b", "900 (slice4.2; ping-pong :893-900)", moving=False, other="cra.s3b")]
            elif r.key == "prop_a":
                rows += [_row("cra.y", "cra.y2", "807 / 810-813 (the block's 32 channels stay together)", moving=False, other="cra.y1"),
                         _row("cra.fused", "cra.fused2", "817 (cra.tttf_level: sources {32, 16})", moving=False, other="cra.fused1"),
                         r._replace(line="818 (cra_blend_kernel, resample.hip:401: 24 plain-Q4 channels)"),]
            elif r.key == "prop_b":
                rows.append(r._replace(line="818 (cra_blend_kernel, level 1)"))
            elif r.key == "carry":
                rows.append(r._replace(line="818 (cra_blend_kernel: the 8 P4 channels of each level)"))
            else:
                rows.append(r)
        return rows
    dense = wiring == "dense"
    for r in sc.ROWS:
        if r.key in ("carryw", "carry"):
            continue                                    # in the Layout, written by no launch (NEVER_WRITTEN / CLEARED)
        if r.key == "prop0":
            rows.append(r._replace(line="904 (Layout::pq == 8: `upsample` has 128 output channels)"))
        elif r.key == "prev2w":
            rows.append(r._replace(line="942 (IT_DOWN on prevhrw into the unpadded prev2w; the 8x warp first, :941)"))
        elif r.key == "prevhrw":
            rows.append(r._replace(line="941"))
        elif r.key == "dcn.fa":
            rows.append(r._replace(line="962 (three sources 32 | 32 | flow, :956; paired: stays in LDS, :958-960)"))
        elif r.key == "res.y0":
            rows.append(r._replace(line="998 (two sources; dense: three, :996-997)" if not dense else "998 (three sources 32 | 32 | 32, :996-997)"))
        elif r.key == "prop_a":
            rows.append(r._replace(tap=("res2", None), other=("res0", None), line="808 (one 8-quad destination)"))
        elif r.key == "prop_b":
            rows.append(r._replace(tap=("res1", None), line="808 (one 8-quad destination, level 1)"))
        elif r.key == "res3.z0":
            rows.append(r._replace(live=lambda f: (not f.chain & 2) or (f.bf16 and f.wiring == "dense"),
                                   line="1037 (bf16 build, dense, frames >= 1: r3_chain is false, :933; three source quads, :1036)"))
        elif r.key == "res3.z1":
            rows.append(r._replace(live=lambda f: f.bf16 and f.wiring == "dense",
                                   line="1058 (bf16 build, dense, frames >= 1: res3_pair is false there, :674,1057-1059)"))
        else:
            rows.append(r)
    return rows


ROWS = {w: _build_rows(w) for w in WIRINGS}
ROWS["dsv"] = list(sc.ROWS)
# fetchable buffers of a wiring's Layout that no launch of any schedule of either build writes (beside dsv_stage_cases.UNREACHABLE's, which hold
# for every wiring except where a row above says otherwise).  NEVER_WRITTEN: they keep the workspace's prefill.  CLEARED: Runner::reset_state
# (engine.hip:750-758) zeroes them at the start of every clip with the recurrent state -- `carry` is part of CRFP_DSV's state, and the simple /
# dense wirings, which have no carried features, clear it all the same and never touch it again: exact zeros, read by nobody.
NEVER_WRITTEN = {"cra": (), "simple": ("carryw",), "dense": ("carryw",), "dsv": ()}
CLEARED = {"cra": (), "simple": ("carry",), "dense": ("carry",), "dsv": ()}
NOT_MODEL = sc.NOT_MODEL
# rows whose fp32 bound is 4 x the oracle's own measured fp32-vs-float64 distance instead of 1e-4 * max(1, max |tap64|): (wiring, key) -> bound
ROW_BOUNDS = {}

tap_of, slots, fetch_name, dilate, region = sc.tap_of, sc.slots, sc.fetch_name, sc.dilate, sc.region


def bound_of(wiring, row, tap64):
    return ROW_BOUNDS.get((wiring, row.key), None) or sc.bound_of(tap64)


def rows_for(wiring, build, sched, compared_only=True):
    f = flags(wiring, build, sched)
    return [r for r in ROWS[wiring] if r.live(f) and (r.tensor(f) or not compared_only)]


def fetch_names(wiring, t):
    """Every fetch name the census reads after a t-frame clip: the table's, written or not, and the wiring's NEVER_WRITTEN / CLEARED buffers."""
    out = []
    for r in ROWS[wiring]:
        for n in ([fetch_name(r.buf, 0), fetch_name(r.buf, 1)] if r.frames == "set" else [r.buf]):
            if n not in out:
                out.append(n)
    return out + [n for n in NEVER_WRITTEN[wiring] + CLEARED[wiring] if n not in out]


def written_names(wiring, build, sched, t):
    return sorted({name for r in rows_for(wiring, build, sched, compared_only=False) for name, _, _ in slots(r, t)})


# ----------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def shapes(wiring, mid=32, y_only=False):
    """{key: shape} of the wiring's model at mid_channels = mid (parameters only: built on the CPU)."""
    import torch
    from crfp_amd.model import CRFP
    m = getattr(CRFP, CLASSES[wiring])(torch.device("cpu"), mid_channels=mid, y_only=y_only)
    return collections.OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())


def l_mask(t, H8, W8):
    """bool [1, t, 1, H8, W8]: an L-shaped union of two rectangles whose edges sit at 4 d + 2, so that the x0.25 bilinear resample -- the mean of
    the centre 2 x 2 pixels (4 d + 1, 4 d + 2) of each 4 x 4 block -- takes 1/2 along the edges, 1/4 at the five convex corners and 3/4 at
    the concave one; frame i is shifted by 4 i pixels, which keeps the alignment."""
    H2, W2 = H8 // 4, W8 // 4
    r0, r1, r2 = H2 // 6, H2 // 2, (5 * H2) // 6 - 2
    c0, c1, c2 = W2 // 6, W2 // 2, (5 * W2) // 6 - 2
    mk = np.zeros((1, t, 1, H8, W8), np.bool_)
    for i in range(t):
        e = lambda d: 4 * (d + i) + 2      # noqa: E731
        mk[0, i, 0, e(r0):e(r2), e(c0):e(c1)] = True
        mk[0, i, 0, e(r1):e(r2), e(c0):e(c2)] = True
    return mk


def mk2_values(mks):
    """The sorted set of values of F.interpolate(mk.float(), scale_factor=0.25, mode="bilinear") over a clip's masks."""
    import torch
    import torch.nn.functional as F
    m = torch.from_numpy(np.asarray(mks)).float()
    return sorted(set(F.interpolate(m.reshape(-1, 1, *m.shape[-2:]), scale_factor=0.25, mode="bilinear", align_corners=False).unique().tolist()))


@functools.lru_cache(maxsize=None)
def case(wiring, regime, t, h, w, y_only=False, mask="stock", mid=32):
    """(state dict, lrs, fvs, mks): ``steer_fnet(make_state_dict_like(the wiring's shapes, WEIGHTS_SEED))`` -- test_gpu_motion._like_model's
    weights -- and motion_cases' steered frames of the regime.  mask "L": the fovea mask replaced by ``l_mask`` (fvs untouched)."""
    from crfp_amd import synth
    sd = mc.steer_fnet(synth.make_state_dict_like(shapes(wiring, mid, y_only), WEIGHTS_SEED))
    lrs, fvs, mks = mc.steered_frames(mc.CLIP_SEED, t, h, w, mc.REGIMES[regime])
    if mask == "L":
        mks = l_mask(t, 8 * h, 8 * w)
    else:
        assert mask == "stock", mask
    return sd, lrs, fvs, mks


# ----------------------------------------------------------------------------- mid_channels = 16 embedded in the 32-channel schedule
def embedded_channels(wiring, row, mid=16):
    """Where ``crfp_amd.engine.embed_mid32`` puts the narrow model's tensor inside a row's fetched tensor (after the row's channel selection):
    (channel positions in the narrow tap's order, the narrow tap's own selection), or None for a tensor mid_channels is not part of (the
    frames, the flows, FNet, the DCN offsets and masks).  Every other channel of the fetched tensor must be exactly zero."""
    m, l = mid, mid // 8
    abl = wiring in ("simple", "dense")
    p = m if abl else 3 * m // 4
    feat, lq, q4 = list(range(m)), list(range(l)), list(range(4 * l))
    cur = feat if abl else list(range(p)) + [24 + j for j in range(m - p)]
    grp = [4 * (j // l) + j % l for j in range(m)]
    k = row.key
    if k in ("enc_lr0", "x_lr", "dcn.fa", "dcn.fb", "offfeat0", "offfeat1", "offfeat2", "aligned", "res.y1"):
        return feat, row.tap[1]
    if k in ("prop0", "prop_a", "prop_b"):
        return list(range(p)), (None if abl or k == "prop0" else slice(0, p))
    if k in ("prev2", "prev2w"):
        return grp, None
    if k in ("carry", "carryw"):
        return [8 * lv + j for lv in range(3) for j in range(m - p)], None
    if k in ("res.y0", "cra.y", "cra.fused"):
        return cur, None
    if k in ("cra.s1", "x_hr", "enc_hr0", "up", "poff", "prevhrw", "dcn3.g0", "dcn3.g1", "dcn3.g2", "aligned3", "res3.z0", "res3.z1", "feat", "state_hr"):
        return lq, None
    if k in ("cra.lv0", "cra.lv1", "cra.lv2", "cra.a", "cra.b"):
        return q4, None
    assert k in ("flow_lr", "fnet.g1", "xin8", "flow2", "flow8", "offmask:offsets", "offmask:masks", "om3:offset", "om3:mask") or k.startswith("fnet."), k
    return None


# ----------------------------------------------------------------------------- the oracle, tapped frame by frame
def oracle_taps(orc, wiring, sd, lrs, fvs, mks, flows=None, double=False, bf16=False, y_only=False, mid=32, **frame_kw):
    """dsv_stage_cases.oracle_taps for any wiring: [taps of frame 0, ..., frame t - 1] (plus "out"; frames >= 1 carry "flow_lr" and "fnet.*" of
    their pair).  frame_kw: the guards' switches of ``cra_frame`` / ``ablation_frame`` (mk2_mode, drop_third)."""
    import contextlib
    import torch
    dt = torch.float64 if double else torch.float32
    P = orc.load_numpy_state(sd)
    if bf16:
        P = orc.bf16_weights(P)
    P = {k: v.to(dt) for k, v in P.items()}
    T = torch.from_numpy
    L, Fv, M = T(np.asarray(lrs)).to(dt), T(np.asarray(fvs)).to(dt), T(np.asarray(mks))
    n, t, _, h, w = L.shape
    cfg = orc.WiringConfig(wiring, mid, y_only)
    step, ftaps = orc.frame_fn(cfg), {}
    with torch.no_grad(), (orc.bf16_storage() if bf16 else contextlib.nullcontext()):
        with orc.tapping(ftaps):
            own = orc.compute_flow(P, L)
        ftaps["flow_lr"] = own[0]
        flows = own if flows is None else torch.as_tensor(flows).to(dt)
        st = orc.wiring_new_state(cfg, n, h, w, L)
        per = []
        for i in range(t):
            taps = {}
            with orc.tapping(taps):
                out, st = step(P, cfg, st, L[:, i], Fv[:, i], M[:, i], flows[:, i - 1] if i else None, **frame_kw)
            taps["out"] = out
            if i:
                taps.update({k: v[i - 1:i] for k, v in ftaps.items()})
            per.append(taps)
    return per


# ----------------------------------------------------------------------------- the engine: one case, every buffer of the table
def make_model(wiring, sd, storage="f32", y_only=False, mid=32, stream=False):
    import torch
    from crfp_amd.model import CRFP
    dev = torch.device("cuda:0")
    cls = CLASSES[wiring] if not stream else {"dsv": "MRCF_simple_v18", "cra": "MRCF_simple_v18_cra", "simple": "MRCF_simple_v13", "dense": "MRCF_simple_v15"}[wiring]
    m = getattr(CRFP, cls)(device=dev, mid_channels=mid, y_only=y_only, hr_dcn=True, offset_prop=True)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m.storage = storage
    return m.to(dev).eval()


def run_case(wiring, regime, t, h, w, storage="f32", y_only=False, mask="stock", dirty=True, names=None, mid=32):
    """{fetch name: numpy array, "out", "overflowed", "flow_engine"} of one case through the wiring's clip engine (the schedule is the process's).
    "flow_engine": the engine's ``compute_flow`` on the clip's frame pairs."""
    import torch
    sd, lrs, fvs, mks = case(wiring, regime, t, h, w, y_only, mask, mid)
    dev = torch.device("cuda:0")
    with torch.no_grad():
        m = make_model(wiring, sd, storage, y_only, mid)
        eng = m.engine()
        if dirty:
            sc.dirty_workspace(eng, t, h, w)
        L, Fv, M = (torch.from_numpy(a).to(dev) for a in (lrs, fvs, mks))
        out = m(L, Fv, M)
        got = {"out": out.cpu().numpy(), "overflowed": np.array(eng.overflowed())}
        for n in (fetch_names(wiring, t) if names is None else names):
            got[n] = eng.debug_fetch(n, t, h, w).cpu().numpy()
        # FNet alone through the engine's own kernels (crfp_fnet_forward; of the four families only CRFP_DSV's handle exports it): the flow
        # network has no mid_channels and no wiring in it, and steer_fnet's weights are the same for every model
        fm = m if wiring == "dsv" and mid == 32 else make_model("dsv", case("dsv", regime, t, h, w, y_only)[0], storage, y_only)
        got["flow_engine"] = fm.compute_flow(L)[0].cpu().numpy()
    return got


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out")
    ap.add_argument("--wiring", default="cra", help="comma-separated: " + ", ".join(WIRINGS))
    ap.add_argument("--regime", default="large")
    ap.add_argument("--t", type=int, default=3)
    ap.add_argument("--h", type=int, default=33)
    ap.add_argument("--w", type=int, default=47)
    ap.add_argument("--storage", default="f32,bf16")
    ap.add_argument("--mask", default="stock")
    ap.add_argument("--y-only", action="store_true")
    a = ap.parse_args(argv)
    res = {}
    for wiring in a.wiring.split(","):
        for storage in a.storage.split(","):
            for k, v in run_case(wiring, a.regime, a.t, a.h, a.w, storage, a.y_only, a.mask).items():
                res[f"{wiring}:{storage}:{k}"] = v
    np.savez(a.out, **res)
    print("wrote", len(res), "arrays")


if __name__ == "__main__":
    main(sys.argv[1:])
