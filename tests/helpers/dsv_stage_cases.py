"""The stage table of the CRFP_DSV clip engine (``crfp_dsv_forward_batch``, csrc/engine.hip): one row per fetchable workspace buffer of
``Layout`` (W_DSV, one clip) that carries a model tensor -- which oracle tap it equals, which frame of a t-frame clip it holds, whether its
launch is mask-gated, and which schedules of which build write it at all.  tests/test_dsv_stage_cases.py (CPU), tests/test_gpu_dsv_stages.py
(GPU) and tools/bisect_engine.py all read this one table.

Schedules (``SCHEDULES``; the process-wide switches are read once per process, so every schedule but `product` runs in a child process):
    product       the shipped default
    dcn_fused0    CRFP_DCN_FUSED=0: offset / mask head and DCN as two kernels -> `offmask` (and the fp32 build's `om3`) reach HBM
    conv_pair0    CRFP_CONV_PAIR=0: dcn_block.0 / .2 and the residual block's conv1 / conv2 as single launches -> `dcn.fa`, `res.y1`
    mask_gate0    CRFP_MASK_GATE=0: dense fovea-side launches -> `xin8`, `enc_hr0`, `x_hr` hold the whole frame
    lab_unfused   the lab library with CRFP_NARROW_SEQ=0 CRFP_NARROW_CHAIN=0: the 8x chains as single stencils -> `res3.z0` (fp32 build).
                  The lab library links the product's bf16 objects (csrc/Makefile, LAB_OBJS), so the bf16 build has no run-time chain switch:
                  there this schedule is the product's, and the run only extends the census and the bit comparison to that pairing

Where a row's ``live`` rule comes from is its ``line`` (crfp_amd/csrc/engine.hip).  A buffer is *compared* where it is live and holds a
tensor; the fp32 build's `offfeat0..2` are live but hold the producer-split S3 image of the tensor (engine.hip:885), so they are compared in the
bf16 build only; `res3.z1` has no writer in any schedule of either build (fp32: ``res3_pair`` is a constant, engine.hip:628,984; bf16:
``chain_mask()`` is the constant 3, engine.hip:612,620), and the bf16 build never writes `dcn3.g0`, `dcn3.g1`, `res3.z0` for the same reason (the
fp32 build does).  ``UNREACHABLE`` lists these with their reasons; ``NOT_MODEL`` lists the fetchable buffers that carry no model tensor.

Frames.  After a t-frame clip the frame-level buffers hold frame t - 1; the parity sets (`xin8`, `enc_hr0`, `x_hr`, `prop0`, `flow2`, `flow8`)
hold frame t - 1 in set (t - 1) & 1 (`x_hr.1` after t = 2, `x_hr` after t = 3) and frame t - 2 in the other one; `enc_lr0` / `x_lr` hold
every frame, `flow_lr` and FNet's buffers every pair.  Buffers reused across the three 2x levels hold level 2 (`prop_b`: level 1).

Mask-gated rows carry the number of 3x3 convs between them and the fovea blend (`x_hr` 1, `enc_hr0` 2, `xin8` 3): under the gate they are
compared inside the fovea mask dilated by that many pixels -- nothing else is ever read -- and full-frame under mask_gate0.

Bound of the fp32 build against the float64 oracle: ``1e-4 * max(1, max |tap64|)`` per tensor (1e-4: this engine's output bound against the
oracle; the scaling: test_rt_stage_by_stage).  The bound is safe on the reference alone -- max |oracle fp32 - oracle float64| with the same
injected flow, as a share of the bound, worst over frames 1 and 2 of steered_case("large", 3, 33, 47) and ("moderate", 3, 24, 40)
(tests/test_dsv_stage_cases.py asserts <= 0.25 for every tap the table names):

    prevhrw 0.153 (fp32 coordinate rounding at +-480 px)   aligned3 0.063   aligned 0.059   om3:mask 0.043   offmask:masks 0.038
    carryw 0.036   prop_a 0.030   res.y0 0.029   flow_lr 0.028   fnet.g1 0.028   prop_b 0.028   carry 0.024   res3.z0 0.021   feat 0.021
    up 0.019   prev2w 0.017   state_hr 0.014   every other row <= 0.008 (fnet.a0 .. fnet.g0 <= 0.001)
(rows, not taps: `aligned` is level 2's; the levels a row does not hold reach 0.121 on dcn_1.aligned.)

Run as a script it runs one case on the GPU with the workspace filled with 0xFF bytes first and writes the output and every fetchable buffer
of the table, for each storage asked for, to an .npz (keys ``<storage>:<fetch name>``):
    python tests/helpers/dsv_stage_cases.py out.npz [--regime large --t 3 --h 33 --w 47 --storage f32,bf16 --y-only]
"""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BOUND = 1e-4
LAB_LIB = os.path.join(ROOT, "crfp_amd", "libcrfp_hip_lab.so")
BUILDS = ("f32", "bf16")
# name -> (environment of the child process, lab library)
SCHEDULES = collections.OrderedDict([
    ("product", ({}, False)),
    ("dcn_fused0", ({"CRFP_DCN_FUSED": "0"}, False)),
    ("conv_pair0", ({"CRFP_CONV_PAIR": "0"}, False)),
    ("mask_gate0", ({"CRFP_MASK_GATE": "0"}, False)),
    ("lab_unfused", ({"CRFP_NARROW_SEQ": "0", "CRFP_NARROW_CHAIN": "0"}, True)),
])
# the two clips of the GPU tests: ragged in both axes / the geometry of smoke()
CASES = {"large": ("large", 33, 47), "moderate": ("moderate", 24, 40)}

Flags = collections.namedtuple("Flags", "bf16 pair fused gate chain")


def flags(build, sched):
    """What Runner::frame's switches are under a schedule: pair_convs() at these map sizes (engine.hip:534-544: at most 512 tiles -> both pair
    sites on), dcn_fused_enabled(), mask_gate_enabled(), chain_mask() (engine.hip:605-621: shipped 2 in the fp32 build, 3 in the bf16 build; only
    the fp32 objects of the lab library read CRFP_NARROW_CHAIN, its bf16 objects are the product's)."""
    assert build in BUILDS and sched in SCHEDULES, (build, sched)
    bf16 = build == "bf16"
    return Flags(bf16, sched != "conv_pair0", sched != "dcn_fused0", sched != "mask_gate0", 3 if bf16 else (0 if sched == "lab_unfused" else 2))


# buf: fetch name (parity rows: without the ".1");  sel: channels of the fetched NCHW tensor;  tap: (oracle tap, channels of it);
# frames: "last" = frame t - 1, "set" = a parity set (two rows' worth: frame t - 1 and t - 2), "clip" = slot i is frame i, "pairs" = slot n is the
# FNet pass of frame n + 1;  moving: written by frames >= 1 only;  gated: 3x3 convs to the blend (0: not gated);  f32: fp32 in the bf16 build too;
# live / tensor: Flags -> written at all / holds the tensor;  other: the tap a stale level would hold (reused buffers);  state: read by the next frame
Row = collections.namedtuple("Row", "key buf sel tap frames moving gated f32 live tensor line other state")
_always = lambda f: True   # noqa: E731


def _row(key, tap, line, buf=None, sel=None, frames="last", moving=True, gated=0, f32=False, live=_always, tensor=_always, other=None, state=False):
    tap = tap if isinstance(tap, tuple) else (tap, None)
    other = other if other is None or isinstance(other, tuple) else (other, None)
    return Row(key, buf or key, sel, tap, frames, moving, gated, f32, live, tensor, line, other, state)


_FNET = [("a0", 680), ("a1", 682), ("p1", 683), ("b0", 684), ("b1", 685), ("p2", 686), ("c0", 687), ("c1", 688), ("p3", 689), ("d0", 690),
         ("d1", 691), ("u1", 692), ("e0", 693), ("e1", 694), ("u2", 695), ("f0", 696), ("f1", 697), ("u3", 698), ("g0", 699)]
_RGB6 = [0, 1, 2, 4, 5, 6]
_P24 = slice(0, 24)

ROWS = [
    # ---- clip level
    _row("flow_lr", "flow_lr", "702", sel=slice(0, 2), frames="pairs", f32=True),
    _row("enc_lr0", "enc_lr0", "724", frames="clip", moving=False),
    _row("x_lr", "x_lr", "725", frames="clip", moving=False),
] + [_row("fnet." + n, "fnet." + n, str(ln), frames="pairs") for n, ln in _FNET] + [
    _row("fnet.g1", "fnet.g1", "701", sel=slice(0, 2), frames="pairs", f32=True),
    # ---- the two parity sets (state-independent pre-work of a frame, Runner::frame_pre)
    _row("xin8", "xin8", "816 (gate :815)", sel=_RGB6, frames="set", moving=False, gated=3),
    _row("enc_hr0", "enc_hr0", "819", frames="set", moving=False, gated=2),
    _row("x_hr", "x_hr", "820", frames="set", moving=False, gated=1),
    _row("prop0", "prop0", "836", frames="set", moving=False),
    _row("flow2", "flow2", "839", frames="set", f32=True),
    _row("flow8", "flow8", "840", frames="set", f32=True),
    # ---- the recurrent part of the last frame (Runner::frame)
    _row("prev2", "prev2", "846"),
    _row("prev2w", "prev2w", "877"),
    _row("carryw", "carryw", "877"),
    _row("prevhrw", "prevhrw", "878"),
    _row("dcn.fa", "dcn_2.block0", "893 (paired: stays in LDS, :889-891)", live=lambda f: not f.pair, other="dcn_1.block0"),
    _row("dcn.fb", "dcn_2.block2", "891 / 898", other="dcn_1.block2"),
    _row("offfeat0", "dcn_0.block2", "890-891 / 896 (fp32 build: the S3 image, :885)", tensor=lambda f: f.bf16),
    _row("offfeat1", "dcn_1.fuse", "901-902 (fp32 build: the S3 image, :885)", tensor=lambda f: f.bf16),
    _row("offfeat2", "dcn_2.fuse", "901-902 (fp32 build: the S3 image, :885)", tensor=lambda f: f.bf16),
    _row("offmask:offsets", "dcn_2.offset", "917 (fused: stays in registers, :906-915)", buf="offmask", sel=slice(0, 144), f32=True,
         live=lambda f: not f.fused, other="dcn_1.offset"),
    _row("offmask:masks", "dcn_2.mask", "917 (fused: stays in registers, :906-915)", buf="offmask", sel=slice(144, 216), f32=True,
         live=lambda f: not f.fused, other="dcn_1.mask"),
    _row("aligned", "dcn_2.aligned", "914 / 919", other="dcn_1.aligned"),
    _row("res.y0", "forward_resblocks_2.main0", "931", other="forward_resblocks_1.main0"),
    _row("res.y1", "forward_resblocks_2.conv1", "769 (paired: stays in LDS, :766-767)", live=lambda f: not f.pair, other="forward_resblocks_1.conv1"),
    _row("prop_a", ("res2", _P24), "763 (level 2: :932-934)", other=("res0", _P24)),
    _row("prop_b", ("res1", _P24), "763 (level 1: :932-934)"),
    _row("up", "up", "938"),
    _row("poff", "dcn_3.pre_offset", "938", state=True),
    _row("dcn3.g0", "dcn_3.block0", "945 (chained: :941-943)", live=lambda f: not f.chain & 1),
    _row("dcn3.g1", "dcn_3.block2", "946 (chained: :941-943)", live=lambda f: not f.chain & 1),
    _row("dcn3.g2", "dcn_3.fuse", "943 / 947"),
    _row("om3:offset", ("dcn_3.offset", slice(0, 2)), "957 (fp32 build, fused: inside dcn3_kernel, :952-955)", buf="om3", sel=slice(0, 2), f32=True,
         live=lambda f: f.bf16 or not f.fused),
    _row("om3:mask", ("dcn_3.mask", slice(0, 1)), "957 (fp32 build, fused: inside dcn3_kernel, :952-955)", buf="om3", sel=slice(2, 3), f32=True,
         live=lambda f: f.bf16 or not f.fused),
    _row("aligned3", "dcn_3.aligned", "955 / 958"),
    _row("res3.z0", "forward_resblocks_3.main0", "967 (chained: :982-983)", live=lambda f: not f.chain & 2),
    _row("res3.z1", "forward_resblocks_3.conv1", "987 (chained: :982-983; fp32 build: paired, :628,984-985)", live=lambda f: not f.chain & 2 and f.bf16),
    _row("feat", "feat", "983 / 985 / 988"),
    # ---- what only the next frame reads
    _row("state_hr", "state_hr", "991 (away from the fovea: :981-983 / 990)", moving=False, state=True),
    _row("carry", "carry", "763 (:932)", moving=False, state=True),
]

UNREACHABLE = {
    ("f32", "offfeat0"): "the fp32 build keeps dcn_0's block.2 output as the producer-split S3 image (engine.hip:885); a Q4 tensor only under "
                         "CRFP_PRECISION=f32, which is none of the schedules here.  Compared in the bf16 build.",
    ("f32", "offfeat1"): "as offfeat0 (dcn_1's conv_fuse output).  Compared in the bf16 build.",
    ("f32", "offfeat2"): "as offfeat0 (dcn_2's conv_fuse output).  Compared in the bf16 build.",
    ("f32", "res3.z1"): "no schedule of the fp32 build writes it: res3's conv1 -> conv2 pair is a compile-time constant (res3_pair, "
                        "engine.hip:628,984-985).  Not compared in either build.",
    ("bf16", "res3.z1"): "the bf16 build runs forward_resblocks_3 as one chained launch in every schedule: chain_mask() is the constant 3 in the "
                         "product objects (engine.hip:612,620), and the lab library links those (csrc/Makefile, LAB_OBJS).  Not compared in either build.",
    ("bf16", "res3.z0"): "as res3.z1 of the bf16 build (chain bit 1).  Compared in the fp32 build (lab_unfused).",
    ("bf16", "dcn3.g0"): "the bf16 build runs dcn_3's block.0 -> .2 -> conv_fuse as one chained launch in every schedule (chain bit 0, constant: "
                         "engine.hip:612,620,941-943).  Compared in the fp32 build (every schedule).",
    ("bf16", "dcn3.g1"): "as dcn3.g0 of the bf16 build.  Compared in the fp32 build (every schedule).",
}
# fetchable buffers of Layout (W_DSV, t > 1) that carry no model tensor
NOT_MODEL = {"status": "status words", "lr_q4": "the LR input frames repacked as quads (fp32 build)", "gate": "mask-gate flag bytes",
             "gate.1": "mask-gate flag bytes"}


def tap_of(taps, spec):
    name, sel = spec
    x = taps[name]
    return x if sel is None else x[:, sel]


def rows_for(build, sched, compared_only=True):
    f = flags(build, sched)
    return [r for r in ROWS if r.live(f) and (r.tensor(f) or not compared_only)]


def fetch_name(buf, par):
    return buf + (".1" if par else "")


def slots(row, t):
    """[(fetch name, index into the fetched batch axis, frame whose tap it holds)] of a row after a t-frame clip (t >= 2)."""
    last = t - 1
    if row.frames == "last":
        return [(row.buf, 0, last)]
    if row.frames == "set":
        return [(fetch_name(row.buf, i & 1), 0, i) for i in (last, last - 1) if i >= (1 if row.moving else 0)]
    if row.frames == "clip":
        return [(row.buf, i, i) for i in range(t)]
    return [(row.buf, i - 1, i) for i in range(1, t)]      # pairs


def fetch_names(t):
    """Every fetch name the table touches after a t-frame clip, written or not (the census reads them all)."""
    out = []
    for r in ROWS:
        for n in ([fetch_name(r.buf, 0), fetch_name(r.buf, 1)] if r.frames == "set" else [r.buf]):
            if n not in out:
                out.append(n)
    return out


def written_names(build, sched, t):
    """Fetch names that hold anything after a t-frame clip under the schedule -- the census' expectation."""
    live = rows_for(build, sched, compared_only=False)
    return sorted({name for r in live for name, _, _ in slots(r, t)})


def dilate(mk, k):
    """Bool mask [H, W] grown by k pixels in the Chebyshev metric: what k 3x3 convs in front of a masked read can reach."""
    m = np.asarray(mk, bool)
    for _ in range(k):
        p = np.pad(m, 1)
        m = np.zeros_like(m)
        for dy in range(3):
            for dx in range(3):
                m |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return m


def region(row, f, mk):
    """Where a row's buffer must hold its tensor: None = everywhere; gated rows under the gate = the fovea mask `mk` [8h, 8w] of the buffer's
    frame, dilated by the row's distance to the blend."""
    return dilate(mk, row.gated) if (row.gated and f.gate) else None


def bound_of(tap64):
    return BOUND * max(1.0, float(np.abs(np.asarray(tap64, np.float64)).max()))


# ----------------------------------------------------------------------------- the oracle, tapped frame by frame
def oracle_taps(orc, sd, lrs, fvs, mks, flows=None, double=False, bf16=False, y_only=False):
    """[taps of frame 0, ..., taps of frame t - 1] (plus "out"; frames >= 1 also carry "flow_lr" and FNet's "fnet.*" of their pair, from the
    oracle's own flow network) of ``orc.dsv_frame`` run frame by frame.  flows [1, t - 1, 2, h, w]: the flow to inject (None: the oracle's
    own).  double: float64 oracle; bf16: the storage twin (``bf16_storage`` + ``bf16_weights``)."""
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
    cfg = orc.DSVConfig(y_only=y_only)
    ftaps = {}
    with torch.no_grad(), (orc.bf16_storage() if bf16 else contextlib.nullcontext()):
        with orc.tapping(ftaps):
            own = orc.compute_flow(P, L)
        ftaps["flow_lr"] = own[0]
        flows = own if flows is None else torch.as_tensor(flows).to(dt)
        st = orc.new_state(cfg, n, h, w, L)
        per = []
        for i in range(t):
            taps = {}
            with orc.tapping(taps):
                out, st = orc.dsv_frame(P, cfg, st, L[:, i], Fv[:, i], M[:, i], flows[:, i - 1] if i else None)
            taps["out"] = out
            if i:
                taps.update({k: v[i - 1:i] for k, v in ftaps.items()})
            per.append(taps)
    return per


# ----------------------------------------------------------------------------- the engine: one case, every buffer of the table
def make_model(sd, storage="f32", y_only=False, cls="CRFP_DSV"):
    import torch
    from crfp_amd.model import CRFP
    dev = torch.device("cuda:0")
    m = getattr(CRFP, cls)(device=dev, mid_channels=32, y_only=y_only, hr_dcn=True, offset_prop=True)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m.storage = storage
    return m.to(dev).eval()


def dirty_workspace(eng, t, h, w, n=1):
    """Fill the clip workspace the next forward() of this geometry uses with 0xFF bytes (NaN in fp32 and in bf16)."""
    eng._workspace(t, h, w, n).fill_(0xFF)


def run_case(regime, t, h, w, storage="f32", y_only=False, dirty=True, names=None):
    """{fetch name: numpy array, "out": ...} of one steered clip through the clip engine (the schedule is the process's)."""
    import torch
    from helpers import motion_cases as mc
    sd, lrs, fvs, mks = mc.steered_case(regime, t, h, w, y_only=y_only)
    dev = torch.device("cuda:0")
    with torch.no_grad():
        m = make_model(sd, storage, y_only)
        eng = m.engine()
        if dirty:
            dirty_workspace(eng, t, h, w)
        out = m(*(torch.from_numpy(a).to(dev) for a in (lrs, fvs, mks)))
        got = {"out": out.cpu().numpy(), "overflowed": np.array(eng.overflowed())}
        for n in (fetch_names(t) if names is None else names):
            got[n] = eng.debug_fetch(n, t, h, w).cpu().numpy()
    return got


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out")
    ap.add_argument("--regime", default="large")
    ap.add_argument("--t", type=int, default=3)
    ap.add_argument("--h", type=int, default=33)
    ap.add_argument("--w", type=int, default=47)
    ap.add_argument("--storage", default="f32,bf16")
    ap.add_argument("--y-only", action="store_true")
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    res = {}
    for storage in a.storage.split(","):
        for k, v in run_case(a.regime, a.t, a.h, a.w, storage, a.y_only).items():
            res[f"{storage}:{k}"] = v
    np.savez(a.out, **res)
    print("wrote", len(res), "arrays")


if __name__ == "__main__":
    main(sys.argv[1:])
