"""Bisect the engine against the oracle: run a t-frame clip, fetch the workspace buffers the active schedule writes
(crfp_dsv_debug_fetch; which those are: the stage table of tests/helpers/dsv_stage_cases.py) and print max / mean |delta| per tensor
against the oracle's taps of the same frame, run with the engine's own flow.
  python tools/bisect_engine.py [--storage bf16] [--h 24 --w 40] [--t 2]
  CRFP_DCN_FUSED=0 python tools/bisect_engine.py --schedule dcn_fused0       another schedule: its switches go into the environment
  python tools/bisect_engine.py --wiring cra|simple|dense [--storage bf16] [--t 3]   the other clip wirings (crfp_cra_ / crfp_simple_ /
        crfp_dense_debug_fetch; the tables of tests/helpers/wiring_stage_cases.py; schedules product | unfused: CRFP_DCN_FUSED=0 CRFP_CONV_PAIR=0)
  python tools/bisect_engine.py --rt [--h 24 --w 40 --fv 64 --warp 128 192]    the regional runtime engine (crfp_rt_debug_fetch)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crfp_amd import synth  # noqa: E402
from oracle import crfp_oracle as orc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--storage", default="f32")
ap.add_argument("--h", type=int, default=24)
ap.add_argument("--w", type=int, default=40)
ap.add_argument("--fv", type=int, default=64)
ap.add_argument("--t", type=int, default=2, help="frames of the clip: the buffers hold frame t - 1 (parity set (t - 1) & 1)")
ap.add_argument("--schedule", default="product", help="the schedule the environment selects (tests/helpers/dsv_stage_cases.py, SCHEDULES): "
                "decides which buffers are live")
ap.add_argument("--wiring", default="dsv", choices=("dsv", "cra", "simple", "dense"), help="the clip engine's wiring: CRFP_DSV, or CRFP_DSV_CRA / "
                "CRFP_simple / CRFP through their own debug fetch and stage table (tests/helpers/wiring_stage_cases.py)")
ap.add_argument("--rt", action="store_true", help="the regional runtime engine (crfp_rt_debug_fetch) instead of CRFP_DSV")
ap.add_argument("--warp", type=int, nargs=2, default=(128, 192), help="--rt: warp_size")
a = ap.parse_args()
T = torch.from_numpy
dev = torch.device("cuda:0")


def show(name, got, want):
    got, want = got.float().cpu(), want.float()
    if got.shape != want.shape:
        print(f"{name:24s} SHAPE {tuple(got.shape)} vs {tuple(want.shape)}")
        return
    d = (got - want).abs()
    print(f"{name:24s} max {float(d.max()):.3e} mean {float(d.mean()):.3e}  (|ref| max {float(want.abs().max()):.2e})")


if a.rt:   # frame 1 of a 2-frame clip: every fetch name against the fp32 oracle's tap, run with the engine's own flow
    from crfp_amd.model import MRCF_runtime
    from oracle import runtime_oracle as ro
    m = MRCF_runtime.MRCF_simple_v18(dev, mid_channels=32)
    sd = synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, 3)
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    rs = np.random.RandomState(5)
    lrs, fvs = T(rs.rand(1, 2, 3, a.h, a.w).astype(np.float32)), T(rs.rand(1, 2, 3, a.fv, a.fv).astype(np.float32))
    with torch.no_grad():
        out = m(lrs.to(dev), fvs.to(dev), warp_size=tuple(a.warp)).cpu()
        eng = m.engine()
        taps = {}
        ref = ro.runtime_forward(orc.load_numpy_state(sd), lrs, fvs, tuple(a.warp), flows=eng.debug_fetch("flow_lr")[None, :, :2].cpu(), taps=taps)
    for n in ("x_lr", "x_hr", "flow2", "flow8", "win", "upw", "state_w", "prev2w", "prev2", "carryw", "offfeat0", "aligned0", "offfeat1", "aligned1",
              "offfeat2", "aligned2", "poff", "al3", "carry", "feat2", "state"):
        show(n, eng.debug_fetch(n), taps[n])
    show("out frame 0", out[:, 0], ref[:, 0])
    show("out frame 1", out[:, 1], ref[:, 1])
    sys.exit(0)

# The clip engine: the stage table of tests/helpers/dsv_stage_cases.py says which buffers the active schedule of this build writes, which oracle
# tap each equals and where (mask-gated buffers: inside the fovea mask dilated by their distance to the blend) -- nothing else is printed.
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import dsv_stage_cases as sc  # noqa: E402

if a.wiring != "dsv":   # the wiring's own table, weights of its own shapes, the same walk
    from helpers import wiring_stage_cases as wc  # noqa: E402
    sched, build, wiring = a.schedule, "bf16" if a.storage == "bf16" else "f32", a.wiring
    for k, v in wc.SCHEDULES[sched].items():
        if os.environ.get(k) != v:
            sys.exit(f"--schedule {sched} needs {k}={v} in the environment (the library reads it once)")
    sd = synth.make_state_dict_like(wc.shapes(wiring), wc.WEIGHTS_SEED)
    t, h, w = a.t, a.h, a.w
    lrs, fvs, mks = synth.make_clip(3, 1, t, h, w, fv_size=a.fv)
    m = wc.make_model(wiring, sd, a.storage)
    with torch.no_grad():
        sc.dirty_workspace(m.engine(), t, h, w)
        out = m(lrs=T(lrs).to(dev), fvs=T(fvs).to(dev), mks=T(mks).to(dev)).cpu()
        eng = m.engine()
        flows = eng.debug_fetch("flow_lr", t, h, w)[:, :2].cpu()[None]
        refs = wc.oracle_taps(orc, wiring, sd, lrs, fvs, mks, flows=flows, bf16=build == "bf16")
    f = wc.flags(wiring, build, sched)
    print(f"{wiring}: {build} build, schedule {sched}, frame {t - 1} of a {t}-frame clip {h} x {w}; not written under this schedule: "
          + " ".join(n for n in wc.fetch_names(wiring, t) if n not in wc.written_names(wiring, build, sched, t)))
    for r in wc.rows_for(wiring, build, sched):
        for name, idx, frame in wc.slots(r, t):
            got = eng.debug_fetch(name, t, h, w)[idx:idx + 1].cpu()
            got = got if r.sel is None else got[:, r.sel]
            want = wc.tap_of(refs[frame], r.tap)
            reg = wc.region(r, f, mks[0, frame, 0])
            if reg is not None:
                keep = T(reg)[None, None]
                got, want = torch.where(keep, got, torch.zeros(())), torch.where(keep, want, torch.zeros(()))
            show(f"{r.key} [{name}, frame {frame}]", got, want)
    for i in range(t):
        show(f"out frame {i}", out[:, i], refs[i]["out"])
    sys.exit(0)

sched = a.schedule
for k, v in sc.SCHEDULES[sched][0].items():
    if os.environ.get(k) != v:
        sys.exit(f"--schedule {sched} needs {k}={v} in the environment (the library reads it once)" + (" and CRFP_HIP_LIB=" + sc.LAB_LIB if sc.SCHEDULES[sched][1] else ""))
build = "bf16" if a.storage == "bf16" else "f32"
sd = synth.make_state_dict(7)
t, h, w = a.t, a.h, a.w
lrs, fvs, mks = synth.make_clip(3, 1, t, h, w, fv_size=a.fv)
m = sc.make_model(sd, a.storage)
with torch.no_grad():
    sc.dirty_workspace(m.engine(), t, h, w)     # what is not written reads as NaN
    out = m(lrs=T(lrs).to(dev), fvs=T(fvs).to(dev), mks=T(mks).to(dev)).cpu()
    eng = m.engine()
    flows = eng.debug_fetch("flow_lr", t, h, w)[:, :2].cpu()[None]
    refs = sc.oracle_taps(orc, sd, lrs, fvs, mks, flows=flows, bf16=build == "bf16")      # the engine's own flow, injected
f = sc.flags(build, sched)
print(f"{build} build, schedule {sched}, frame {t - 1} of a {t}-frame clip {h} x {w}; not written under this schedule: "
      + " ".join(n for n in sc.fetch_names(t) if n not in sc.written_names(build, sched, t)))
for r in sc.rows_for(build, sched):
    for name, idx, frame in sc.slots(r, t):
        got = eng.debug_fetch(name, t, h, w)[idx:idx + 1].cpu()
        got = got if r.sel is None else got[:, r.sel]
        want = sc.tap_of(refs[frame], r.tap)
        reg = sc.region(r, f, mks[0, frame, 0])
        if reg is not None:     # outside the region the gated launches wrote nothing anybody reads
            keep = T(reg)[None, None]
            got, want = torch.where(keep, got, torch.zeros(())), torch.where(keep, want, torch.zeros(()))
        show(f"{r.key} [{name}, frame {frame}]", got, want)
for i in range(t):
    show(f"out frame {i}", out[:, i], refs[i]["out"])
