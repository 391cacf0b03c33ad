"""GPU (-m gpu): every stage of the CRFP_DSV clip engine (``crfp_dsv_forward_batch``, csrc/engine.hip) against the float64 oracle.

The rest of the suite holds this engine to its output frames.  Here every workspace buffer that carries a model tensor is read back
(``crfp_dsv_debug_fetch``) and compared with the oracle's tap of the same tensor, following the one table of tests/helpers/dsv_stage_cases.py
(which buffer equals which tap, which frame it holds, which schedules of which build write it; tests/test_dsv_stage_cases.py checks the table
against the oracle alone).  The clips are ``steered_case("large", t, 33, 47)`` and ``("moderate", t, 24, 40)`` with t = 2 (frame 1, the first
moving frame, in parity set .1) and t = 3 (frame 2, the first frame with a full recurrent state, in set 0); every test asserts the regime on the
flow it fetched, and the oracle runs frame by frame with that flow injected.  The workspace is filled with 0xFF bytes before every run.

(a) fp32 build, product schedule: every live buffer against the float64 tap, bound 1e-4 * max(1, max |tap64|) per tensor; the next frame's
    state (`carry`, `state_hr`, `poff`) included.  Mask-gated buffers (`xin8`, `enc_hr0`, `x_hr`) inside the fovea mask dilated by their
    distance to the blend.
(b) the other schedules in four child processes (the large clip, t = 3, both builds per child): the buffers only they write against the same
    taps under the same bound; every buffer live in a child and in the product run is bit-equal between the two.
(c) census: after a run on a 0xFF workspace the buffers holding any non-NaN value are exactly the table's written set of that schedule and build;
    written tensors hold no NaN (gated ones: inside their dilated mask).
(d) a 0xFF-filled workspace gives the bits of a fresh one: clip engine in both storages and both stream schedules, n = 2 lock-step, and the
    one-frame-per-call model (MRCF_simple_v18, three calls).
(e) bf16 build: the same live buffers against the storage twin's taps (``bf16_storage`` + ``bf16_weights``, injected flow), per stage by the
    yardstick of test_gpu_bf16.py: mean |HIP - twin| <= 0.75 mean |twin - fp32 oracle| and max <= 1.5 max, both right-hand sides from the
    reference alone.  `flow2` / `flow8` are fp32 functions of the injected flow in the twin and in the fp32 oracle alike -- the right-hand side is
    exactly zero -- so they are held to the fp32 bound of (a) against the twin instead.  Per-stage factors other than (0.75, 1.5): BF16_FACTORS.

Measured on an MI355X (both clips; the output frames sit 0.9e-6 .. 2.1e-6 from the float64 oracle).  No stage came near its bound -- the worst
fp32 share is 0.18 (`prevhrw`, moderate clip, frame 2: 2.5e-5 of 1.4e-4; the fp32 oracle itself is 0.15 there) -- and every bf16 stage meets the
default factors (worst mean ratio 0.64 on `up`, worst max ratio 1.32 on `prop_b`), so BF16_FACTORS is empty.  Every buffer live in a child run
and in the product run (81 fetches per build and schedule) is bit-equal between the two, and a 0xFF workspace never changed a bit.  The census
found one disagreement with the table as first written, in the table: the lab library's bf16 objects are the product's, so
CRFP_NARROW_CHAIN=0 unchains nothing in the bf16 build (`dcn3.g0`, `dcn3.g1`, `res3.z0`, `res3.z1` stay untouched there).  No defect in the engine.

Census (t = 3; t = 2 the same plus `flow2` / `flow8` of set 0, which frame 0 does not write): buffers of the table left untouched
    schedule      fp32 build                                    bf16 build
    product       dcn.fa offmask res.y1 om3 res3.z0 res3.z1     dcn.fa offmask res.y1 dcn3.g0 dcn3.g1 res3.z0 res3.z1
    dcn_fused0    dcn.fa res.y1 res3.z0 res3.z1                 dcn.fa res.y1 dcn3.g0 dcn3.g1 res3.z0 res3.z1
    conv_pair0    offmask om3 res3.z0 res3.z1                   offmask dcn3.g0 dcn3.g1 res3.z0 res3.z1
    mask_gate0    as product                                    as product
    lab_unfused   dcn.fa offmask res.y1 om3 res3.z1             as product

fp32 build, product schedule, last frame of the t = 2 (f1) and t = 3 (f2) clips: max |HIP - tap64| (max |tap64|), bound 1e-4 * max(1, max |tap64|):

    row              large f1              large f2              moderate f1           moderate f2
    flow_lr          1.02e-04 (57.7)       1.07e-04 (57.9)       1.10e-04 (23.6)       1.05e-04 (23.6)
    enc_lr0          2.93e-07 (1.37)       2.27e-07 (1.27)       2.65e-07 (1.26)       2.47e-07 (1.23)
    x_lr             5.22e-07 (1.3)        5.32e-07 (1.38)       5.26e-07 (1.18)       4.97e-07 (1.15)
    fnet.a0          5.96e-08 (0.79)       5.96e-08 (0.811)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.a1          5.96e-08 (0.79)       5.96e-08 (0.811)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.p1          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.b0          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.b1          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.p2          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.c0          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.c1          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.p3          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.d0          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.d1          5.96e-08 (0.79)       5.96e-08 (0.731)      5.96e-08 (0.676)      5.96e-08 (0.677)
    fnet.u1          7.64e-08 (0.752)      7.64e-08 (0.71)       7.45e-08 (0.675)      8.01e-08 (0.66)
    fnet.e0          8.94e-08 (0.752)      1.23e-07 (0.71)       1.06e-07 (0.675)      1.19e-07 (0.66)
    fnet.e1          8.94e-08 (0.752)      1.23e-07 (0.71)       1.06e-07 (0.675)      1.19e-07 (0.66)
    fnet.u2          1.07e-07 (0.735)      1.25e-07 (0.7)        1.08e-07 (0.675)      1.33e-07 (0.654)
    fnet.f0          1.49e-07 (0.735)      1.29e-07 (0.7)        1.45e-07 (0.675)      1.33e-07 (0.654)
    fnet.f1          1.49e-07 (0.735)      1.29e-07 (0.7)        1.45e-07 (0.675)      1.33e-07 (0.654)
    fnet.u3          1.50e-07 (0.734)      1.36e-07 (0.699)      1.40e-07 (0.675)      1.43e-07 (0.654)
    fnet.g0          1.66e-07 (0.734)      1.62e-07 (0.699)      1.67e-07 (0.675)      1.75e-07 (0.654)
    fnet.g1          1.24e-04 (57.7)       1.08e-04 (57.9)       1.10e-04 (23.6)       1.05e-04 (23.6)
    xin8             8.09e-08 (1)          5.61e-08 (1)          7.28e-08 (1)          7.32e-08 (1)
    enc_hr0          6.05e-07 (1.68)       7.24e-07 (1.76)       5.20e-07 (1.71)       5.58e-07 (1.54)
    x_hr             7.51e-07 (1.46)       8.65e-07 (1.61)       7.11e-07 (1.53)       7.77e-07 (1.45)
    prop0            5.82e-07 (1.45)       5.43e-07 (1.37)       5.39e-07 (1.34)       4.60e-07 (1.3)
    flow2            1.48e-05 (115)        1.43e-05 (116)        4.05e-06 (47.1)       4.53e-06 (47.1)
    flow8            6.16e-05 (462)        5.19e-05 (464)        2.64e-05 (189)        2.45e-05 (189)
    prev2            9.44e-07 (2.3)        1.08e-06 (2.36)       1.26e-06 (2.34)       1.39e-06 (2.42)
    prev2w           3.67e-06 (2.2)        4.26e-06 (2.33)       2.71e-06 (2.2)        4.94e-06 (2.23)
    carryw           3.34e-06 (0.52)       3.03e-06 (0.723)      3.45e-06 (0.537)      3.11e-06 (0.756)
    prevhrw          2.04e-05 (1.44)       1.45e-05 (1.42)       1.67e-05 (1.57)       2.55e-05 (1.43)
    dcn.fb           1.56e-05 (29.4)       1.52e-05 (21.7)       5.40e-06 (13)         6.87e-06 (14.1)
    aligned          1.31e-05 (1.43)       7.00e-06 (1.43)       5.07e-06 (1.6)        4.74e-06 (1.67)
    res.y0           3.40e-06 (0.794)      2.13e-06 (0.781)      1.86e-06 (0.798)      1.80e-06 (0.872)
    prop_a           3.28e-06 (0.795)      2.11e-06 (0.791)      1.85e-06 (0.795)      1.66e-06 (0.926)
    prop_b           2.52e-06 (0.641)      2.53e-06 (1.02)       2.57e-06 (0.699)      1.88e-06 (0.803)
    up               2.74e-06 (0.646)      1.71e-06 (0.647)      1.46e-06 (0.702)      1.18e-06 (0.766)
    poff             3.94e-05 (59.1)       3.43e-05 (57.7)       1.25e-05 (19.9)       1.22e-05 (20.2)
    dcn3.g0          7.00e-05 (319)        6.94e-05 (346)        2.58e-05 (132)        2.28e-05 (107)
    dcn3.g1          8.71e-05 (174)        1.11e-04 (238)        3.89e-05 (81.2)       2.67e-05 (76.8)
    dcn3.g2          8.21e-05 (140)        7.61e-05 (131)        2.57e-05 (42.5)       3.07e-05 (49.2)
    aligned3         8.84e-06 (1.06)       8.38e-07 (0.565)      3.07e-06 (0.722)      5.91e-06 (0.787)
    feat             3.01e-06 (0.679)      1.15e-06 (0.555)      1.66e-06 (0.686)      2.55e-06 (0.739)
    state_hr         3.01e-06 (1.46)       1.15e-06 (1.47)       1.66e-06 (1.48)       2.55e-06 (1.45)
    carry            1.95e-06 (0.952)      2.38e-06 (0.881)      2.31e-06 (0.997)      1.79e-06 (0.824)

bf16 build, product schedule, same frames: mean |HIP - twin| / mean |twin - fp32 oracle| and max / max (asserted <= 0.75 and <= 1.5;
`abs`: max |HIP - twin| of a tensor the twin and the fp32 oracle share exactly, held to the fp32 bound):

    row              large f1        large f2        moderate f1     moderate f2
    flow_lr          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    enc_lr0          0.00 / 0.03     0.00 / 0.20     0.00 / 0.00     0.00 / 0.00
    x_lr             0.00 / 0.13     0.00 / 0.33     0.00 / 0.00     0.00 / 0.00
    fnet.a0          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.a1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.p1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.b0          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.b1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.p2          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.c0          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.c1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.p3          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.d0          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.d1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.u1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.e0          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.e1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.u2          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.f0          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.f1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.u3          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.g0          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    fnet.g1          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    xin8             0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    enc_hr0          0.00 / 0.00     0.00 / 0.00     0.00 / 0.00     0.00 / 0.00
    x_hr             0.00 / 0.00     0.00 / 0.10     0.00 / 0.00     0.00 / 0.00
    prop0            0.00 / 0.55     0.00 / 0.62     0.00 / 0.24     0.00 / 0.28
    flow2            1.5e-05 abs     1.5e-05 abs     3.8e-06 abs     3.8e-06 abs
    flow8            6.1e-05 abs     6.1e-05 abs     3.1e-05 abs     3.1e-05 abs
    prev2            0.17 / 0.78     0.49 / 0.51     0.12 / 0.65     0.52 / 1.25
    prev2w           0.15 / 0.74     0.47 / 0.52     0.14 / 0.70     0.43 / 0.69
    carryw           0.01 / 0.27     0.33 / 0.65     0.02 / 0.22     0.32 / 0.22
    prevhrw          0.06 / 0.77     0.41 / 0.54     0.08 / 0.70     0.34 / 0.65
    dcn.fb           0.03 / 0.75     0.04 / 0.81     0.12 / 0.90     0.12 / 0.73
    offfeat0         0.01 / 0.74     0.02 / 0.57     0.04 / 0.82     0.08 / 0.79
    offfeat1         0.07 / 0.79     0.07 / 0.61     0.17 / 0.49     0.20 / 0.85
    offfeat2         0.12 / 0.35     0.13 / 0.40     0.26 / 0.45     0.27 / 0.87
    aligned          0.50 / 0.82     0.54 / 0.65     0.57 / 0.83     0.62 / 0.60
    res.y0           0.44 / 0.56     0.45 / 0.73     0.50 / 0.57     0.59 / 0.59
    prop_a           0.44 / 0.46     0.46 / 0.75     0.51 / 0.63     0.60 / 0.60
    prop_b           0.27 / 0.50     0.36 / 1.32     0.34 / 0.33     0.47 / 0.66
    up               0.49 / 0.75     0.49 / 0.66     0.55 / 0.63     0.64 / 0.73
    poff             0.20 / 0.65     0.21 / 0.79     0.37 / 0.76     0.39 / 0.78
    dcn3.g2          0.08 / 0.38     0.07 / 0.73     0.12 / 0.42     0.13 / 0.64
    om3:offset       0.27 / 0.49     0.21 / 0.39     0.31 / 0.70     0.41 / 0.58
    om3:mask         0.27 / 0.19     0.45 / 0.42     0.19 / 0.13     0.35 / 0.26
    aligned3         0.27 / 0.67     0.05 / 0.46     0.30 / 0.64     0.35 / 0.57
    feat             0.49 / 0.39     0.50 / 0.65     0.55 / 0.82     0.63 / 0.42
    state_hr         0.43 / 0.39     0.43 / 0.86     0.45 / 0.82     0.53 / 0.61
    carry            0.25 / 0.97     0.30 / 1.17     0.29 / 0.33     0.42 / 0.65

The other schedules (large clip, t = 3; frame 2 unless noted), the buffers only they write:

    f32  dcn_fused0  offmask:offsets  offmask frame 2     9.49e-05 (126)
    f32  dcn_fused0  offmask:masks    offmask frame 2     4.31e-06 (1)
    f32  dcn_fused0  om3:offset       om3 frame 2         2.07e-04 (454)
    f32  dcn_fused0  om3:mask         om3 frame 2         6.52e-07 (0.914)
    bf16 dcn_fused0  offmask:offsets  offmask frame 2     0.29 / 0.35
    bf16 dcn_fused0  offmask:masks    offmask frame 2     0.29 / 0.43
    f32  conv_pair0  dcn.fa           dcn.fa frame 2      1.19e-05 (37.6)
    f32  conv_pair0  res.y1           res.y1 frame 2      3.93e-07 (0.181)
    bf16 conv_pair0  dcn.fa           dcn.fa frame 2      0.01 / 0.64
    bf16 conv_pair0  res.y1           res.y1 frame 2      0.49 / 0.69
    f32  mask_gate0  xin8             xin8 frame 2        9.31e-08 (1)
    f32  mask_gate0  xin8             xin8.1 frame 1      8.96e-08 (1)
    f32  mask_gate0  enc_hr0          enc_hr0 frame 2     7.24e-07 (1.76)
    f32  mask_gate0  enc_hr0          enc_hr0.1 frame 1   6.40e-07 (1.68)
    f32  mask_gate0  x_hr             x_hr frame 2        8.65e-07 (1.61)
    f32  mask_gate0  x_hr             x_hr.1 frame 1      9.73e-07 (1.46)
    bf16 mask_gate0  xin8             xin8 frame 2        0.00 / 0.00
    bf16 mask_gate0  xin8             xin8.1 frame 1      0.00 / 0.00
    bf16 mask_gate0  enc_hr0          enc_hr0 frame 2     0.00 / 0.00
    bf16 mask_gate0  enc_hr0          enc_hr0.1 frame 1   0.00 / 0.00
    bf16 mask_gate0  x_hr             x_hr frame 2        0.00 / 0.09
    bf16 mask_gate0  x_hr             x_hr.1 frame 1      0.00 / 0.00
    f32  lab_unfused res3.z0          res3.z0 frame 2     1.12e-06 (0.545)

Large-motion timing of this engine is not measured here or anywhere else."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import dsv_stage_cases as sc
from helpers import motion_cases as mc

pytestmark = pytest.mark.gpu

T = torch.from_numpy
RUNS = [("large", 2, 33, 47), ("large", 3, 33, 47), ("moderate", 2, 24, 40), ("moderate", 3, 24, 40)]
CHILD = ("large", 3, 33, 47)
# bf16 build, per row key: (mean factor, max factor) where the default (0.75, 1.5) is missed without a defect -- measured value x 2, never above
# 1.0 x the twin's mean distance to the fp32 oracle (see the module docstring's table)
BF16_FACTORS = {}
BF16_DEFAULT = (0.75, 1.5)


@pytest.fixture(scope="module")
def orc():
    from oracle import crfp_oracle
    return crfp_oracle


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def _case(regime, t, h, w, y_only=False):
    return mc.steered_case(regime, t, h, w, y_only=y_only)


@functools.lru_cache(maxsize=None)
def _run(regime, t, h, w, storage="f32", y_only=False):
    """The product schedule in this process, on a 0xFF workspace: the output and every buffer of the table."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    got = sc.run_case(regime, t, h, w, storage, y_only)
    assert not bool(got["overflowed"])
    return got


def _flows(got):
    return T(got["flow_lr"][:, :2].copy())[None]        # [1, t - 1, 2, h, w]; channels 2, 3 of the quad are padding


@functools.lru_cache(maxsize=None)
def _ref(regime, t, h, w, kind, storage="f32", y_only=False):
    """Oracle taps per frame with the flow the `storage` engine fetched: kind "f64" / "f32" / "twin"."""
    from oracle import crfp_oracle
    sd, lrs, fvs, mks = _case(regime, t, h, w, y_only)
    return sc.oracle_taps(crfp_oracle, sd, lrs, fvs, mks, flows=_flows(_run(regime, t, h, w, storage, y_only)), double=kind == "f64",
                          bf16=kind == "twin", y_only=y_only)


def _assert_regime(got, regime, h, w, what):
    s = mc.flow_stats(_flows(got), h, w)
    print(f"{what}: engine flow {mc.fmt_stats(s)}")
    mc.assert_regime(s, regime)


def _pick(got, row, name, idx, reg):
    """The row's tensor out of a fetched buffer, as float64 [1, C, H, W] (flow2 / flow8: [1, H, W, 2]), and the boolean region to read."""
    x = got[name][idx:idx + 1]
    if row.sel is not None:
        x = x[:, row.sel]
    x = x.astype(np.float64)
    where = np.ones(x.shape, bool) if reg is None else np.broadcast_to(reg[None, None], x.shape)
    return x, where


def _compare(got, build, sched, t, refs, mks, rows, what, refs32=None):
    """Every slot of `rows`: fp32 build against the float64 taps under the bound; bf16 build against the twin's taps by the per-stage yardstick
    (refs = twin, refs32 = fp32 oracle).  Prints every figure, then asserts."""
    f = sc.flags(build, sched)
    bad = []
    for r in rows:
        for name, idx, frame in sc.slots(r, t):
            tap = sc.tap_of(refs[frame], r.tap).double().numpy()
            x, where = _pick(got, r, name, idx, sc.region(r, f, mks[0, frame, 0]))
            assert x.shape == tap.shape, (r.key, x.shape, tap.shape)
            d = np.abs(x - tap)[where]
            finite = bool(np.isfinite(x[where]).all())
            tag = f"STAGE {what} {build} {sched} {r.key} [{name} frame {frame}]"
            if refs32 is None:
                bound = sc.bound_of(tap)
                print(f"{tag} max|HIP-tap64| {d.max():.3e} max|tap64| {np.abs(tap).max():.3e} bound {bound:.1e}")
                ok = finite and float(d.max()) < bound
            else:
                td = np.abs(tap - sc.tap_of(refs32[frame], r.tap).double().numpy())[where]
                fm, fx = BF16_FACTORS.get(r.key, BF16_DEFAULT)
                if td.max() == 0.0:      # a tensor the storage does not touch (flow2 / flow8 of the injected flow): the fp32 bound
                    bound = sc.bound_of(tap)
                    print(f"{tag} max|HIP-twin| {d.max():.3e} max|twin| {np.abs(tap).max():.3e} twin == fp32 oracle: bound {bound:.1e}")
                    ok = finite and float(d.max()) < bound
                else:
                    print(f"{tag} mean|HIP-twin| {d.mean():.3e} max {d.max():.3e} | twin vs fp32 oracle mean {td.mean():.3e} max {td.max():.3e} | "
                          f"ratios {d.mean() / td.mean():.3f} {d.max() / td.max():.3f} (factors {fm} {fx})")
                    ok = finite and float(d.mean()) <= fm * float(td.mean()) and float(d.max()) <= fx * float(td.max())
            if not ok:
                bad.append((r.key, name, frame))
    assert not bad, bad


def _census(got, build, sched, t, mks, what):
    """(c): which buffers hold anything after a run on a 0xFF workspace, and no NaN where a tensor was written."""
    f = sc.flags(build, sched)
    holds = sorted(n for n in sc.fetch_names(t) if not np.isnan(got[n]).all())
    want = sc.written_names(build, sched, t)
    print(f"CENSUS {what} {build} {sched} t={t}: written {' '.join(holds)} | untouched {' '.join(n for n in sc.fetch_names(t) if n not in holds)}")
    assert holds == want, (sorted(set(holds) - set(want)), sorted(set(want) - set(holds)))
    for r in sc.rows_for(build, sched):
        for name, idx, frame in sc.slots(r, t):
            x, where = _pick(got, r, name, idx, sc.region(r, f, mks[0, frame, 0]))
            assert not np.isnan(x[where]).any(), (r.key, name)
    assert np.isfinite(got["out"]).all()


# ----------------------------------------------------------------------------- (a), (c), (e): the product schedule, in this process
@pytest.mark.parametrize("regime,t,h,w", RUNS)
def test_f32_stages_vs_float64(regime, t, h, w):
    got, mks = _run(regime, t, h, w), _case(regime, t, h, w)[3]
    what = f"{regime}/t{t}"
    _assert_regime(got, regime, h, w, what)
    refs = _ref(regime, t, h, w, "f64")
    d = float(np.abs(got["out"].astype(np.float64) - torch.stack([p["out"] for p in refs], 1).numpy()).max())
    print(f"STAGE {what} f32 product out max|HIP-oracle64| {d:.3e}")
    assert d < 1e-4
    _compare(got, "f32", "product", t, refs, mks, sc.rows_for("f32", "product"), what)
    _census(got, "f32", "product", t, mks, what)


def test_f32_stages_vs_float64_y_only():
    regime, t, h, w = CHILD
    got, mks = _run(regime, t, h, w, "f32", True), _case(regime, t, h, w, True)[3]
    _assert_regime(got, regime, h, w, "large/t3 y_only")
    refs = _ref(regime, t, h, w, "f64", "f32", True)
    assert got["out"].shape[2] == 1
    assert float(np.abs(got["out"].astype(np.float64) - torch.stack([p["out"] for p in refs], 1).numpy()).max()) < 1e-4
    _compare(got, "f32", "product", t, refs, mks, sc.rows_for("f32", "product"), "large/t3/y_only")
    _census(got, "f32", "product", t, mks, "large/t3/y_only")


@pytest.mark.parametrize("regime,t,h,w", RUNS)
def test_bf16_stages_vs_twin(regime, t, h, w):
    got, mks = _run(regime, t, h, w, "bf16"), _case(regime, t, h, w)[3]
    what = f"{regime}/t{t}"
    _assert_regime(got, regime, h, w, what + " bf16")
    _compare(got, "bf16", "product", t, _ref(regime, t, h, w, "twin", "bf16"), mks, sc.rows_for("bf16", "product"), what,
             refs32=_ref(regime, t, h, w, "f32", "bf16"))
    _census(got, "bf16", "product", t, mks, what)


# ----------------------------------------------------------------------------- (b): the other schedules, one child process each
@functools.lru_cache(maxsize=None)
def _child(sched, tmp):
    env_add, lab = sc.SCHEDULES[sched]
    env = dict(os.environ, **env_add)
    if lab:
        assert os.path.exists(sc.LAB_LIB), "the lab library is not built (make -C crfp_amd/csrc lab)"
        env["CRFP_HIP_LIB"] = sc.LAB_LIB
    path = os.path.join(tmp, sched + ".npz")
    regime, t, h, w = CHILD
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(sc.__file__)), "dsv_stage_cases.py"), path, "--regime", regime,
                        "--t", str(t), "--h", str(h), "--w", str(w), "--storage", "f32,bf16"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def child_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dsv_stages"))


@pytest.mark.parametrize("build", sc.BUILDS)
@pytest.mark.parametrize("sched", [s for s in sc.SCHEDULES if s != "product"])
def test_other_schedules_stages_and_bits(sched, build, child_dir):
    regime, t, h, w = CHILD
    both = _child(sched, child_dir)
    got = {k.split(":", 1)[1]: v for k, v in both.items() if k.startswith(build + ":")}
    prod, mks = _run(regime, t, h, w, build), _case(regime, t, h, w)[3]
    assert not bool(got["overflowed"])
    what = "large/t3"
    _census(got, build, sched, t, mks, what)
    # the buffers this schedule writes and the product does not (mask_gate0: the gated ones, now over the whole frame)
    fp, fc = sc.flags(build, "product"), sc.flags(build, sched)
    mine = [r for r in sc.rows_for(build, sched) if r not in sc.rows_for(build, "product") or (r.gated and not fc.gate)]
    assert mine or (build, sched) == ("bf16", "lab_unfused"), (sched, build)      # (the lab library's bf16 objects are the product's)
    if build == "f32":
        _compare(got, build, sched, t, _ref(regime, t, h, w, "f64"), mks, mine, what)
    else:
        _compare(got, build, sched, t, _ref(regime, t, h, w, "twin", "bf16"), mks, mine, what, refs32=_ref(regime, t, h, w, "f32", "bf16"))
    # what both runs write is the same bits (gated buffers: where the gated run has to hold them)
    assert np.array_equal(got["out"].view(np.uint32), prod["out"].view(np.uint32)), "output"
    shared = [r for r in sc.rows_for(build, sched, compared_only=False) if r in sc.rows_for(build, "product", compared_only=False)]
    n = 0
    for r in shared:
        for name, idx, frame in sc.slots(r, t):
            a, where = _pick(got, r._replace(sel=None), name, idx, sc.region(r, fp, mks[0, frame, 0]))
            b, _ = _pick(prod, r._replace(sel=None), name, idx, None)
            assert np.array_equal(np.where(where, a, 0.0).astype(np.float32).view(np.uint32), np.where(where, b, 0.0).astype(np.float32).view(np.uint32)), \
                (sched, build, name)
            n += 1
    print(f"BITS large/t3 {build} {sched}: {n} buffers bit-equal to the product run; compared on their own: {' '.join(r.key for r in mine)}")


# ----------------------------------------------------------------------------- (d): a dirty workspace gives a fresh one's bits
def _gpu(*arrays):
    return tuple(T(a).to("cuda:0") for a in arrays)


@pytest.mark.parametrize("single_stream", [False, True])
@pytest.mark.parametrize("storage", sc.BUILDS)
def test_dirty_workspace_clip(storage, single_stream):
    regime, t, h, w = CHILD
    sd, lrs, fvs, mks = _case(regime, t, h, w)
    names = ["state_hr", "carry", "poff", "feat", "x_lr", "flow_lr"]
    res = []
    for dirty in (False, True):
        m = sc.make_model(sd, storage)
        eng = m.engine()
        eng.single_stream = single_stream
        if dirty:
            sc.dirty_workspace(eng, t, h, w)
        out = m(*_gpu(lrs, fvs, mks))
        assert not eng.overflowed()
        res.append([out.cpu()] + [eng.debug_fetch(n, t, h, w).cpu() for n in names])
    assert torch.isfinite(res[0][0]).all()
    for n, a, b in zip(["out"] + names, *res):
        assert torch.equal(a, b), f"{n}: a 0xFF workspace changes the bits ({storage}, single_stream={single_stream})"
    if storage == "f32" and not single_stream:       # and they are the bits of the run every other test here reads
        assert np.array_equal(res[0][0].numpy(), _run(regime, t, h, w)["out"])


@pytest.mark.parametrize("storage", sc.BUILDS)
def test_dirty_workspace_lockstep(storage):
    """n = 2 (the large and the moderate clip of one geometry in one lock-step call) on a 0xFF workspace == on a fresh one == two one-clip calls."""
    t, h, w = 3, 33, 47
    sd, big = _case("large", t, h, w)[0], _case("large", t, h, w)[1:]
    small = _case("moderate", t, h, w)[1:]
    two = _gpu(*(np.concatenate([a, b], 0) for a, b in zip(big, small)))
    res = []
    for dirty in (False, True):
        m = sc.make_model(sd, storage)
        if dirty:
            sc.dirty_workspace(m.engine(), t, h, w, 2)
        res.append(m(*two).cpu())
        assert not m.engine().overflowed()
    assert torch.isfinite(res[0]).all() and torch.equal(res[0], res[1]), "lock-step: a 0xFF workspace changes the bits"
    one = sc.make_model(sd, storage)
    assert torch.equal(res[1][:1], one(*_gpu(*big)).cpu()) and torch.equal(res[1][1:], one(*_gpu(*small)).cpu())


@pytest.mark.parametrize("storage", sc.BUILDS)
def test_dirty_workspace_stream(storage):
    """MRCF_simple_v18, three one-frame calls: the streaming workspace filled with 0xFF before the first call gives a fresh one's bits, which
    are the clip engine's."""
    regime, t, h, w = CHILD
    sd, lrs, fvs, mks = _case(regime, t, h, w)
    L, Fv, M = _gpu(lrs, fvs, mks)
    res = []
    for dirty in (False, True):
        m = sc.make_model(sd, storage, cls="MRCF_simple_v18")
        m.clear_states()
        if dirty:
            eng = m.engine()
            nb = eng._call("batch_workspace_bytes")(1, 1, h, w)
            eng._stream_ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda:0")
            eng._stream_hw, eng._stream_prev = (1, h, w), None
        res.append(torch.cat([m(L[:, i:i + 1].contiguous(), Fv[:, i:i + 1].contiguous(), M[:, i:i + 1].contiguous()).clone() for i in range(t)], 1).cpu())
        assert not m.engine().overflowed(stream=True)
    assert torch.isfinite(res[0]).all() and torch.equal(res[0], res[1]), "streaming: a 0xFF workspace changes the bits"
    assert np.array_equal(res[1].numpy(), _run(regime, t, h, w, storage)["out"])
