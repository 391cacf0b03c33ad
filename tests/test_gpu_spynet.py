"""GPU (-m gpu): ``crfp_spynet_forward`` (csrc/spynet.hip) and the per-operator SPyNet route against float64, by pyramid level, by conv branch
and under large motion.

The call exposes no intermediate buffer, so the levels are separated through the weights (tests/helpers/spynet_cases.py: `only<L>` leaves one
level's conv chain, `push:<regime>` injects a uniform motion at one level; tests/test_spynet_cases.py checks the cases against the reference
alone).  The bound is the project's stage bound, 1e-4 * max(1, max |flow64|), on every case.

(a) every case of ``CASES`` through ``SPyNet.forward`` against the float64 reference.
(b) the launch counts of the library's own event profiler under `spynet_conv7_mfma` / `spynet_conv7_mfma_ksplit` equal the direct / split
    counts of ``conv_branches``, for every shape of the cases.
(c) one n = 2 call equals two n = 1 calls bit for bit, at the shapes whose branch table does not depend on n.
(d) the C ABI called directly on a workspace of exactly ``crfp_spynet_workspace_bytes`` followed by a 64 KiB canary: 0xFF bytes in the workspace
    give the bits of zeroes, the canary survives; one byte short / a null parameter pointer return CRFP_E_WORKSPACE / CRFP_E_BADARG.
(e) the call on a fresh stream gives the default stream's bits.
(f) ``SPyNet.compute_flow`` (ops.avgpool2, upsample_bilinear_ac, flow_warp(border), convkxk) against the float64 level-5 flow under large motion.
(g) ``ops.convkxk`` (K = 3, 5, 7) against F.conv2d in float64;  (h) ``ops.upsample_bilinear_ac`` on 1-pixel inputs.

Measured on an MI355X.  No case came near its bound: the worst share is 0.077 (180x320 `only5`: 7.7e-6 of 1.0e-4, where the CPU fp32 reference
itself is at 0.078), the HIP call sits as far from float64 as the CPU fp32 reference does on every row, and no defect was found.  Launch counts
reported by the library's profiler, direct + split of 30: 3 + 27 at 24x40 n=2, 32x32 n=2, 33x47 n=1 and 64x96 n=2; 5 + 25 at 180x320 n=1 and
128x256 n=2 -- the table of ``conv_branches`` at every shape.  n = 2 calls, 0xFF workspaces and the side stream were bit-equal to their baselines
and the canary was intact.

(a) per case: max |HIP - flow64| / max |CPU fp32 - flow64| (max |flow64|) clamped share; bound 1e-4 * max(1, max |flow64|):

    shape, weight set          smooth frames                          noise frames
    24x40n2 plain              6.70e-07 / 6.83e-07 (0.711) 0.030      1.43e-06 / 1.55e-06 (1.26) 0.032
    24x40n2 only0              3.75e-07 / 4.60e-07 (1.54) 0.106       3.86e-07 / 4.11e-07 (1.54) 0.106
    24x40n2 only1              2.67e-07 / 2.24e-07 (0.88) 0.062       2.63e-07 / 2.29e-07 (0.875) 0.062
    24x40n2 only2              1.09e-07 / 1.14e-07 (0.309) 0.018      1.41e-07 / 1.67e-07 (0.322) 0.020
    24x40n2 only3              2.32e-07 / 2.93e-07 (0.383) 0.040      2.80e-07 / 3.55e-07 (0.467) 0.038
    24x40n2 only4              3.94e-07 / 3.77e-07 (0.686) 0.046      7.39e-07 / 7.20e-07 (0.955) 0.044
    24x40n2 only5              6.48e-07 / 5.68e-07 (0.424) 0.000      1.08e-06 / 1.03e-06 (0.694) 0.000
    24x40n2 push:inside        6.48e-07 / 5.68e-07 (0.424) 0.000      1.08e-06 / 1.03e-06 (0.694) 0.000
    24x40n2 push:partial       4.43e-06 / 3.95e-06 (10.8) 0.429       4.55e-06 / 3.99e-06 (10.8) 0.426
    24x40n2 push:off_frame     3.57e-05 / 3.86e-05 (82) 1.000         3.45e-05 / 3.95e-05 (81.9) 1.000
    32x32n2 plain              1.39e-06 / 1.21e-06 (0.913) 0.080      2.10e-06 / 2.25e-06 (1.33) 0.064
    32x32n2 only0              1.57e-07 / 5.90e-07 (2.33) 0.150       1.61e-07 / 5.81e-07 (2.33) 0.150
    32x32n2 only1              3.37e-07 / 2.84e-07 (1.38) 0.092       3.52e-07 / 2.98e-07 (1.38) 0.092
    32x32n2 only2              1.02e-07 / 8.56e-08 (0.418) 0.031      1.10e-07 / 1.11e-07 (0.445) 0.031
    32x32n2 only3              1.73e-07 / 2.00e-07 (0.709) 0.053      2.75e-07 / 3.10e-07 (0.715) 0.048
    32x32n2 only4              4.46e-07 / 7.45e-07 (1.03) 0.059       6.50e-07 / 1.02e-06 (1.38) 0.058
    32x32n2 only5              1.30e-06 / 9.43e-07 (0.8) 0.000        2.34e-06 / 1.68e-06 (1.37) 0.000
    32x32n2 push:inside        1.30e-06 / 9.43e-07 (0.8) 0.000        2.34e-06 / 1.68e-06 (1.37) 0.000
    32x32n2 push:partial       7.44e-06 / 7.31e-06 (14.7) 0.525       7.75e-06 / 7.34e-06 (14.9) 0.523
    32x32n2 push:off_frame     4.98e-05 / 5.57e-05 (118) 1.000        5.38e-05 / 8.82e-05 (118) 1.000
    33x47n1 plain              1.33e-06 / 1.09e-06 (0.896) 0.038      1.92e-06 / 2.06e-06 (1.37) 0.056
    33x47n1 only0              5.68e-07 / 4.88e-07 (1.87) 0.077       5.56e-07 / 4.16e-07 (1.87) 0.077
    33x47n1 only1              3.16e-07 / 3.37e-07 (1.13) 0.046       2.84e-07 / 3.83e-07 (1.11) 0.046
    33x47n1 only2              3.29e-07 / 3.39e-07 (0.688) 0.030      3.85e-07 / 4.60e-07 (0.73) 0.032
    33x47n1 only3              3.39e-07 / 4.22e-07 (0.421) 0.031      5.48e-07 / 7.66e-07 (0.572) 0.027
    33x47n1 only4              5.05e-07 / 6.45e-07 (0.736) 0.031      1.11e-06 / 1.25e-06 (1.29) 0.035
    33x47n1 only5              8.95e-07 / 9.39e-07 (0.291) 0.000      2.33e-06 / 1.63e-06 (0.54) 0.000
    33x47n1 push:inside        8.95e-07 / 9.39e-07 (0.291) 0.000      2.33e-06 / 1.63e-06 (0.54) 0.000
    33x47n1 push:partial       4.79e-06 / 4.63e-06 (9.42) 0.295       5.23e-06 / 4.96e-06 (9.61) 0.292
    33x47n1 push:off_frame     4.75e-05 / 5.39e-05 (94.3) 1.000       4.44e-05 / 5.30e-05 (94.4) 1.000
    64x96n2 plain              2.89e-06 / 3.37e-06 (1.46) 0.034       4.88e-06 / 5.00e-06 (1.94) 0.038
    64x96n2 only0              8.26e-07 / 6.90e-07 (2.56) 0.062       7.51e-07 / 7.49e-07 (2.57) 0.062
    64x96n2 only1              5.17e-07 / 3.80e-07 (1.56) 0.036       5.13e-07 / 4.93e-07 (1.61) 0.036
    64x96n2 only2              7.06e-07 / 7.54e-07 (1.06) 0.021       7.54e-07 / 1.05e-06 (1.14) 0.026
    64x96n2 only3              5.26e-07 / 4.93e-07 (0.585) 0.026      9.12e-07 / 9.97e-07 (0.826) 0.022
    64x96n2 only4              1.53e-06 / 1.44e-06 (1.23) 0.026       2.56e-06 / 2.44e-06 (1.74) 0.026
    64x96n2 only5              1.83e-06 / 1.60e-06 (0.82) 0.000       3.60e-06 / 3.51e-06 (1.73) 0.000
    64x96n2 push:inside        1.83e-06 / 1.60e-06 (0.82) 0.000       3.60e-06 / 3.51e-06 (1.73) 0.000
    64x96n2 push:partial       8.92e-06 / 9.92e-06 (15) 0.253         9.84e-06 / 1.10e-05 (15.7) 0.250
    64x96n2 push:off_frame     6.43e-05 / 8.28e-05 (130) 1.000        6.44e-05 / 9.10e-05 (130) 1.000
    180x320n1 plain            1.02e-05 / 1.04e-05 (4.87) 0.012       -
    180x320n1 only5            7.69e-06 / 7.78e-06 (0.639) 0.000      -
    180x320n1 push:partial     1.15e-04 / 1.13e-04 (85.2) 0.404       -
    128x256n2 plain            -                                      1.08e-05 / 1.15e-05 (4.05) 0.017
    128x256n2 only5            -                                      7.32e-06 / 6.86e-06 (1.56) 0.000
    128x256n2 push:partial     -                                      7.16e-05 / 7.56e-05 (82.8) 0.514
(`push:inside` is `only5` by construction -- see the helper -- so the two rows agree.)

(f) ``compute_flow`` against the float64 level-5 flow, max |HIP - flow64| over both frame kinds (same bound): 64x96 plain 5.3e-06, push:partial
1.4e-05, push:off_frame 9.9e-05; 32x32 plain 3.0e-06, push:partial 1.0e-05, push:off_frame 8.1e-05.
(g) ``convkxk``: worst max |HIP - ref64| 7.3e-06 at max |ref64| 6.2 (K = 7, 16 -> 16, 17x33).  (h) ``upsample_bilinear_ac``: <= 5.6e-07, 1x1 exact.

The tests bite.  Four arithmetic-only one-line changes to spynet.hip, each built apart and run once against this file; every one fails
``test_forward_vs_float64`` and nothing else (the bit comparisons hold a changed library to itself):
    u and v swapped in spy_w9_kernel (transposed 7x7 taps)      84 of 86 cases fail (32x32 `only0` passes: on a 1x1 map only the centre tap is read)
    1.0 instead of 2.0 in the flow upsampling                   68: every case but `only5` / `push:inside`, whose upsampled flow is zero
    8 of the 9 partial sums in spy_sum9_kernel                  72: every case with a split conv on a map the (+3, +3) view reaches; what passes is `only0`
                                                                everywhere and `only1` at 24x40 / 32x32 (maps at most 2 pixels high: that view is all
                                                                padding) and `only5` at the two large shapes (finest level all direct)
    mulx and muly swapped in the final rescale                  43: all cases of 24x40, 33x47 and 180x320, the shapes with h / h_up != w / w_up
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import spynet_cases as sp

pytestmark = pytest.mark.gpu

T = torch.from_numpy
IDS = [c.id for c in sp.CASES]
SHAPES = sorted({(c.h, c.w, c.n) for c in sp.CASES})
CRFP_E_BADARG, CRFP_E_WORKSPACE = -1, -2      # include/crfp_hip.h
CANARY = 64 * 1024


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def _model(wset, hu, wu):
    """SPyNet with a weight set of the cases (the pushes depend on the padded shape)."""
    from crfp_amd.model import CRFP
    m = CRFP.SPyNet(None, dev())
    m.load_state_dict({k: T(v.copy()) for k, v in sp.weight_set(wset, hu, wu).items()}, strict=True)
    return m.to(dev()).eval()


def _model_for(wset, h, w):
    return _model(wset, sp.up32(h), sp.up32(w))


def _frames(kind, n, h, w):
    ref, supp = sp.frames(kind, n, h, w)
    return T(ref.copy()).to(dev()), T(supp.copy()).to(dev())


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------- (a) every case against float64
@pytest.mark.parametrize("case", sp.CASES, ids=IDS)
def test_forward_vs_float64(case):
    flow64, taps = sp.case_reference(case)
    flow32, _ = sp.case_reference(case, False)
    got = _model_for(case.wset, case.h, case.w)(*_frames(case.kind, case.n, case.h, case.w)).cpu()
    bound = sp.bound_of(flow64)
    d = float((got.double() - flow64).abs().max())
    d32 = float((flow32.double() - flow64).abs().max())
    direct, split = sp.launch_counts(case.n, case.h, case.w)
    print(f"CASE {case.id:34s} max|HIP-flow64| {d:.3e} max|cpu32-flow64| {d32:.3e} max|flow64| {float(flow64.abs().max()):.4g} bound {bound:.1e} "
          f"clamped {sp.clamped_share(taps):.3f} launches {direct}+{split}")
    assert tuple(got.shape) == (case.n, 2, case.h, case.w) and bool(torch.isfinite(got).all())
    assert d < bound, (case.id, d, bound)


# ----------------------------------------------------------------------------- (b) the branch table is the library's
@pytest.mark.parametrize("h,w,n", SHAPES, ids=[f"{h}x{w}n{n}" for h, w, n in SHAPES])
def test_launch_counts_match_branch_table(h, w, n):
    from crfp_amd import _lib
    m = _model_for("plain", h, w)
    ref, supp = _frames("noise", n, h, w)
    m(ref, supp)                        # nothing of the first call of a process is counted
    torch.cuda.synchronize()
    L = _lib.lib()
    L.crfp_prof_reset()
    L.crfp_prof_enable(1)
    try:
        m(ref, supp)
        torch.cuda.synchronize()
        recs = {r["name"]: r["launches"] for r in _lib.prof_report(512)}
    finally:
        L.crfp_prof_enable(0)
        L.crfp_prof_reset()
    got = (recs.get("spynet_conv7_mfma", 0), recs.get("spynet_conv7_mfma_ksplit", 0))
    print(f"LAUNCHES {h}x{w} n={n}: direct {got[0]} split {got[1]}; table {sp.launch_counts(n, h, w)}")
    assert got == sp.launch_counts(n, h, w)
    assert sum(got) == 30


# ----------------------------------------------------------------------------- (c) batch
@pytest.mark.parametrize("wset", ["plain", "push:partial"])
@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("h,w", sp.BATCH_SHAPES, ids=[f"{h}x{w}" for h, w in sp.BATCH_SHAPES])
def test_batch_of_two_is_two_calls(h, w, kind, wset):
    assert sp.conv_branches(1, h, w) == sp.conv_branches(2, h, w)
    m = _model_for(wset, h, w)
    ref, supp = _frames(kind, 2, h, w)
    assert not torch.equal(ref[0], ref[1])
    both = m(ref, supp)
    for i in range(2):
        one = m(ref[i:i + 1].contiguous(), supp[i:i + 1].contiguous())
        assert _bits(both[i:i + 1], one), f"pair {i} of the n = 2 call differs from its n = 1 call"


# ----------------------------------------------------------------------------- (d) workspace contract, through the C ABI
def _raw_call(m, ref, supp, fill, short=0, null_param=None):
    """crfp_spynet_forward called directly: a workspace of exactly the queried size filled with `fill` bytes, followed by a canary.
    -> (return code, flow, canary intact)."""
    from crfp_amd import _lib
    L = _lib.lib()
    n, _, h, w = ref.shape
    keep = [p.detach().contiguous() for p in m._params()]
    assert len(keep) == 60 and all(p.is_cuda and p.dtype == torch.float32 for p in keep)
    ptrs = (C.c_void_p * 60)(*[p.data_ptr() for p in keep])
    if null_param is not None:
        ptrs[null_param] = None
    need = int(L.crfp_spynet_workspace_bytes(n, h, w))
    assert need > 0
    buf = torch.empty(need + CANARY, dtype=torch.uint8, device=ref.device)
    buf[:need].fill_(fill)
    buf[need:].fill_(0xA5)
    flow = torch.full((n, 2, h, w), 7.0, dtype=torch.float32, device=ref.device)
    with torch.cuda.device(ref.device):
        rc = L.crfp_spynet_forward(ptrs, ref.data_ptr(), supp.data_ptr(), flow.data_ptr(), n, h, w, buf.data_ptr(), need - short,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, flow, bool((buf[need:] == 0xA5).all())


@pytest.mark.parametrize("wset", ["plain", "push:partial"])
@pytest.mark.parametrize("h,w,n", [(24, 40, 2), (64, 96, 1)], ids=["24x40n2", "64x96n1"])
def test_dirty_workspace_and_canary(h, w, n, wset):
    m = _model_for(wset, h, w)
    ref, supp = _frames("smooth", n, h, w)
    rc0, clean, ok0 = _raw_call(m, ref, supp, 0x00)
    rc1, dirty, ok1 = _raw_call(m, ref, supp, 0xFF)
    assert rc0 == 0 and rc1 == 0
    assert bool(torch.isfinite(clean).all()) and _bits(clean, dirty), "a 0xFF workspace changes the bits"
    assert ok0 and ok1, "the call wrote past crfp_spynet_workspace_bytes"
    assert _bits(clean, m(ref, supp)), "the C ABI and ops.spynet_forward disagree"


def test_argument_errors_return_before_any_launch():
    from crfp_amd import _lib
    h, w, n = 24, 40, 2
    m = _model_for("plain", h, w)
    ref, supp = _frames("smooth", n, h, w)
    rc, flow, ok = _raw_call(m, ref, supp, 0xFF, short=1)
    assert rc == CRFP_E_WORKSPACE and ok and bool((flow == 7.0).all())
    assert b"workspace" in _lib.lib().crfp_last_error_string()
    rc, flow, ok = _raw_call(m, ref, supp, 0xFF, null_param=37)
    assert rc == CRFP_E_BADARG and ok and bool((flow == 7.0).all())
    assert b"parameter 37" in _lib.lib().crfp_last_error_string()
    assert _lib.lib().crfp_spynet_workspace_bytes(0, h, w) == 0


# ----------------------------------------------------------------------------- (e) stream
@pytest.mark.parametrize("h,w,n", [(24, 40, 2), (64, 96, 2)], ids=["24x40n2", "64x96n2"])
def test_other_stream_gives_the_same_bits(h, w, n):
    m = _model_for("push:partial", h, w)
    ref, supp = _frames("noise", n, h, w)
    base = m(ref, supp)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = m(ref, supp)
    s.synchronize()
    assert bool(torch.isfinite(base).all()) and _bits(base, other)


# ----------------------------------------------------------------------------- (f) the per-operator route under large motion
@pytest.mark.parametrize("wset", ["plain", "push:partial", "push:off_frame"])
@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("h,w", [(64, 96), (32, 32)], ids=["64x96", "32x32"])
def test_compute_flow_vs_float64(h, w, kind, wset):
    case = sp.Case(h, w, 2, kind, wset)
    assert case in sp.CASES
    _, taps = sp.case_reference(case)
    want = taps[sp.LEVELS - 1]["flow"]           # no resize at these shapes: the level-5 flow is the network's
    got = _model_for(wset, h, w).compute_flow(*_frames(kind, 2, h, w)).cpu()
    bound = sp.bound_of(want)
    d = float((got.double() - want).abs().max())
    print(f"COMPUTE_FLOW {case.id}: max|HIP-flow64| {d:.3e} max|flow64| {float(want.abs().max()):.4g} bound {bound:.1e} "
          f"clamped {sp.clamped_share(taps):.3f}")
    assert bool(torch.isfinite(got).all()) and d < bound


# ----------------------------------------------------------------------------- (g) convkxk
@pytest.mark.parametrize("size", [(1, 1), (5, 37), (17, 33)], ids=["1x1", "5x37", "17x33"])
@pytest.mark.parametrize("cin,cout", [(3, 2), (6, 20), (8, 32), (16, 16)])
@pytest.mark.parametrize("K", [3, 5, 7])
def test_convkxk_vs_float64(K, cin, cout, size):
    from crfp_amd import ops
    h, w = size
    rs = np.random.RandomState(1000 * K + 10 * cin + cout + h)
    x = T(rs.standard_normal((2, cin, h, w)).astype(np.float32))
    wt = T((rs.standard_normal((cout, cin, K, K)) * np.sqrt(2.0 / (cin * K * K))).astype(np.float32))
    b = T((rs.standard_normal((cout,)) * 0.1).astype(np.float32))
    for pre_relu in (False, True):
        got = ops.convkxk(x.to(dev()), wt.to(dev()), b.to(dev()), pre_relu=pre_relu).cpu()
        xin = F.relu(x.double()) if pre_relu else x.double()
        want = F.conv2d(xin, wt.double(), b.double(), padding=K // 2)
        d, bound = float((got.double() - want).abs().max()), 2e-5 * max(1.0, float(want.abs().max()))
        print(f"CONVKXK K={K} {cin}->{cout} {h}x{w} pre_relu={int(pre_relu)}: max|HIP-ref64| {d:.3e} max|ref64| {float(want.abs().max()):.3g}")
        assert got.shape == want.shape and bool(torch.isfinite(got).all()) and d < bound, (K, cin, cout, size, pre_relu)


# ----------------------------------------------------------------------------- (h) upsample_bilinear_ac on 1-pixel inputs
@pytest.mark.parametrize("size", [(1, 1), (1, 5), (3, 2)], ids=["1x1", "1x5", "3x2"])
def test_upsample_ac_vs_float64(size):
    from crfp_amd import ops
    h, w = size
    x = T(np.random.RandomState(17 + 10 * h + w).standard_normal((2, 3, h, w)).astype(np.float32))
    got = ops.upsample_bilinear_ac(x.to(dev()), 2, mul=2.0).cpu()
    want = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True) * 2.0
    d = float((got.double() - want).abs().max())
    print(f"UPSAMPLE_AC {h}x{w}: max|HIP-ref64| {d:.3e}")
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    assert d < 1e-5 * max(1.0, float(want.abs().max()))
