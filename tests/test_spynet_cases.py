"""CPU: the SPyNet cases of tests/helpers/spynet_cases.py against the reference alone -- the float64-capable restatement is the oracle's, every
weight set does what its name says, every push meets its regime, every case is well conditioned under the bound the GPU tests assert, and the
cases together reach every branch of the host's split / direct rule (tests/test_gpu_spynet.py holds that rule to the library's own launches)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import spynet_cases as sp

IDS = [c.id for c in sp.CASES]


def test_reference_f32_is_the_oracle_bit_for_bit():
    from crfp_amd import synth
    from oracle import crfp_oracle as orc
    g = dict(np.load(os.path.join(GOLDEN, "spynet_small.npz")))
    assert int(g["weights_seed"]) == sp.WEIGHT_SEED
    sd = synth.make_spynet_state_dict(sp.WEIGHT_SEED)
    P = orc.load_numpy_state(sd)
    for tag in "ab":
        ref, supp = torch.from_numpy(g[tag + "_ref"]), torch.from_numpy(g[tag + "_supp"])
        with torch.no_grad():
            want = orc.spynet(P, ref, supp)
        got, taps = sp.reference(sd, ref, supp, torch.float32)
        assert got.dtype == torch.float32 and torch.equal(got, want), tag
        assert float((got - torch.from_numpy(g[tag + "_flow"])).abs().max()) < 1e-6, tag
        assert len(taps) == sp.LEVELS and all(set(t) == {"flow_up", "warped", "flow"} for t in taps)
        f64, _ = sp.reference(sd, ref, supp, torch.float64)
        assert f64.dtype == torch.float64 and float((f64 - want.double()).abs().max()) < 0.25 * sp.bound_of(f64)


def test_cases_cover_the_issue_shapes():
    shapes = {(c.h, c.w, c.n) for c in sp.CASES}
    assert {(24, 40, 2), (32, 32, 2), (33, 47, 1), (64, 96, 2), (180, 320, 1), (128, 256, 2)} <= shapes
    assert len(set(IDS)) == len(IDS)
    for h, w, n in sp.SMALL_SHAPES:
        for kind in sp.KINDS:
            assert {c.wset for c in sp.CASES if (c.h, c.w, c.n, c.kind) == (h, w, n, kind)} == set(sp.ALL_SETS)
    for h, w, n, kind in sp.LARGE_SHAPES:
        assert {c.wset for c in sp.CASES if (c.h, c.w, c.n) == (h, w, n)} == set(sp.LARGE_SETS)
    # two different pairs in a batch, and the two frame kinds differ
    for kind in sp.KINDS:
        ref, supp = sp.frames(kind, 2, 64, 96)
        assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(supp[0], supp[1]) and not np.array_equal(ref, supp)
        assert ref.dtype == np.float32 and 0.0 <= ref.min() and ref.max() <= 1.0


@pytest.mark.parametrize("case", sp.CASES, ids=IDS)
def test_weight_set_regime_and_conditioning(case):
    flow64, taps = sp.case_reference(case)
    flow32, _ = sp.case_reference(case, False)
    share = sp.clamped_share(taps)
    bound = sp.bound_of(flow64)
    d = float((flow32.double() - flow64).abs().max())
    print(f"CASE {case.id}: max|flow64| {float(flow64.abs().max()):.3f} max|flow32-flow64| {d:.3e} = {d / bound:.4f} of the bound, "
          f"clamped share {share:.4f}")
    assert torch.isfinite(flow64).all() and tuple(flow64.shape) == (case.n, 2, case.h, case.w)
    if case.wset.startswith("only"):
        L = int(case.wset[4:])
        for level in range(sp.LEVELS):
            if level <= L:
                assert float(taps[level]["flow_up"].abs().max()) == 0.0, level
            if level > L:      # later levels add exactly nothing
                assert torch.equal(taps[level]["flow"], taps[level]["flow_up"]), level
        assert float(taps[L]["flow"].abs().max()) > 0.05      # and level L's chain is no stub
    if case.wset.startswith("push:"):
        regime = case.wset.split(":")[1]
        L, bx, by = sp.PUSHES[(sp.up32(case.h), sp.up32(case.w))][regime]
        f = taps[L]["flow"]
        assert bool((f[:, 0] == float(np.float32(bx))).all()) and bool((f[:, 1] == float(np.float32(by))).all())
        if regime == "inside":
            assert share == 0.0
        elif regime == "partial":
            assert 0.1 < share < 0.9
        else:
            assert share >= 0.99
        assert sp.regime_of(share) == regime
    # conditioning: the fp32 reference sits well inside the bound the GPU tests hold the kernels to
    assert d <= 0.25 * bound, (d, bound)


def test_branch_coverage():
    seen = set()
    for h, w, n in {(c.h, c.w, c.n) for c in sp.CASES}:
        for r in sp.conv_table(n, h, w):
            seen.add((r.cout, r.branch))
            seen.add(("n", n, r.branch))
            if r.H == 1:
                seen.add(("1-high", r.branch))
            if r.H == 1 and r.W == 1:
                seen.add(("1x1", r.branch))
            assert r.ct2 == (r.cout == 64)
    for cout in (32, 64, 16, 2):
        assert (cout, "split") in seen and (cout, "direct") in seen, cout
    assert ("n", 1, "direct") in seen and ("n", 2, "direct") in seen
    assert ("1-high", "split") in seen and ("1x1", "split") in seen
    for h, w in sp.BATCH_SHAPES:
        assert sp.conv_branches(1, h, w) == sp.conv_branches(2, h, w), (h, w)
        assert any(c.n == 2 and (c.h, c.w) == (h, w) for c in sp.CASES)


def test_branch_rule_on_known_shapes():
    """The figures of the rule that can be worked out by hand."""
    b = sp.conv_branches(1, 64, 96)       # finest level: cout 32 / 64 / 32 direct, 16 / 2 split; every coarser level split
    assert [b[(5, j)] for j in range(5)] == ["direct", "direct", "direct", "split", "split"]
    assert all(b[(lv, j)] == "split" for lv in range(5) for j in range(5))
    b = sp.conv_branches(1, 180, 320)     # 192 x 320: ceil(320 / 64) * (192 / 4) = 240 >= 228 -> cout 16 / 2 direct
    assert [b[(5, j)] for j in range(5)] == ["direct"] * 5
    assert sp.launch_counts(1, 180, 320) == (5, 25) and sp.launch_counts(1, 64, 96) == (3, 27)
    assert sp.launch_counts(2, 128, 256) == (5, 25) and sp.launch_counts(1, 128, 256) == (3, 27)
    assert sp.up32(33) == 64 and sp.up32(32) == 32 and sp.up32(180) == 192
