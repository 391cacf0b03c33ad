"""CPU: the cases, references and bounds of the gather probe tests (tests/helpers/gather_cases.py) pinned without a GPU -- the conditions on
the inputs (computed from the float64 coordinates: conditions, not measurements), the power-of-two arguments of the exact cases, and the cap
on the reference: the fp32 restatement of every ordinary-data case stays within half of the case's bound from float64, so the bound is known
to be safe on the reference alone before a kernel is held to it."""
import numpy as np
import pytest
import torch

import dcn_paper_ref
from conv_cases import rne_bf16
from helpers import gather_cases as gc
from helpers import motion_cases as mc

ROW_ID = lambda r: f"{r[0]}-{r[1][0]}x{r[1][1]}"   # noqa: E731


def test_tables():
    assert {m: len(s) for m, s in gc.SHAPES.items()} == {"warp": 6, "warp_dual": 6, "dcn_g8": 5, "dcn_fused": 6, "dcn3": 5, "dcn3_fused": 5}
    for h, w in gc.EXACT_WARP_SHAPES:   # the warps' normalisation is exact when both divisors are powers of two
        assert (h - 1) & (h - 2) == 0 and (w - 1) & (w - 2) == 0 and (h, w) in gc.SHAPES["warp"]
    assert gc.N == 3 and gc.RANGES == (9.0, 64.0, 2058.0)
    # tiles straddled: below, on and above one tile, and more than one workgroup, per kernel
    for mode, (th, tw) in (("warp", (4, 64)), ("dcn_g8", (4, 32)), ("dcn_fused", (8, 32)), ("dcn3", (12, 64))):
        hs, ws = {s[0] for s in gc.SHAPES[mode]}, {s[1] for s in gc.SHAPES[mode]}
        assert any(h < th for h in hs) and any(h > th for h in hs) and any(w > tw for w in ws) and any(w < tw for w in ws)
        assert (th, tw) in gc.SHAPES[mode] and any(h % th and w % tw and (h > th or w > tw) for h, w in gc.SHAPES[mode])


@pytest.mark.parametrize("which", ("exact", "normal"))
@pytest.mark.parametrize("row", gc.ROWS, ids=ROW_ID)
def test_conditions_on_the_inputs(row, which):
    """1. every shape above 1 x 1 samples inside the map, in (-1, 0), in (size - 1, size) and clamped at both ends, on both axes; 3. no sampled
    tensor holds a non-finite value; the displacement fields hold the +-3e9 vectors and the three ranges."""
    mode, (h, w) = row
    if which == "exact" and row not in gc.EXACT_ROWS:
        return
    for table in (gc.SAT_TABLES.get(mode, (0,)) if which == "exact" else (0,)):
        inp, ref = gc.case(mode, h, w, which, "f32", table)
        for k in ("x", "x2", "aux"):
            assert inp[k] is None or np.isfinite(inp[k]).all()
        assert np.isfinite(ref["out"]).all()
        if (h, w) == (1, 1):
            continue
        py, px = gc.coords(mode, inp, ref)
        assert all(gc.coverage(py, h).values()), (mode, h, w, "y", gc.coverage(py, h))
        assert all(gc.coverage(px, w).values()), (mode, h, w, "x", gc.coverage(px, w))
        d = inp["flow"] if inp["flow"] is not None else (inp["aux"] if mode == "dcn_g8" else inp["aux"][:, :2])
        last = np.abs(d[gc.N - 1])
        assert np.abs(d).max() == np.float32(gc.HUGE) and (last == np.float32(gc.HUGE)).sum() >= 4 and 64.0 < last[last < 1e9].max()   # R = 2058 in the last item
        if which == "exact":
            assert np.array_equal(d * 4.0, np.round(d * 4.0))
            assert gc.exact_ok(mode, ref)


def test_planted_targets_survive():
    """On and 2^-10 beside -1, 0, size - 1 and size: the planted samples of the ordinary-data fields, on the maps planted_flow cannot take too."""
    for mode, (h, w) in (("warp", (3, 5)), ("warp", (9, 130)), ("dcn_g8", (4, 32)), ("dcn_g8", (23, 45)), ("dcn3", (11, 63))):
        inp, ref = gc.case(mode, h, w, "normal", "f32")
        py, px = gc.coords(mode, inp, ref)
        for p, size in ((py, h), (px, w)):
            for t in mc.edge_targets(size):
                assert (p == t).any(), (mode, h, w, size, t)


def test_exact_arguments():
    """The per-case power-of-two statements: coordinates in quarters, sampled values in 2^-7 (8 bits, an fp16 head without a tail), partial
    sums bounded by S <= 2^10; the fine-weight case: samples in quarters, weights in 2^-12."""
    for mode, (h, w) in (("dcn_g8", (23, 45)), ("dcn3", (13, 65)), ("dcn_fused", (9, 33)), ("dcn3_fused", (13, 65))):
        inp, ref = gc.case(mode, h, w, "exact", "f32")
        assert np.array_equal(ref["off"] * 4, np.round(ref["off"] * 4)) and np.array_equal(ref["msk"].astype(np.float32) * 4, np.round(ref["msk"] * 4))
        assert np.array_equal(inp["x"] * 2, np.round(inp["x"] * 2)) and np.array_equal(inp["weight"] * 2, np.round(inp["weight"] * 2))
        assert np.array_equal(inp["bias"] * 4, np.round(inp["bias"] * 4))
        assert gc.exact_ok(mode, ref)
        out = ref["out"].astype(np.float32).astype(np.float64)
        assert np.abs(out - ref["out"]).max() < 1e-30 and np.array_equal(out * 256, np.round(out * 256))   # an fp32 value, in 2^-8
        if mode.endswith("fused"):   # the saturated head: +-10 + flow, masks 0 / 1 (float64 sigmoid(-200) is 1e-87, not 0: nothing in fp32)
            assert np.array_equal(np.abs(ref["pre"]), np.full_like(ref["pre"], 200.0)) and ref["msk"].max() == 1.0
            assert mode == "dcn3_fused" or ref["msk"].min() < 1e-80
    inp, ref = gc.case("dcn_g8", 23, 45, "fine_w", "f32")
    assert set(np.unique(inp["x"])) == {-1.0, 0.0, 1.0} and set(np.unique(inp["mask"])) == {0.0, 1.0} and np.array_equal(inp["aux"] * 2, np.round(inp["aux"] * 2))
    wt = inp["weight"].astype(np.float64)
    assert np.array_equal(wt * 4096, np.round(wt * 4096)) and (wt != wt.astype(np.float16).astype(np.float64)).mean() > 0.25   # the low part is live
    assert gc.exact_ok("dcn_g8", ref) and np.array_equal(ref["out"] * 2 ** 14, np.round(ref["out"] * 2 ** 14))
    assert np.array_equal(ref["out"].astype(np.float32).astype(np.float64), ref["out"])
    # bf16 build: the reference sees bf16 weights
    inp, refb = gc.case("dcn_g8", 23, 45, "fine_w", "bf16")
    assert np.abs(refb["out"] - ref["out"]).max() > 1e-3


def test_sign_tables():
    """Every (group, tap) of dcn_fused has its own pattern of (dy, dx, mask) signs over the three tables, and its mask on in one at least."""
    rows = np.stack([gc.saturated_bias("dcn_fused", t) for t in gc.SAT_TABLES["dcn_fused"]])
    assert set(np.unique(rows)) == {-200.0, 200.0}
    pat = {tuple(np.concatenate([rows[:, 2 * P], rows[:, 2 * P + 1], rows[:, 144 + P]])) for P in range(72)}
    assert len(pat) == 72
    assert (rows[:, 144:].max(0) == 200.0).all()
    r3 = np.stack([gc.saturated_bias("dcn3_fused", t) for t in gc.SAT_TABLES["dcn3_fused"]])
    assert len({tuple(r) for r in r3}) == 5 and {tuple(r[:2]) for r in r3[:4]} == {(a, b) for a in (-200.0, 200.0) for b in (-200.0, 200.0)}


def test_saturating_share_of_the_scaled_head():
    """Head times 8: a tenth and more of the raw sums sit where tanh and sigmoid are flat to 1e-2 (|s| > 3); head times 1: fewer than a tenth."""
    for mode, (h, w) in (("dcn_fused", (17, 65)), ("dcn3_fused", (25, 130))):
        share = {}
        for scale in (1.0, 8.0):
            _, ref = gc.case(mode, h, w, "normal", "f32", 0, scale)
            share[scale] = float((np.abs(ref["pre"]) > 3.0).mean())
        assert share[8.0] >= 0.1 > share[1.0] * 0.5 and share[8.0] > 4 * share[1.0], share
        _, ref = gc.case(mode, h, w, "normal", "f32", 0, 1.0)
        assert 1.2 < ref["pre"].std() < 1.9


@pytest.mark.parametrize("mode", ("dcn3", "dcn3_fused"))
def test_dcn3_branch_shares(mode):
    """2. one case with 0.2 .. 0.8 of the 64-pixel wave rows all-regular (both branches of dcn3_kernel run), one with every row regular."""
    h, w = gc.BRANCH_SHAPE
    for mixed, lo, hi in ((True, 0.2, 0.8), (False, 1.0, 1.0)):
        inp = gc.branch_inputs(mode, h, w, mixed)
        ref = gc.reference(mode, inp, "f32")
        share = gc.regular_share(ref["off"][:, :2], h, w)
        assert lo <= share <= hi, (mode, mixed, share)
        shareb = gc.regular_share(gc.reference(mode, inp, "bf16")["off"][:, :2], h, w)
        assert lo <= shareb <= hi, (mode, mixed, shareb)
    # the planted fields of the ordinary cases leave (almost) no wave row regular
    _, ref = gc.case(mode, h, w, "normal", "f32")
    assert gc.regular_share(ref["off"][:, :2], h, w) < 0.2


def test_regular_share_by_hand():
    off = np.zeros((1, 2, 4, 70))
    assert gc.regular_share(off, 4, 70) == 1.0
    off[0, 0, 1, 3] = -9.0          # y - 1 + q - 9 < -1 for every tap: clamped, integer parts -1, -1, -1
    assert gc.regular_share(off, 4, 70) == 7 / 8
    off[0, 1, 2, 69] = 0.25         # x + q - 0.75: 68, 69, 70 (clamped to the width, still one apart)
    assert gc.regular_share(off, 4, 70) == 7 / 8


def test_references_agree():
    """dcn_ref64_batched == motion_cases.dcn_ref64 == the paper form; warp_ref == warp_ref64 except on one-pixel axes; rne_bf16 where the
    bf16 build stores."""
    inp, ref = gc.case("dcn_g8", 5, 33, "normal", "f32")
    a = gc.dcn_ref64_batched(inp["x"], inp["aux"], inp["mask"], inp["weight"], inp["bias"], 8)
    assert np.abs(a - ref["out"]).max() < 1e-12
    assert np.abs(dcn_paper_ref.dcnv2_paper(inp["x"][:1], inp["aux"][:1], inp["mask"][:1], inp["weight"], inp["bias"], 8) - ref["out"][:1]).max() < 1e-11
    x = np.arange(6, dtype=np.float64).reshape(1, 1, 1, 6)
    fl = np.zeros((1, 1, 6, 2))
    fl[..., 0], fl[..., 1] = 0.5, 7.0
    assert np.array_equal(gc.warp_ref(x, fl)[0, 0, 0], [0.5, 1.5, 2.5, 3.5, 4.5, 2.5]) and mc.warp_ref64(x, fl).max() == 0.0
    _, refb = gc.case("dcn_g8", 5, 33, "normal", "bf16")
    xb = rne_bf16(torch.from_numpy(inp["x"])).numpy()
    wb = rne_bf16(torch.from_numpy(inp["weight"])).numpy()
    assert np.abs(mc.dcn_ref64(xb, inp["aux"], inp["mask"], wb, inp["bias"], 8) - refb["out"]).max() < 1e-12
    assert np.abs(refb["out"] - ref["out"]).max() > 1e-3
    e = gc.expected(refb["out"], "bf16")
    assert torch.equal(e, e.bfloat16().float()) and torch.equal(gc.expected(ref["out"], "f32"), torch.from_numpy(ref["out"]).float())


def test_fused_reference_is_the_composition():
    """The fused reference == dcn_ref64 on head_ref's offsets and masks, the flow added flipped to (y, x)."""
    inp, ref = gc.case("dcn_fused", 9, 33, "normal", "f32")
    off, msk, S, pre = gc.head_ref(inp["aux"], inp["flow"], inp["head_w"], inp["head_b"], 144)
    want = torch.nn.functional.conv2d(torch.from_numpy(inp["aux"]).double(), torch.from_numpy(inp["head_w"]).double(), torch.from_numpy(inp["head_b"]).double(), padding=1)
    assert np.abs(pre - want.numpy()).max() < 1e-12 and (S >= np.abs(pre) - 1e-12).all()
    fl = inp["flow"].astype(np.float64)
    assert np.abs(off[:, 0] - (10 * np.tanh(pre[:, 0]) + fl[..., 1])).max() < 1e-6 * 3e9 * 2 ** -52 * 4 + 1e-12
    assert np.abs(off[:, 1] - (10 * np.tanh(pre[:, 1]) + fl[..., 0])).max() < 1e-5
    assert np.array_equal(ref["off"], off) and np.array_equal(ref["msk"], msk)
    inp3, ref3 = gc.case("dcn3_fused", 13, 65, "normal", "f32")
    assert ref3["off"].shape[1] == 18 and np.array_equal(ref3["off"][:, 0:2], ref3["off"][:, 16:18]) and ref3["S_head"].shape[1] == 3


@pytest.mark.parametrize("storage", ("f32", "bf16"))
@pytest.mark.parametrize("row", gc.ROWS, ids=ROW_ID)
def test_cap_on_the_reference(row, storage):
    """The fp32 CPU restatement (oracle.flow_warp / oracle.dcnv2 behind an fp32 head) of every ordinary-data case is within half of the case's
    bound from float64 -- the bf16 destination's 2^-8 |ref| not counted."""
    mode, (h, w) = row
    for scale in ((1.0, 8.0) if mode.endswith("fused") else (1.0,)):
        inp, ref = gc.case(mode, h, w, "normal", storage, 0, scale)
        b1, b2 = gc.bound(mode, inp, ref, storage)
        r1, r2 = gc.restate32(mode, inp, storage)
        for got, want, b in ((r1, ref["out"], b1), (r2, ref["out2"], b2)):
            if got is None:
                continue
            share = float((np.abs(got - want) / b).max())
            assert share <= 0.5, (mode, h, w, storage, scale, share)


@pytest.mark.parametrize("mode", ("dcn3", "dcn3_fused"))
def test_cap_on_the_branch_cases(mode):
    h, w = gc.BRANCH_SHAPE
    for mixed in (True, False):
        inp = gc.branch_inputs(mode, h, w, mixed)
        for storage in ("f32", "bf16"):
            ref = gc.reference(mode, inp, storage)
            b, _ = gc.bound(mode, inp, ref, storage)
            share = float((np.abs(gc.restate32(mode, inp, storage)[0] - ref["out"]) / b).max())
            assert share <= 0.5, (mode, mixed, storage, share)
