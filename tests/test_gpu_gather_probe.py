"""GPU: the engines' gather kernels of csrc/gather.hip and dcn_fused.inc, one launch at a time, through the C-ABI's test hook crfp_gather_probe
(crfp_amd.ops.gather_probe): flow_warp_p4_kernel, flow_warp_p4_dual_split_kernel and its unsplit fallback, dcn_g8_pipe_kernel on the split-fp16
weight image, dcn_fused_kernel<8> in its one-tile and persistent forms, dcn3_kernel<false> and <true> -- in the fp32 and the bf16 build.

Every test asserts the kernel the report names.  On the exact inputs of tests/helpers/gather_cases.py the result is the float64 reference bit for
bit (bf16 build: through the destination's rounding); on ordinary data the error is held to the derived bounds of that module.  Every
destination is prefilled with 0xFF bytes: an element no lane wrote comes back NaN, and the slack between batch items must keep every byte."""
import numpy as np
import pytest
import torch

from helpers import gather_cases as gc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STORAGES = ("f32", "bf16")
ROW_ID = lambda r: f"{r[0]}-{r[1][0]}x{r[1][1]}"   # noqa: E731


def launch(mode, inp, storage, raw=False, c=None):
    from crfp_amd import ops
    dev = {k: (None if v is None else gc.T(v).to(DEV)) for k, v in inp.items()}
    x = dev.pop("x")
    return ops.gather_probe(mode, x if c is None else x[:, :c].contiguous(), storage=storage, raw=raw, **dev)


def assert_same_bits(got, want, what):
    got, want = got.cpu(), want.float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements unwritten or not finite"
    if not torch.equal(got, want):
        bad = got != want
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, max |d| = {float((got - want).abs().max()):.3e}, "
                             f"first at {idx}: got {got[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}")


def check_untouched(r, storage):
    """No 0xFF element inside the maps (an unwritten element is NaN in either storage type); the slack behind every item keeps every byte."""
    eb = 2 if storage == "bf16" else 4
    for out, raw in ((r["out"], r["raw"]), (r["out2"], r["raw2"])):
        if out is None:
            continue
        assert bool(torch.isfinite(out).all()), "an element inside the map kept its prefill"
        item = out[0].numel() * eb
        assert raw.shape[1] > item + 256
        assert bool((raw[:, item:] == 0xFF).all()), "bytes between the batch items or behind the last one touched"
        assert not bool((raw[:, :item].reshape(out.shape[0], -1, eb) == 0xFF).all(-1).any())


def check_kernel(mode, r):
    assert r["report"]["kernel"] == gc.KERNEL[mode], r["report"]
    if mode == "dcn_fused":
        assert not r["report"]["persistent"] and r["report"]["cus"] >= 8
    if mode == "warp_dual":
        assert r["report"]["split"]


# ---------------------------------------------------------------- a. exact inputs
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("row", gc.EXACT_ROWS, ids=ROW_ID)
def test_exact(row, storage):
    """Bit for bit against float64 (bf16 build: rne_bf16 of it).  The fused modes run with a saturated head, once per sign table: a wrong
    ST_DCNFUSE row order, a swapped (dy, dx) or a wrong sign fails here.  Whether the hardware exp / rcp return exactly inf, 0 and 1 at +-200 is
    what these cases measure on the first run."""
    mode, (h, w) = row
    for table in gc.SAT_TABLES.get(mode, (0,)):
        inp, ref = gc.case(mode, h, w, "exact", storage, table)
        assert gc.exact_ok(mode, ref)
        r = launch(mode, inp, storage, raw=True)
        check_kernel(mode, r)
        assert_same_bits(r["out"], gc.expected(ref["out"], storage), f"{mode} {h}x{w} {storage} table {table}")
        if mode == "warp_dual":
            assert_same_bits(r["out2"], gc.expected(ref["out2"], storage), f"{mode} {h}x{w} {storage} second tensor")
        check_untouched(r, storage)
        assert int(r["status"].abs().sum()) == 0


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", ((5, 33), (23, 45)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_with_fine_weights(shape, storage):
    """dcn_g8 with weights of 13 significant bits: both fp16 parts of the weight image carry bits (fp32 build; the bf16 build rounds the weights
    to bf16 first, and so does its reference).  A dropped or misplaced low part fails here bit for bit."""
    h, w = shape
    inp, ref = gc.case("dcn_g8", h, w, "fine_w", storage)
    assert gc.exact_ok("dcn_g8", ref)
    r = launch("dcn_g8", inp, storage)
    check_kernel("dcn_g8", r)
    assert_same_bits(r["out"], gc.expected(ref["out"], storage), f"dcn_g8 fine weights {h}x{w} {storage}")


# ---------------------------------------------------------------- b. ordinary data
def check_bounded(what, mode, inp, ref, storage, r):
    b1, b2 = gc.bound(mode, inp, ref, storage)
    worst = 0.0
    for got, want, b in ((r["out"], ref["out"], b1), (r["out2"], ref["out2"], b2)):
        if got is None:
            continue
        got = got.cpu().double().numpy()
        assert np.isfinite(got).all(), f"{what}: elements unwritten or not finite"
        err = np.abs(got - want)
        full = b + (2.0 ** -8 * np.abs(want) if storage == "bf16" else 0.0)
        worst = max(worst, float((err / full).max()))
        print(f"\n{what} {storage}: max |got - ref| = {err.max():.3e}, max err / bound = {(err / full).max():.3f}, "
              f"without the bf16 store = {(np.maximum(err - (full - b), 0) / b).max():.3f}")
        assert bool((err <= full).all()), (what, float((err / full).max()))
    return worst


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("row", gc.ROWS, ids=ROW_ID)
def test_bounded_error_on_ordinary_data(row, storage):
    """Standard-normal x, weights * 1.5 / sqrt(9 cin), planted displacements of R = 9, 64 and 2058 (one batch item each) with vectors of +-3e9:
    gather_cases.sampler_bound / fused_bound / warp_bound, plus 2^-8 |ref| for the bf16 store.  The fused modes run a second time with the head
    times 8: a tenth and more of the activations in the saturating tails."""
    mode, (h, w) = row
    for scale in ((1.0, 8.0) if mode.endswith("fused") else (1.0,)):
        inp, ref = gc.case(mode, h, w, "normal", storage, 0, scale)
        r = launch(mode, inp, storage)
        check_kernel(mode, r)
        check_bounded(f"{mode} {h}x{w} head x{scale:g}", mode, inp, ref, storage, r)
        assert int(r["status"].abs().sum()) == 0


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mixed", (True, False), ids=("mixed", "regular"))
@pytest.mark.parametrize("mode", ("dcn3", "dcn3_fused"))
def test_dcn3_regular_and_per_tap_paths(mode, mixed, storage):
    """dcn3_kernel's __all(regular) 4 x 4-neighbourhood path and its per-tap path: a field that keeps every wave row regular, and one that
    leaves 0.2 .. 0.8 of them regular (test_gather_cases.py asserts the shares)."""
    h, w = gc.BRANCH_SHAPE
    inp = gc.branch_inputs(mode, h, w, mixed)
    ref = gc.reference(mode, inp, storage)
    r = launch(mode, inp, storage)
    check_kernel(mode, r)
    check_bounded(f"{mode} {'mixed' if mixed else 'regular'}", mode, inp, ref, storage, r)


# ---------------------------------------------------------------- c. batches, the dual warp
def _item(inp, b):
    return {k: (v if v is None or k in ("weight", "bias", "head_w", "head_b") else v[b:b + 1]) for k, v in inp.items()}


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("row", gc.ROWS, ids=ROW_ID)
def test_batch_equals_single_items(row, storage):
    """n = 3 == three n = 1 calls, bit for bit: batch strides, the status words and (dcn_fused) the tile list across batch items."""
    mode, (h, w) = row
    inp, _ = gc.case(mode, h, w, "normal", storage)
    whole = launch(mode, inp, storage)
    for b in range(gc.N):
        one = launch(mode, _item(inp, b), storage)
        check_kernel(mode, one)
        assert_same_bits(whole["out"][b:b + 1], one["out"].cpu(), f"{mode} {h}x{w} item {b}")
        if mode == "warp_dual":
            assert_same_bits(whole["out2"][b:b + 1], one["out2"].cpu(), f"{mode} {h}x{w} item {b}, second tensor")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", gc.SHAPES["warp_dual"], ids=lambda s: f"{s[0]}x{s[1]}")
def test_warp_dual_equals_two_warps(shape, storage):
    """Bit for bit, the 8-quad and the 6-quad tensor (whose second group is the cnt == 2 tail of the split kernel); the 4-channel launch is the
    8x state warp's."""
    h, w = shape
    inp, _ = gc.case("warp_dual", h, w, "normal", storage)
    dual = launch("warp_dual", inp, storage)
    check_kernel("warp_dual", dual)
    a = launch("warp", dict(inp, x2=None), storage)
    b = launch("warp", dict(inp, x=inp["x2"], x2=None), storage)
    c4 = launch("warp", dict(inp, x2=None), storage, c=4)
    for r in (a, b, c4):
        check_kernel("warp", r)
    assert_same_bits(dual["out"], a["out"].cpu(), f"warp_dual {h}x{w}: 32-channel tensor")
    assert_same_bits(dual["out2"], b["out"].cpu(), f"warp_dual {h}x{w}: 24-channel tensor")
    assert_same_bits(c4["out"], a["out"][:, :4].cpu(), f"warp {h}x{w}: one quad")


@pytest.mark.parametrize("storage", STORAGES)
def test_unsplit_dual_warp(storage):
    """N = 16 384 items of a 1 x 2 map: N * 4 groups do not fit the grid's z axis, the launcher falls back to flow_warp_p4_dual_kernel."""
    n = 16384
    inp = gc.make_inputs("warp_dual", 1, 2, "exact", n=n, seed=5)
    r = launch("warp_dual", inp, storage, raw=True)
    assert r["report"]["kernel"] == "flow_warp_p4_dual" and not r["report"]["split"]
    s = {k: gc.ref_x(inp, storage, k) for k in ("x", "x2")}
    assert_same_bits(r["out"], gc.expected(gc.warp_ref(s["x"], inp["flow"]), storage), "unsplit dual warp, 32 channels")
    assert_same_bits(r["out2"], gc.expected(gc.warp_ref(s["x2"], inp["flow"]), storage), "unsplit dual warp, 24 channels")
    check_untouched(r, storage)
    first = launch("warp_dual", {k: (None if v is None else v[:64]) for k, v in inp.items()}, storage)
    check_kernel("warp_dual", first)
    assert_same_bits(r["out"][:64], first["out"].cpu(), "unsplit against split, 32 channels")
    assert_same_bits(r["out2"][:64], first["out2"].cpu(), "unsplit against split, 24 channels")


# ---------------------------------------------------------------- d. the fused DCN launch
@pytest.mark.parametrize("storage", STORAGES)
def test_persistent_fused_walk(storage):
    """dcn_fused_kernel<8, true> in the product library: 3 x 5 maps, one tile each, as many items as the launcher's own threshold asks for
    (6 cus + 1 tiles).  Every item against float64 on exact inputs (a saturated head), the first and the last against a one-tile n = 1 call."""
    from crfp_amd import ops
    cus = ops.gather_probe_plan("dcn_fused", 1, 3, 5, storage=storage)["cus"]
    n = 6 * cus + 1
    plan = ops.gather_probe_plan("dcn_fused", n, 3, 5, storage=storage)
    assert plan["persistent"] and plan["tiles"] == n and plan["kernel"] == "dcn_fused_persistent"
    assert not ops.gather_probe_plan("dcn_fused", 6 * cus - 1, 3, 5, storage=storage)["persistent"]   # the launcher's rule: tiles >= 6 cus
    inp = gc.make_inputs("dcn_fused", 3, 5, "exact", n=n, table=1, seed=11)
    r = launch("dcn_fused", inp, storage, raw=True)
    assert r["report"]["kernel"] == "dcn_fused_persistent" and r["report"]["persistent"] and r["report"]["tiles"] == n
    s = {k: gc.ref_x(inp, storage, k) for k in ("x", "aux", "weight", "head_w")}
    off, msk, _, _ = gc.head_ref(s["aux"], inp["flow"], s["head_w"], inp["head_b"], 144)
    ref = gc.dcn_ref64_batched(s["x"], off, msk, s["weight"], inp["bias"], 8)
    assert_same_bits(r["out"], gc.expected(ref, storage), "persistent dcn_fused")
    check_untouched(r, storage)
    assert int(r["status"].abs().sum()) == 0
    for b in (0, n - 1):
        one = launch("dcn_fused", _item(inp, b), storage)
        check_kernel("dcn_fused", one)
        assert_same_bits(r["out"][b:b + 1], one["out"].cpu(), f"persistent against one-tile, item {b}")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("which", ("exact", "normal"))
@pytest.mark.parametrize("shape", ((9, 33), (20, 36)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_fused_equals_g8_on_the_float64_heads_offsets(shape, which, storage):
    """The hook's dcn_fused against its dcn_g8 fed with the float64 head's offsets and masks rounded to fp32: within the fused bound on ordinary
    data, bit for bit where the head is saturated (and so exact)."""
    h, w = shape
    inp, ref = gc.case("dcn_fused", h, w, which, storage, 2)
    fused = launch("dcn_fused", inp, storage)
    g8 = launch("dcn_g8", dict(inp, aux=ref["off"].astype(np.float32), mask=ref["msk"].astype(np.float32), flow=None, head_w=None, head_b=None), storage)
    check_kernel("dcn_fused", fused)
    check_kernel("dcn_g8", g8)
    if which == "exact":
        assert_same_bits(fused["out"], g8["out"].cpu(), f"dcn_fused against dcn_g8 {h}x{w}")
        return
    b, _ = gc.bound("dcn_fused", inp, ref, storage)
    err = (fused["out"] - g8["out"]).abs().cpu().double().numpy()
    full = b + (2.0 ** -7 * np.abs(ref["out"]) if storage == "bf16" else 0.0)   # two bf16 stores
    print(f"\ndcn_fused against dcn_g8 {h}x{w} {storage}: max |d| = {err.max():.3e}, max d / bound = {(err / full).max():.3f}")
    assert bool((err <= full).all())


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mode", ("dcn_g8", "dcn_fused"))
def test_range_guard_words(mode, storage):
    """The epilogue's fp16-range guard, one word per batch item.  Zero DCN weights: a bias of 65504 raises every item's word, 65503 none.  With
    one centre-tap weight of 1 on a channel that is 1 in one batch item alone, 65503 + 1 = 65504 raises that item's word and no other."""
    h, w, n, k = 9, 33, 3, 1
    z = lambda *s: np.zeros(s, np.float32)   # noqa: E731
    inp = {"x": z(n, 32, h, w), "x2": None, "weight": z(32, 32, 3, 3), "bias": z(32)}
    if mode == "dcn_g8":
        inp.update(aux=z(n, 144, h, w), mask=np.ones((n, 72, h, w), np.float32), flow=None, head_w=None, head_b=None)
        one = 1.0
    else:   # a zero head: offsets 10 tanh(0) + 0, masks sigmoid(0) = 1/2
        inp.update(aux=z(n, 32, h, w), mask=None, flow=z(n, h, w, 2), head_w=z(216, 32, 3, 3), head_b=z(216))
        one = 2.0
    for bias, want in ((65504.0, [1, 1, 1]), (65503.0, [0, 0, 0])):
        inp["bias"][5] = bias
        r = launch(mode, inp, storage)
        check_kernel(mode, r)
        assert r["status"].cpu().tolist() == want, (bias, r["status"].cpu().tolist())
        assert float(r["out"][:, 5].min()) >= 65503.0 and float(r["out"].abs().sum() - r["out"][:, 5].abs().sum()) == 0.0
    inp["weight"][5, 7, 1, 1] = 1.0
    inp["x"][k, 7] = one
    r = launch(mode, inp, storage)
    check_kernel(mode, r)
    assert r["status"].cpu().tolist() == [0, 1, 0], r["status"].cpu().tolist()
    assert float(r["out"][k, 5].min()) >= 65504.0 and float(r["out"][0, 5].max()) == (65536.0 if storage == "bf16" else 65503.0)
