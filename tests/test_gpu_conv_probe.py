"""GPU: the engines' own MFMA conv kernels, one launch at a time, through the C-ABI's test hook crfp_conv_probe (crfp_amd.ops.conv_probe).

fp32 build: conv3x3_split8_kernel, conv3x3_split_kernel<1,1,2>, conv3x3_split_dual_kernel (and the fp32-MFMA fallback); bf16 build:
conv3x3_bf16_kernel<1>, conv3x3_bf16x8_kernel, conv3x3_bf16_pair_kernel.  Every test asserts the kernel variant it means to test, that no
element of a destination stayed unwritten (the probe pre-fills them with NaN), and -- on the exact inputs of tests/conv_cases.py -- that
the result is the float64 reference bit for bit (bf16 build: its bf16 rounding).  On ordinary data the error is held to bounds derived
from the arithmetic, not tuned (see test_bounded_error_on_ordinary_data)."""
import dataclasses

import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STORAGES = ("f32", "bf16")


def probe(conv, inp, storage, **kw):
    from crfp_amd import ops
    return ops.conv_probe(cc.probe_spec(conv, inp, DEV), storage=storage, **kw)


def stored(ref_t, storage, conv=None):
    """What a correct kernel stores for an exactly computed value: itself, or its bf16 rounding in the bf16 build's activation tensors."""
    if storage == "bf16" and not (conv is not None and (conv.dst_f32 or conv.store == "offmask")):
        return cc.rne_bf16(ref_t).float()
    return ref_t.float()


def assert_same_bits(got, want, what):
    got = got.cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements unwritten or not finite"
    if not torch.equal(got, want):
        bad = got != want
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, max |d| = {float((got - want).abs().max()):.3e}, "
                             f"first at {idx}: got {got[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}")


# fp32 build: fine x against coarse weights, and coarse x against fine weights; bf16 build: both coarse (bf16 values)
EXACT_RUNS = (("f32", "fine_x"), ("f32", "fine_w"), ("bf16", "coarse"))
RUN_ID = lambda r: f"{r[0]}-{r[1]}"


# ---------------------------------------------------------------- a. exactness
@pytest.mark.parametrize("run", EXACT_RUNS, ids=RUN_ID)
@pytest.mark.parametrize("case", cc.EXACT, ids=lambda c: c.name)
def test_exact(case, run):
    storage, which = run
    case, inp, ref = cc.exact_case(case.name, which)
    r = probe(case.conv, inp, storage)
    assert r["kernel"] == (case.kernel[storage == "bf16"], "none")
    assert len(r["out"][0]) == len(ref["out"])
    for d, (got, want) in enumerate(zip(r["out"][0], ref["out"])):
        assert_same_bits(got, stored(want, storage, case.conv), f"{case.name} destination {d}")
    assert int(r["status"].abs().sum()) == 0


# ---------------------------------------------------------------- b. dispatch edges
@pytest.mark.parametrize("storage", STORAGES)
def test_batch_of_513_tiles_and_its_first_item_alone(storage):
    """N * 8-row tiles = 513: the bf16 build leaves its 8-wave kernel (one round of 512 slots), n = 1 stays on it; both are exact, so item 0
    of the batch equals the one-item call although another kernel computed it."""
    case, inp, ref = cc.exact_case("edge513", "coarse" if storage == "bf16" else "fine_x")
    r = probe(case.conv, inp, storage)
    assert r["kernel"][0] == case.kernel[storage == "bf16"]
    want = stored(ref["out"][0], storage)
    assert_same_bits(r["out"][0][0], want, "n = 19")
    one = dict(inp, srcs=[t[:1] for t in inp["srcs"]])
    r1 = probe(case.conv, one, storage)
    assert r1["kernel"][0] == cc.EDGE_1.kernel[storage == "bf16"]
    assert_same_bits(r1["out"][0][0], want[:1], "n = 1")
    assert torch.equal(r1["out"][0][0][0], r["out"][0][0][0])


@pytest.mark.parametrize("run", EXACT_RUNS + (("f32", "normal"), ("bf16", "normal")), ids=RUN_ID)
@pytest.mark.parametrize("name", [d[0] for d in cc.DUAL])
def test_dual_launch_equals_two_single_launches(name, run):
    storage, which = run
    _, n, h, w, k32, k16 = {d[0]: d for d in cc.DUAL}[name]
    if which == "normal":
        ia, ib = cc.make_inputs(cc.DUAL_A, n, h, w, "normal", 3), cc.make_inputs(cc.DUAL_B, n, h, w, "normal", 4)
        refs = None
    else:
        _, _, _, (ia, ib), refs = cc.dual_case(name, which)
    from crfp_amd import ops
    r = ops.conv_probe(cc.probe_spec(cc.DUAL_A, ia, DEV), cc.probe_spec(cc.DUAL_B, ib, DEV), mode="dual", storage=storage)
    assert r["kernel"] == (k16 if storage == "bf16" else k32)
    for k, (conv, inp) in enumerate(((cc.DUAL_A, ia), (cc.DUAL_B, ib))):
        single = probe(conv, inp, storage)
        assert_same_bits(r["out"][k][0], single["out"][0][0].cpu(), f"{name} half {k} against its single launch")
        if refs is not None:
            assert_same_bits(r["out"][k][0], stored(refs[k]["out"][0], storage), f"{name} half {k} against float64")
    assert int(r["status"].abs().sum()) == 0


@pytest.mark.parametrize("resid", [0, 1])
@pytest.mark.parametrize("hw", cc.PAIR_GEOMETRY, ids=lambda g: f"{g[0]}x{g[1]}")
def test_pair_kernel_equals_its_two_launch_composition(hw, resid):
    """bf16 build: conv a -> conv b in one launch, 62-column tiles, the tensor between them in LDS as rne_bf16(relu(a) * post_scale)."""
    from crfp_amd import ops
    conv_b, ia, ib, mid, ra, rb = cc.pair_case(hw[0], hw[1], resid)
    r = ops.conv_probe(cc.probe_spec(cc.PAIR_A, ia, DEV), cc.probe_spec(conv_b, ib, DEV), mode="pair", storage="bf16")
    assert r["kernel"] == ("bf16_pair", "bf16_pair")
    a_alone = probe(dataclasses.replace(cc.PAIR_A, dsts=None), ia, "bf16")
    assert_same_bits(a_alone["out"][0][0], mid.float(), "conv a alone")
    b_alone = probe(conv_b, dict(ib, srcs=[a_alone["out"][0][0]]), "bf16")
    assert_same_bits(r["out"][1][0], b_alone["out"][0][0].cpu(), "pair against two launches")
    assert_same_bits(r["out"][1][0], cc.rne_bf16(rb["out"][0]).float(), "pair against float64")
    assert int(r["status"].abs().sum()) == 0


def test_pair_mode_is_refused_by_the_fp32_build():
    conv_b, ia, ib, *_ = cc.pair_case(8, 62, 0)
    from crfp_amd import ops
    with pytest.raises(RuntimeError, match="bf16 build only"):
        ops.conv_probe(cc.probe_spec(cc.PAIR_A, ia, DEV), cc.probe_spec(conv_b, ib, DEV), mode="pair", storage="f32")


@pytest.mark.parametrize("which", ["fine_x", "fine_w", "normal"])
def test_s3_chain_equals_the_q4_path(which):
    """fp32 build: conv a stores only the pre-split fp16 pair image, conv b reads it: the same bits as through an fp32 Q4 tensor, and on
    exact inputs the float64 result."""
    from crfp_amd import ops
    ia, ib, ra, rb = cc.chain_case(which)
    r = ops.conv_probe(cc.probe_spec(cc.CHAIN_A, ia, DEV), cc.probe_spec(cc.CHAIN_B, ib, DEV), mode="s3_chain", storage="f32")
    assert r["kernel"] == ("split8", "split4")
    a_alone = probe(dataclasses.replace(cc.CHAIN_A, dsts=None), ia, "f32")
    b_alone = probe(cc.CHAIN_B, dict(ib, srcs=[a_alone["out"][0][0]]), "f32")
    assert_same_bits(r["out"][1][0], b_alone["out"][0][0].cpu(), "through S3 against through Q4")
    if which != "normal":
        assert_same_bits(a_alone["out"][0][0], ra["full"].float(), "conv a")
        assert_same_bits(r["out"][1][0], rb["out"][0].float(), "chain against float64")
    assert int(r["status"].abs().sum()) == 0


# ---------------------------------------------------------------- c. bounded error on ordinary data
def _k_padded(conv):
    quads = sum({"q4": (s[1] + 3) // 4, "flow2": 1, "unshuf4": ((s[1] // 16 + 3) // 4) * 16}[s[0]] for s in conv.srcs)
    return 4 * ((quads + 3) // 4 * 4)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", cc.NORMAL, ids=lambda c: c.name)
def test_bounded_error_on_ordinary_data(case, storage):
    """Standard-normal x, weights * 1.5 / sqrt(9 cin): both operands carry full mantissas, so the x1 w1 term the f16x3 scheme drops is live.
    With S = sum |x| |w| + |b| per output and n = 9 * cin_padded + 3 additions:
      fp32 build: |got - ref64| <= (2^-22 + n 2^-24) S   (the dropped term is below 2^-22 |x| |w|; the rest is worst-case
                  fp32 accumulation);
      bf16 build: the reference sees the operands as the kernel does (x, w and the flow channels rounded to bf16, the bias not):
                  <= n 2^-24 S, plus 2^-8 |ref| for the one storage rounding;
      offset / mask store: 3e-6 on the offsets and 3e-7 on the masks (the hardware exp / rcp forms, conv_mfma.hip and crfp_common.h),
                  plus the conv bound times the activation's Lipschitz constant, 10 and 1/4.
    lrelu(0.1) has Lipschitz constant 1.  Measured max |got - ref| / S: DESIGN.md section 4."""
    conv = case.conv
    inp = cc.make_inputs(conv, case.n, case.h, case.w, "normal", seed=7)
    seen = inp
    if storage == "bf16":
        rb = lambda t: cc.rne_bf16(t).float()
        seen = dict(inp, srcs=[rb(t) for t in inp["srcs"]], weight=rb(inp["weight"]))
        if "weight2" in inp:
            seen["weight2"] = rb(inp["weight2"])
    ref = cc.reference(conv, seen)
    r = probe(conv, inp, storage)
    assert r["kernel"] == (case.kernel[storage == "bf16"], "none")
    got = r["out"][0][0].cpu().double()
    assert bool(torch.isfinite(got).all())
    n_add = 9 * _k_padded(conv) + 3
    S = ref["S"]
    conv_bound = ((2.0 ** -22 if storage == "f32" else 0.0) + n_add * 2.0 ** -24) * S
    err = (got - ref["full"]).abs()
    storage_round = 2.0 ** -8 * ref["full"].abs() if storage == "bf16" and conv.store != "offmask" else torch.zeros_like(err)
    print(f"\nconv_probe {case.name} {storage}: kernel {r['kernel'][0]}, n = {n_add}, max |got - ref| / S = {float((err / S).max()):.3e}, "
          f"max (|got - ref| - storage rounding) / S = "
          f"{float(((err - storage_round).clamp(min=0) / S).max()):.3e} (bound {float((conv_bound / S).max()):.3e}), max |got - ref| = {float(err.max()):.3e}")
    if conv.store == "offmask":
        noff = 4 * conv.n_off_quads
        assert bool((err[:, :noff] <= 3e-6 + 10.0 * conv_bound[:, :noff]).all()), float((err[:, :noff] - 10.0 * conv_bound[:, :noff]).max())
        assert bool((err[:, noff:] <= 3e-7 + 0.25 * conv_bound[:, noff:]).all()), float((err[:, noff:] - 0.25 * conv_bound[:, noff:]).max())
    else:
        bound = conv_bound + storage_round
        assert bool((err <= bound).all()), float((err / S).max())
    assert int(r["status"].abs().sum()) == 0


# ---------------------------------------------------------------- d. range guard
def _guard_inputs(conv, n, h, w):
    """Channel 5 = 65503 everywhere (the bias); item 1 adds 1 at the far corner through a centre-tap weight of 1: 65504, there alone."""
    cin = conv.cin
    x = torch.zeros(n, cin, h, w)
    x[1, 0, h - 1, w - 1] = 1.0
    wgt = torch.zeros(conv.cout, cin, 3, 3)
    wgt[5, 0, 1, 1] = 1.0
    b = torch.zeros(conv.cout)
    b[5] = 65503.0
    return {"srcs": [x], "weight": wgt, "bias": b}


@pytest.mark.parametrize("storage", STORAGES)
def test_range_guard_raises_only_the_item_that_stored_65504(storage):
    conv = cc.Conv((cc.Q(32),), 32)
    inp = _guard_inputs(conv, 3, 5, 65)
    r = probe(conv, inp, storage)
    assert r["kernel"][0] == ("bf16_x8" if storage == "bf16" else "split8")
    st = r["status"].cpu()
    assert st[0].tolist() == [0, 1, 0] and st[1].tolist() == [0, 0, 0]          # 65503 raises nothing, 65504 its own item's word
    want = torch.zeros(3, 32, 5, 65)
    want[:, 5] = 65503.0
    want[1, 5, 4, 64] = 65504.0
    assert_same_bits(r["out"][0][0], stored(want.double(), storage), "guard case")
    # the 4-wave kernels (two cout tiles), the value in the second tile
    conv2 = cc.Conv((cc.Q(32),), 64)
    inp2 = _guard_inputs(conv2, 3, 5, 65)
    for t in (inp2["weight"], inp2["bias"]):
        t[40] = t[5].clone()
        t[5] = 0
    r2 = probe(conv2, inp2, storage)
    assert r2["kernel"][0] == ("bf16_4w" if storage == "bf16" else "split4")
    assert r2["status"].cpu()[0].tolist() == [0, 1, 0]
    # strict fp32 and the offset / mask store never raise: nothing downstream makes an fp16 operand of them
    rs = probe(dataclasses.replace(conv, strict=True), inp, storage)
    assert rs["kernel"][0] == "mfma_rows4" and int(rs["status"].abs().sum()) == 0
    assert_same_bits(rs["out"][0][0], stored(want.double(), storage), "strict guard case")
    om = cc.Conv((cc.Q(32),), 32, store="offmask", cout_split=16, n_off_quads=4)
    io = _guard_inputs(dataclasses.replace(om, cout=16), 3, 5, 65)
    io.update(weight2=torch.zeros(16, 32, 3, 3), bias2=torch.full((16,), 70000.0), flow=torch.zeros(3, 5, 65, 2))
    ro = probe(om, io, storage)
    assert int(ro["status"].abs().sum()) == 0
    out = ro["out"][0][0].cpu()
    assert bool(torch.isfinite(out).all()) and float(out[:, 5].min()) == 10.0 and float(out[:, 16:].min()) == 1.0 and float(out[:, 0].abs().max()) == 0.0


@pytest.mark.parametrize("storage", STORAGES)
def test_padded_destination_keeps_its_pad_row_and_column(storage):
    case, inp, ref = cc.exact_case("three_dsts", "coarse" if storage == "bf16" else "fine_x")
    r = probe(case.conv, inp, storage, raw=True)
    eb = 2 if storage == "bf16" else 4
    for d, (q0, q1, *pad) in enumerate(case.conv.dsts):
        pad = pad[0] if pad else 0
        raw = r["raw"][0][d].cpu().reshape(case.n, q1 - q0, case.h + pad, case.w + pad, 4 * eb)
        assert not bool((raw[:, :, :case.h, :case.w] == 0xFF).all(-1).any()), f"destination {d}: an unwritten quad"
        if pad:
            assert bool((raw[:, :, case.h] == 0xFF).all()) and bool((raw[:, :, :, case.w] == 0xFF).all()), f"destination {d}: pad touched"
    assert sum(len(p) > 2 and p[2] for p in case.conv.dsts) == 1
