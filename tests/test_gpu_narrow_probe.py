"""GPU: the 8x narrow conv kernels of csrc/conv_narrow.hip, one launch at a time, through the C-ABI's test hook crfp_narrow_probe
(crfp_amd.ops.narrow_probe): conv3x3_narrow_kernel<KQ, EPI, GATE, ST2>, conv3x3_narrow_seq_kernel (fp32 build), conv3x3_narrow_pair_kernel and
both texts of conv3x3_narrow_chain_kernel.

Every test asserts the kernel variant it means to reach and -- unless it is about elements that must stay unwritten -- that no destination
element kept its NaN prefill.  On the exact inputs of tests/narrow_cases.py the result is the float64 reference bit for bit (bf16 build: with
its storage roundings); on ordinary data the error is held to bounds derived from the arithmetic (test_bounded_error_on_ordinary_data)."""
import dataclasses

import numpy as np
import pytest
import torch

import narrow_cases as nc
from conv_cases import conv3x3_f64, rne_bf16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STORAGES = ("f32", "bf16")
RUN_ID = lambda r: f"{r[0]}-{r[1]}"


def launch(case, inputs, storage, **kw):
    from crfp_amd import ops
    specs = nc.probe_specs(case, inputs, DEV)
    return ops.narrow_probe(*specs, mode=case.mode, storage=storage, res=case.res, **kw)


def assert_same_bits(got, want, what):
    got, want = got.cpu(), want.float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements unwritten or not finite"
    if not torch.equal(got, want):
        bad = got != want
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, max |d| = {float((got - want).abs().max()):.3e}, "
                             f"first at {idx}: got {got[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}")


def check_pads(case, r, storage):
    """Padded planes (pad 1) and window destinations (pitch excess p): every quad of the window written, every byte outside it as prefilled."""
    st, eb = case.st[-1], (2 if storage == "bf16" else 4)
    if st.dst_pad:
        p = st.dst_pad
        raw = r["raw"].cpu().reshape(case.n, case.h + p, case.w + p, 4 * eb)
        assert not bool((raw[:, :case.h, :case.w] == 0xFF).all(-1).any()), "an unwritten quad inside the window"
        assert bool((raw[:, case.h:] == 0xFF).all()) and bool((raw[:, :, case.w:] == 0xFF).all()), "bytes outside the destination window touched"
    if st.dst2:
        raw = r["raw2"].cpu().reshape(case.n, case.h + 1, case.w + 1, 4 * eb)
        assert not bool((raw[:, :case.h, :case.w] == 0xFF).all(-1).any()), "an unwritten quad of the second destination"
        assert bool((raw[:, case.h] == 0xFF).all()) and bool((raw[:, :, case.w] == 0xFF).all()), "pad row / column of the second destination touched"


def check_exact(case, inputs, refs, storage, r):
    assert nc.variant(r["report"]) == case.kern[storage == "bf16"]
    assert_same_bits(r["out"], refs[-1]["out"], f"{case.name} dst")
    if case.st[-1].dst2:
        assert_same_bits(r["out2"], refs[-1]["out2"], f"{case.name} dst2")
    else:
        assert r["out2"] is None
    check_pads(case, r, storage)
    assert int(r["status"].abs().sum()) == 0


# ---------------------------------------------------------------- a. exactness
@pytest.mark.parametrize("run", nc.EXACT_RUNS, ids=RUN_ID)
@pytest.mark.parametrize("case", nc.EXACT, ids=lambda c: c.name)
def test_exact(case, run):
    """Bit for bit against float64.  LAST is held to bit equality too: with base_lr in multiples of 1/4 the kernel's bilinear weights k / 16 and
    their products are exact, and the y_only luma (0.299f r + 0.587f g + 0.114f b, three rounded products, two rounded sums) is restated in
    fp32 step by step (narrow_cases.luma32)."""
    storage, which = run
    if case.kern[storage == "bf16"] is None:   # a chain shape the bf16 launcher does not have: test_refusals
        from crfp_amd import ops
        with pytest.raises(RuntimeError, match="unsupported chain"):
            ops.narrow_probe(*nc.probe_specs(case, nc.make_inputs(case, storage), DEV), mode="chain", storage=storage, res=case.res)
        return
    case, inputs, refs = nc.case_data(case.name, storage, which)
    r = launch(case, inputs, storage, raw=True)
    check_exact(case, inputs, refs, storage, r)
    rep = r["report"]
    tw = 60 if rep["kernel"] == "chain" else 64
    assert rep["tiles"] == -(-case.w // tw) * -(-case.h // 16) and rep["workgroups"] == rep["tiles"]


def _single_launch(spec, storage, **kw):
    from crfp_amd import ops
    return ops.narrow_probe(spec, mode="single", storage=storage, **kw)


def compose(case, inputs, storage):
    """The launches a pair / chain replaces: one single launch per stencil, the tensors between them through device memory."""
    specs = nc.probe_specs(case, inputs, DEV)
    a = _single_launch(specs[0], storage)["out"]
    fed = a
    for k in range(1, len(specs)):
        spec = dict(specs[k])
        spec["srcs"] = [("q4", fed)] + list(spec["srcs"])
        if case.res and k == len(specs) - 1:
            spec["residual"] = a
        r = _single_launch(spec, storage)
        fed = r["out"]
    return r


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", [c for c in nc.EXACT if c.mode != "single"] + list(nc.COMPOSE), ids=lambda c: c.name)
def test_pair_and_chain_equal_the_composition_of_their_single_launches(case, storage):
    """Bit for bit, on exact inputs and on ordinary data with lrelu between the stages: the tensors between the stages are rounded where the
    separate launches store them, and every stage accumulates in its single kernel's order."""
    if case.kern[storage == "bf16"] is None:
        return
    case, inputs, refs = nc.case_data(case.name, storage)
    fused = launch(case, inputs, storage)
    assert nc.variant(fused["report"]) == case.kern[storage == "bf16"]
    sep = compose(case, inputs, storage)
    assert sep["report"]["kernel"] in ("narrow", "seq")
    assert_same_bits(fused["out"], sep["out"].cpu(), f"{case.name}: fused against separate launches")
    if case.st[-1].dst2:
        assert_same_bits(fused["out2"], sep["out2"].cpu(), f"{case.name}: second destination")
    assert int(fused["status"].abs().sum()) == 0


# ---------------------------------------------------------------- b. the persistent walk
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", nc.WALK, ids=lambda c: c.name)
def test_persistent_walk_is_exact(case, storage):
    """A map with more tiles than the launch has workgroups: every workgroup walks several tiles, the loads of tile t + 1 issued behind tile t's
    LDS write.  The height comes from the launcher's own sizing (the first of WALK_HEIGHTS at which it reports workgroups < tiles)."""
    from crfp_amd import ops
    plans = nc.plan_specs(case)
    h = None
    for cand in nc.WALK_HEIGHTS:
        rep = ops.narrow_probe_plan(*plans, mode=case.mode, storage=storage, res=case.res, n=1, h=cand, w=case.w)
        if rep["workgroups"] < rep["tiles"]:
            h = cand
            break
    assert h is not None, "no height of the ladder makes a workgroup walk more than one tile"
    case, inputs, refs = nc.case_data(case.name, storage, None, h)
    assert nc.exact_ok(case, inputs, refs)
    r = launch(case, inputs, storage)
    assert nc.variant(r["report"]) == case.kern[storage == "bf16"]
    assert r["report"]["workgroups"] == rep["workgroups"] < r["report"]["tiles"] == rep["tiles"]
    print(f"\nnarrow_probe {case.name} {storage}: {h} x {case.w}, {rep['tiles']} tiles on {rep['workgroups']} workgroups")
    assert_same_bits(r["out"], refs[-1]["out"], f"{case.name} at {h} x {case.w}")
    assert int(r["status"].abs().sum()) == 0


# ---------------------------------------------------------------- c. bounded error on ordinary data
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", nc.NORMAL, ids=lambda c: c.name)
def test_bounded_error_on_ordinary_data(case, storage):
    """Standard-normal x, weights * 1.5 / sqrt(9 cin), lrelu.  With S = sum |x| |w| + |b| per output and n_add = 9 * 4 * kq + 1 fp32 additions
    (every product of the 4x4x1 MFMA / the bf16 MFMA is exact or rounded once into the sum):
      conv + bias:   e = (n_add + 3) 2^-24 S -- the 3: the activation's product, post_scale, the epilogue's last addition (residual / base);
                     bf16 build: the reference sees x, w and the residual as the kernel does (rne_bf16; flow, bias and base_lr stay fp32), plus
                     2^-16 sum |flow| |w| for what the (hi, lo) bf16 split of a flow value leaves: hi = bf16(f), lo = bf16(f - hi), so
                     |f - hi - lo| <= 2^-9 |f - hi| <= 2^-18 |f|; the bound keeps the 16 bits two bf16 pieces guarantee;
      plain, blend:  e (lrelu has Lipschitz constant 1; a residual adds one rounding of the result, 2^-24 |ref|), bf16: + 2^-8 |ref| for the
                     storage rounding;
      last:          e + 8 * 2^-24 for the bilinear base on [0, 1] data (six rounded operations on values <= 1, and the luma's);
      offmask3:      3e-6 on the offsets and 3e-7 on the mask (the hardware exp / rcp forms, crfp_common.h), plus e times the Lipschitz
                     constants 10 and 1/4;
      pair:          stage b sees stage a's error: e_b + sum |w_b| e_a over the 3x3 window, e_a including (bf16) the rounding of the tensor
                     between the stages, 2^-8 |mid|.
    Measured max err / bound: DESIGN.md section 4."""
    case, inputs, refs = nc.case_data(case.name, storage)
    r = launch(case, inputs, storage)
    assert nc.variant(r["report"]) == case.kern[storage == "bf16"]
    got = r["out"].cpu().double()
    assert bool(torch.isfinite(got).all())
    st, ref = case.st[-1], refs[-1]
    e = nc.conv_bound(st, ref, storage)
    if len(refs) == 2:
        e_a = nc.conv_bound(case.st[0], refs[0], storage) + (2.0 ** -8 * refs[0]["out"].abs() if storage == "bf16" else 0.0)
        e = e + conv3x3_f64(e_a, ref["wq"].abs())[0]
    want = ref["unrounded"]   # bf16 build: the storage rounding of dst is in the bound, not in the reference
    err = (got - want).abs()
    if st.epi == "offmask3":
        bound = torch.cat([3e-6 + 10.0 * e[:, :2], 3e-7 + 0.25 * e[:, 2:3], torch.zeros_like(e[:, 3:])], 1)
    elif st.epi == "last":
        bound = e[:, :want.shape[1]] + 8 * 2.0 ** -24
    else:
        bound = e + (2.0 ** -24 * want.abs() if st.residual else 0.0) + (2.0 ** -8 * want.abs() if storage == "bf16" else 0.0)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), err)
    print(f"\nnarrow_probe {case.name} {storage}: kernel {nc.variant(r['report'])}, max err / bound = {float(ratio.max()):.3f}, "
          f"max |got - ref| = {float(err.max()):.3e}, max |got - ref| / S = {float((err / ref['S'][:, :err.shape[1]].clamp(min=1e-30)).max()):.3e}")
    assert bool((err <= bound).all()), float(ratio.max())
    assert int(r["status"].abs().sum()) == 0


# ---------------------------------------------------------------- d. the mask gate
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("mask_name", list(nc.GATE_MASKS))
@pytest.mark.parametrize("form", nc.GATED, ids=lambda f: f[0])
def test_gated_forms_write_flagged_tiles_only(form, mask_name, storage):
    """gate_h 0 .. 3: a written tile equals the dense launch's bits, an unwritten one keeps every prefill byte, and every tile within gate_h
    tiles (Chebyshev) of a tile with a set mask pixel is written.  With the empty mask nothing is written."""
    name, st = form
    n, h, w = nc.GATE_N, nc.GATE_H, nc.GATE_W
    case = nc.Case(name, "single", (st,), n, h, w, "normal")
    inputs = nc.make_inputs(case, storage)
    gmask = nc.gate_mask(mask_name)
    inputs[0]["mask"] = gmask   # the blend reads the mask the gate is built from, as in the engine
    dense = launch(case, inputs, storage)
    kq = len(st.srcs)
    assert nc.variant(dense["report"]) == (f"seq<{kq}>" if (st.epi == "plain" and storage == "f32") else f"narrow<{kq},{st.epi}>")
    want = dense["out"].cpu()
    assert bool(torch.isfinite(want).all())
    eb = 2 if storage == "bf16" else 4
    ty, tx = -(-h // nc.TILE_H), -(-w // nc.TILE_W)
    for gate_h in range(4):
        gcase = dataclasses.replace(case, st=(dataclasses.replace(st, gate_h=gate_h),))
        r = launch(gcase, inputs, storage, raw=True)
        assert nc.variant(r["report"]) == f"narrow<{kq},{st.epi},gate>"
        raw = r["raw"].cpu().reshape(n, h, w, 4 * eb)
        got = r["out"].cpu()
        must = nc.gate_flags(gmask, gate_h)
        written = np.zeros((n, ty, tx), dtype=bool)
        for i in range(n):
            for y in range(ty):
                for x in range(tx):
                    ys, xs = slice(y * nc.TILE_H, (y + 1) * nc.TILE_H), slice(x * nc.TILE_W, (x + 1) * nc.TILE_W)
                    written[i, y, x] = not bool((raw[i, ys, xs] == 0xFF).all())
                    if written[i, y, x]:
                        assert torch.equal(got[i, :, ys, xs], want[i, :, ys, xs]), f"gate_h {gate_h}: tile ({i}, {y}, {x}) differs from the dense launch"
        assert not (must & ~written).any(), f"gate_h {gate_h}: a tile within reach of the mask was skipped"
        if mask_name == "empty":
            assert not written.any()
        else:
            assert written.any() and not written.all()
        assert int(r["status"].abs().sum()) == 0


# ---------------------------------------------------------------- e. range guard
def _guard_case(kind):
    """Channel 1 = 65503 everywhere (the bias); item 1 adds 1 at the far corner through a centre-tap weight of 1: 65504, there alone."""
    n, h, w = 3, 17, 65
    if kind == "blend":
        st = nc.Stencil((nc.Q(4), nc.Q(4)), 4, epi="blend")
    else:
        st = nc.Stencil((nc.Q(4),), 4, dst2=True)
    cin = st.cin(False)
    x = torch.zeros(n, 4, h, w)
    x[1, 0, h - 1, w - 1] = 1.0
    wgt = torch.zeros(4, cin, 3, 3)
    wgt[1, 0, 1, 1] = 1.0
    b = torch.zeros(4)
    b[1] = 65503.0
    inp = {"srcs": [x] + [torch.zeros(n, 4, h, w)] * (len(st.srcs) - 1), "weight": wgt, "bias": b}
    if kind == "blend":
        inp["mask"] = torch.ones(n, 1, h, w, dtype=torch.uint8)
    return nc.Case("guard_" + kind, "single", (st,), n, h, w, "normal"), [inp]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kind", ["blend", "dst2"])
def test_range_guard_raises_only_the_item_that_stored_65504(kind, storage):
    case, inputs = _guard_case(kind)
    r = launch(case, inputs, storage)
    assert nc.variant(r["report"]) == ("narrow<2,blend>" if kind == "blend" else "narrow<1,plain,st2>")
    want = torch.zeros(3, 4, 17, 65, dtype=torch.float64)
    want[:, 1] = 65503.0
    want[1, 1, 16, 64] = 65504.0
    stored = rne_bf16(want) if storage == "bf16" else want
    assert_same_bits(r["out"], stored, "guard case dst")
    if kind == "dst2":
        assert_same_bits(r["out2"], stored, "guard case dst2")
    assert r["status"].cpu().tolist() == [0, 1, 0]          # 65503 raises nothing, 65504 its own item's word


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("y_only", [False, True])
def test_output_head_poisons_the_item_whose_word_is_set(y_only, storage):
    name = "last_y" if y_only else "last_rgb"
    case = dataclasses.replace({c.name: c for c in nc.EXACT}[name], n=3, h=16, w=64, name=name + "_poison")
    inputs = nc.make_inputs(case, storage)
    refs = nc.reference(case, inputs, storage)
    assert nc.exact_ok(case, inputs, refs)
    status = torch.tensor([0, 5, 0], dtype=torch.int32, device=DEV)
    r = launch(case, inputs, storage, status=status)
    assert nc.variant(r["report"]) == "narrow<1,last>"
    got = r["out"].cpu()
    assert bool(torch.isnan(got[1]).all())
    assert_same_bits(got[0::2], refs[-1]["out"][0::2], "items 0 and 2")
    assert r["status"].cpu().tolist() == [0, 5, 0]


# ---------------------------------------------------------------- f. refusals
@pytest.mark.parametrize("storage", STORAGES)
def test_refusals(storage):
    from crfp_amd import ops
    n, h, w = 1, 16, 64
    x = torch.zeros(n, 4, h, w, device=DEV)
    mk = torch.zeros(n, 1, h, w, dtype=torch.uint8, device=DEV)
    W = lambda co, ci: torch.zeros(co, ci, 3, 3, device=DEV)
    B = lambda co: torch.zeros(co, device=DEV)
    one = {"srcs": [("q4", x)], "weight": W(4, 4), "bias": B(4)}
    fed = {"srcs": [], "weight": W(4, 4), "bias": B(4)}
    go = lambda *a, **kw: ops.narrow_probe(*a, storage=storage, **kw)
    with pytest.raises(RuntimeError, match="unknown mode 3"):
        go(one, mode=3)
    with pytest.raises(RuntimeError, match=r"cout 5 \(1 .. 4\)"):
        go(dict(one, weight=W(5, 4), bias=B(5)))
    with pytest.raises(RuntimeError, match="4 sources"):
        go(dict(one, srcs=[("q4", x)] * 4, weight=W(4, 16)))
    with pytest.raises(RuntimeError, match="a pair's second stencil reads one quad"):
        go(one, dict(fed, srcs=[("q4", x)], weight=W(4, 8)), mode="pair")
    with pytest.raises(RuntimeError, match=r"conv_narrow_chain narrow_probe:chain: unsupported chain \(kqA=1 kqB=1 kqC=2 res=1\)"):
        go(one, fed, dict(fed, srcs=[("q4", x)], weight=W(4, 8)), mode="chain", res=True)
    if storage == "bf16":   # the bf16 launcher has no chain without a residual or a second global quad, and no residual chain of three quads
        with pytest.raises(RuntimeError, match=r"unsupported chain \(kqA=1 kqB=1 kqC=1 res=0\)"):
            go(one, fed, fed, mode="chain")
        with pytest.raises(RuntimeError, match=r"unsupported chain \(kqA=3 kqB=1 kqC=1 res=1\)"):
            go(dict(one, srcs=[("q4", x)] * 3, weight=W(4, 12)), fed, fed, mode="chain", res=True)
    with pytest.raises(RuntimeError, match="conv_narrow narrow_probe:a: no mask-gated form for kq=3 epi=0"):
        go(dict(one, srcs=[("q4", x)] * 3, weight=W(4, 12), mask=mk, gate_h=1))
    with pytest.raises(RuntimeError, match="no mask-gated form for kq=1 epi=1"):
        go(dict(one, epi="blend", mask=mk, gate_h=0))
    with pytest.raises(RuntimeError, match="no mask-gated form of a pair or chain"):
        go(one, dict(fed, mask=mk, gate_h=0), mode="pair")
    with pytest.raises(RuntimeError, match=r"a second destination needs a plain one-quad stencil \(kq=2 epi=0\)"):
        go(dict(one, srcs=[("q4", x)] * 2, weight=W(4, 8), dst2=True))
    with pytest.raises(RuntimeError, match="only the last stencil of a launch has a second destination or a gate"):
        go(dict(one, dst2=True), fed, mode="pair")
    with pytest.raises(RuntimeError, match="conv_narrow_pair narrow_probe:pair: unsupported pair"):
        go(dict(one, residual=x), fed, mode="pair")
