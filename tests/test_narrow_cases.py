"""CPU pins of tests/narrow_cases.py: an exact case is one the reference alone proves exact, and the restatement of the narrow launch agrees
with plain ATen formulas written independently of it."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as cc   # noqa: E402
import narrow_cases as nc   # noqa: E402

SMALL = [c.name for c in nc.EXACT]


@pytest.mark.parametrize("run", nc.EXACT_RUNS, ids=lambda r: f"{r[0]}-{r[1]}")
@pytest.mark.parametrize("name", SMALL)
def test_every_exact_case_satisfies_the_bound_at_every_stage(name, run):
    storage, which = run
    case, inputs, refs = nc.case_data(name, storage, which)
    assert nc.exact_ok(case, inputs, refs), (name, storage, [r["S"].max().item() for r in refs])
    if storage == "f32":   # the case really has a fine operand: exactness is not trivially true
        i, j = nc._bits(refs[0]["x"]), nc._bits(refs[0]["wq"])
        assert max(i, j) == 12 and min(i, j) == 1
    else:                  # bf16: every operand the kernel reads is a bf16 value
        for r in refs:
            assert torch.equal(cc.rne_bf16(r["x"]), r["x"]) and torch.equal(cc.rne_bf16(r["wq"]), r["wq"])
            assert torch.equal(cc.rne_bf16(refs[-1]["out"]), refs[-1]["out"]) or case.st[-1].epi == "last"


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in nc.WALK])
def test_walk_cases_satisfy_the_bound_at_the_first_height(name, storage):
    """The persistent-walk cases at the smallest height of their ladder (the GPU test picks the height from the launcher's report); the inputs
    of every height come from the same generator, and S is a per-pixel quantity that does not grow with the map."""
    case, inputs, refs = nc.case_data(name, storage, None, nc.WALK_HEIGHTS[0])
    assert nc.exact_ok(case, inputs, refs)


def test_exact_cases_cover_the_issue():
    geo = {(c.h, c.w) for c in nc.EXACT}
    assert geo >= {(1, 1), (15, 63), (16, 64), (17, 65), (16, 60), (17, 61), (49, 193), (49, 181)}
    assert {c.n for c in nc.EXACT} == {1, 3}
    singles = [c.st[0] for c in nc.EXACT if c.mode == "single"]
    assert {tuple(s[1] for s in st.srcs) for st in singles} >= {(3, 3), (4,), (4, 4), (4, 4, 2), (2,)}
    assert {st.cout for st in singles} == {1, 2, 3, 4} and {st.act for st in singles} == {"none", "relu"}
    assert any(st.post_scale == 0.5 for st in singles) and any(st.residual for st in singles)
    assert {st.src_pad for st in singles} == {0, 1, 37} and {st.epi for st in singles} == {"plain", "blend", "last"}
    assert {st.y_only for st in singles if st.epi == "last"} == {False, True}
    f32 = {c.kern[0] for c in nc.EXACT}
    assert f32 >= {f"chain<{k},{g},{r}>" for k in (1, 2, 3) for g, r in ((0, "res"), (1, "nores"), (0, "nores"))}
    assert f32 >= {"pair<1,plain>", "pair<2,plain>", "pair<3,plain>", "narrow<1,plain,st2>", "seq<1>", "seq<2>", "seq<3>"}
    bf16 = {c.kern[1] for c in nc.EXACT}
    assert bf16 >= {"chain<1,0,res>", "chain<2,0,res>", "chain<1,1,nores>", "chain<2,1,nores>", "chain<3,1,nores>", "narrow<1,plain>", "narrow<2,plain>",
                    "narrow<3,plain>"}


def _ordinary(st, n=2, h=11, w=19, seed=3):
    case = nc.Case("t", "single", (st,), n, h, w, "normal")
    return case, nc.make_inputs(case, "f32", seed=seed)


@pytest.mark.parametrize("srcs,cout", [((nc.Q(3), nc.Q(3)), 2), ((nc.Q(4), nc.Q(4), nc.FLOW), 4), ((nc.Q(2),), 1)])
def test_plain_reference_is_conv2d_in_double(srcs, cout):
    st = nc.Stencil(srcs, cout, act="lrelu", post_scale=0.5, residual=True)
    case, inp = _ordinary(st)
    ref = nc.reference(case, inp, "f32")[0]
    x = torch.cat([t.double() if s[0] == "q4" else t.double().permute(0, 3, 1, 2) for s, t in zip(srcs, inp[0]["srcs"])], 1)
    want = F.leaky_relu(F.conv2d(x, inp[0]["weight"].double(), inp[0]["bias"].double(), padding=1), 0.1) * 0.5
    got = ref["out"]
    assert (got[:, :cout] - inp[0]["residual"].double()[:, :cout] - want).abs().max().item() < 1e-7   # 0.1f against 0.1, one fp32 rounding
    assert torch.equal(got[:, cout:], inp[0]["residual"].double()[:, cout:])


def test_blend_and_last_references_against_the_fovea_head_formulas():
    rs = np.random.RandomState(5)
    st = nc.Stencil((nc.Q(4), nc.Q(4)), 4, epi="blend")
    case, inp = _ordinary(st, h=16, w=24)
    ref = nc.reference(case, inp, "f32")[0]
    state, x_hr = inp[0]["srcs"][0].double(), inp[0]["srcs"][1].double()
    mk = inp[0]["mask"].double()
    f2 = F.conv2d(torch.cat((state, x_hr), 1), inp[0]["weight"].double(), inp[0]["bias"].double(), padding=1)
    assert (ref["out"] - F.leaky_relu(mk * f2 + (1 - mk) * state, 0.1)).abs().max().item() < 1e-7
    assert 0.2 < mk.mean().item() < 0.8
    for y_only in (False, True):
        st = nc.Stencil((nc.Q(4),), 1 if y_only else 3, epi="last", y_only=y_only)
        case, inp = _ordinary(st, h=16, w=24)
        ref = nc.reference(case, inp, "f32")[0]
        base = F.interpolate(inp[0]["base_lr"].double(), scale_factor=8, mode="bilinear", align_corners=False)
        if y_only:
            base = 0.299 * base[:, 0:1] + 0.587 * base[:, 1:2] + 0.114 * base[:, 2:3]
        want = F.conv2d(inp[0]["srcs"][0].double(), inp[0]["weight"].double(), inp[0]["bias"].double(), padding=1) + base
        assert ref["out"].shape == want.shape and (ref["out"] - want).abs().max().item() < (3e-7 if y_only else 1e-12)
    del rs


def test_offmask3_reference_against_conv_cases():
    st = nc.Stencil((nc.Q(4),), 3, epi="offmask3", cout_split=2)
    case, inp = _ordinary(st)
    ref = nc.reference(case, inp, "f32")[0]
    d = inp[0]
    # conv_cases: one offset quad (dy, dx, dy, dx) and one mask quad; the narrow triple is (dy, dx, mask) of a 4 -> 3 head
    w8 = torch.cat([d["weight"], d["weight"], d["weight2"].repeat(4, 1, 1, 1)], 0)
    b8 = torch.cat([d["bias"], d["bias"], d["bias2"].repeat(4)], 0)
    conv = cc.Conv((cc.Q(4),), 8, store="offmask", n_off_quads=1)
    want = cc.reference(conv, {"srcs": d["srcs"], "weight": w8, "bias": b8, "flow": d["flow"]})["full"]
    assert torch.equal(ref["out"][:, :2], want[:, :2]) and torch.equal(ref["out"][:, 2], want[:, 4]) and not ref["out"][:, 3].any()


def test_pair_and_chain_references_are_compositions():
    case = next(c for c in nc.COMPOSE if c.name == "c_chain_k3_g")
    for storage in ("f32", "bf16"):
        inputs = nc.make_inputs(case, storage)
        refs = nc.reference(case, inputs, storage)
        a = nc.stage_reference(case.st[0], inputs[0], storage)
        b = nc.stage_reference(case.st[1], inputs[1], storage, fed=a["out"])
        c = nc.stage_reference(case.st[2], inputs[2], storage, fed=b["out"])
        assert torch.equal(refs[2]["out"], c["out"]) and refs[2]["x"].shape[1] == 8
        if storage == "bf16":
            assert torch.equal(cc.rne_bf16(a["out"]), a["out"]) and torch.equal(cc.rne_bf16(b["out"]), b["out"])
    res = next(c for c in nc.COMPOSE if c.name == "c_chain_k2_res")
    inputs = nc.make_inputs(res, "f32")
    refs = nc.reference(res, inputs, "f32")
    plain = nc.reference(dataclasses.replace(res, res=False), inputs, "f32")
    assert torch.equal(refs[2]["out"], plain[2]["out"] + refs[0]["out"])
    assert torch.equal(refs[2]["out2"], nc.lrelu32(refs[2]["out"]))


def test_lrelu_is_the_fp32_product():
    v = torch.tensor([-3.0, -1.0 - 2.0 ** -20, 0.0, 2.5], dtype=torch.float64)
    got = nc.lrelu32(v)
    want = torch.tensor([float(np.float32(np.float32(0.1) * np.float32(x))) if x < 0 else x for x in v.tolist()], dtype=torch.float64)
    assert torch.equal(got, want)


def test_bilinear_restatement_is_exact_on_quarters():
    lr = torch.from_numpy(np.random.RandomState(1).randint(0, 5, (1, 3, 2, 3)) * 0.25)
    up = nc.bilinear_x8(lr)
    assert up.shape == (1, 3, 16, 24) and nc._bits(up) <= 10
    assert torch.equal(up, F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False))


def test_gate_flags_definition():
    m = nc.gate_mask("interior")
    f0, f1 = nc.gate_flags(m, 0), nc.gate_flags(m, 1)
    assert f0.sum() == 1 and f0[0, 2, 2] and f1[0].sum() == 9 and not f1[1].any()
    assert not nc.gate_flags(nc.gate_mask("empty"), 3).any()
    s = nc.gate_flags(nc.gate_mask("straddle"), 0)
    assert s[0, 1, 1] and s[0, 2, 1] and s[0, 1, 2] and s[0, 2, 2] and s[1, 0, 0] and s[1, 1, 1] and s[1, 0, 1] and s[1, 1, 0]
