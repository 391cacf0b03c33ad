"""CPU: pins the cases of tests/warp_backward_cases.py (their float64 references, the conditions their flows and offsets are built to meet,
the written-down fp32 errors the GPU tolerances come from) and the host side of the four new C-ABI entry points -- no GPU here."""
import ctypes
import os
import subprocess

import pytest
import torch

import warp_backward_cases as wc
from conftest import ROOT

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", list(wc.CASES))
def test_written_down_fp32_error_is_the_measured_one(name):
    """TOL = 8 * max(E32, one ulp), and E32 is what measure_e32 gives here within a factor 2."""
    for mode in wc.MODES:
        got = wc.measure_e32(name, mode)
        for k in wc.GRADS:
            e = wc.E32[name][mode][k]
            assert wc.TOL[name][mode][k] == 8.0 * max(e, 2.0 ** -23)
            assert e / 2 <= got[k] <= e * 2, (mode, k, got[k], e)


@pytest.mark.parametrize("name", list(wc.SHARED_CASES))
def test_written_down_shared_fp32_error_is_the_measured_one(name):
    got = wc.measure_shared_e32(name)
    for k in wc.SHARED_GRADS:
        e = wc.SHARED_E32[name][k]
        assert wc.SHARED_TOL[name][k] == 8.0 * max(e, 2.0 ** -23)
        assert e / 2 <= got[k] <= e * 2, (k, got[k], e)


@pytest.mark.parametrize("name", wc.FRACTIONAL)
def test_every_sample_is_away_from_a_cell_boundary(name):
    """A condition, not a tolerance: the position pixel + flow has its fraction in [0.1, 0.9] on both axes in float64, and after the
    normalisation round trip float32 and float64 agree on every floor (along an axis of size 1 the coordinate is exactly 0 in both)."""
    c = wc.CASES[name]
    f = wc.reference_flow(name).double()
    frac = f - torch.floor(f)
    near = f.abs() < 4.0 * max(c["h"], c["w"])   # all but the replaced values of "nonfinite": those lie whole frames outside
    assert bool(((frac >= 0.1) & (frac <= 0.9))[near].all()), (float(frac.min()), float(frac.max()))
    p64, p32 = wc.sample_positions(name), wc.sample_positions(name, torch.float32)
    for a64, a32, size in zip(p64, p32, (c["h"], c["w"])):
        assert torch.equal(torch.floor(a64), torch.floor(a32.double()))
        if size == 1:
            assert bool((a64 == 0).all()) and bool((a32 == 0).all())
        else:
            fr = (a64 - torch.floor(a64))[(a64 > -size) & (a64 < 2 * size)]
            assert bool(((fr > 0.09) & (fr < 0.91)).all())


def test_case_shapes_are_what_they_claim():
    c = wc.CASES
    assert c["odd"]["c"] % 4 == 1 and c["c32"]["c"] == 32 and c["wide"]["w"] > 64 and c["wide"]["h"] == 6 * 4
    assert (c["line"]["h"], c["column"]["w"]) == (1, 1)
    for name, share in wc.OUTSIDE_SHARE.items():
        iy, ix = wc.sample_positions(name)
        outside = (ix < 0) | (ix > c[name]["w"] - 1) | (iy < 0) | (iy > c[name]["h"] - 1)
        assert abs(float(outside.double().mean()) - share) < 0.002, (name, float(outside.double().mean()))
    # motion: shifts beyond the frame and beyond any window of the kernel (tile + 8 px)
    assert c["motion"]["shift"] > max(c["motion"]["h"], c["motion"]["w"]) and c["wide"]["shift"] > 8
    # integer: H - 1 and W - 1 are powers of two, image 0 has no flow, image 1 integers that reach the frame's edges
    h, w = c["integer"]["h"], c["integer"]["w"]
    assert (h - 1) & (h - 2) == 0 and (w - 1) & (w - 2) == 0
    f = wc.leaves("integer")["flow"]
    assert float(f[0].abs().max()) == 0 and float(f[1].abs().max()) == c["integer"]["shift"] and bool((f == torch.round(f)).all())
    iy, ix = wc.sample_positions("integer")
    assert bool((ix == torch.round(ix)).all()) and bool((iy == torch.round(iy)).all())
    assert bool((wc.sample_positions("integer", torch.float32)[1].double() == ix).all())
    assert int(((ix[1] == 0) | (ix[1] == w - 1) | (iy[1] == 0) | (iy[1] == h - 1)).sum()) >= 8
    # edges: samples in (-1, 0) and (size - 1, size) on each axis
    iy, ix = wc.sample_positions("edges")
    h, w = c["edges"]["h"], c["edges"]["w"]
    for p, size in ((iy, h), (ix, w)):
        assert int(((p > -1) & (p < 0)).sum()) >= 3 and int(((p > size - 1) & (p < size)).sum()) >= 3
    assert int(((iy > -1) & (iy < 0) & (ix > -1) & (ix < 0)).sum()) >= 1   # over a corner of the frame: one corner valid
    # nonfinite: a dozen touched pixels, every kind of value
    vals = [v for *_, v in wc.NONFINITE]
    assert int(wc.touched().sum()) >= 12 and any(v != v for v in vals)
    assert {float("inf"), float("-inf"), 1e30, -1e30} <= set(vals)
    ref = wc.reference_flow("nonfinite")
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) == 4.0 * 17


@pytest.mark.parametrize("mode", wc.MODES)
def test_reference_gradients_of_the_special_cases(mode):
    """image 0 of "integer": grad_x is grad_out; the unit axes carry no flow gradient; the touched pixels of "nonfinite" have none
    (zeros mode: on both axes; border mode: on the touched axis -- the other axis still moves the clamped sample)."""
    ref = wc.reference("integer", mode)
    assert torch.equal(ref["x"][0], wc.leaves("integer")["grad_out"][0].double())
    assert float(wc.reference("line", mode)["flow"][..., 1].abs().max()) == 0 and float(wc.reference("line", mode)["flow"][..., 0].abs().max()) > 0
    assert float(wc.reference("column", mode)["flow"][..., 0].abs().max()) == 0
    g = wc.reference("nonfinite", mode)["flow"][0]
    for y, x, k, _ in wc.NONFINITE:
        assert float(g[y, x, k]) == 0
    if mode == "zeros":
        assert float(g[wc.touched()].abs().max()) == 0


@pytest.mark.parametrize("name", list(wc.CASES))
def test_oracle_satisfies_the_adjoint_identity(name):
    """<grad_x, x> = <grad_out, flow_warp(x)>: the warp is linear in x.  Float64 sums of n*c*h*w <= 23040 terms of order 1: 1e-12 of
    sum|terms| is a thousand times the rounding of either side."""
    for mode in wc.MODES:
        L = wc.leaves(name)
        gx, out = wc.reference(name, mode)["x"], wc.reference_out(name, mode)
        lhs, rhs = float((gx * L["x"].double()).sum()), float((L["grad_out"].double() * out).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((L["grad_out"].double() * out).abs().sum()), (mode, lhs, rhs)


def test_shared_cases_meet_their_conditions():
    for name, c in wc.SHARED_CASES.items():
        L = wc.shared_leaves(name)
        assert tuple(L["offset"].shape) == (c["n"], 2, c["h"], c["w"]) and tuple(L["mask"].shape) == (c["n"], 1, c["h"], c["w"])
        assert tuple(L["weight"].shape) == (4, 4, 3, 3)
        py, px = wc.shared_sample_positions(name)
        for p in (py, px):
            f = p - torch.floor(p)
            if c["kind"] == "integer":
                assert bool((f == 0).all())
            else:
                assert bool(((f >= 0.1) & (f <= 0.9)).all())
    assert wc.shared_leaves("shared") is wc.dc.leaves("shared") and wc.shared_reference("shared") is wc.dc.reference("shared")
    c = wc.SHARED_CASES["shared_motion"]
    h, w = c["h"], c["w"]
    assert c["shift"] == 15 and w > 64
    py, px = wc.shared_sample_positions("shared_motion")
    inside = (py > -1) & (py < h) & (px > -1) & (px < w)
    straddle = inside & (((py < 0) | (py > h - 1)) ^ ((px < 0) | (px > w - 1)))
    assert int(straddle.sum()) >= 4 and float((~inside).double().mean()) > 0.5
    off = wc.shared_leaves("shared_integer")["offset"]
    assert float(off[0].abs().max()) == 0 and float(off[1].abs().max()) == 3


def test_alignment_graph_on_the_cpu():
    """The graph of the GPU test: the flow's fractions lie in [0.1, 0.9], offset + flow stays a tenth of a pixel from any integer (so
    float32 picks float64's cells in the warp and in the DCN), one SGD step on the heads lowers the float64 loss, every leaf gets a
    gradient, and GRAPH_E32 is the measured fp32 error."""
    P = wc.graph_params()
    cur, _ = wc.graph_data()
    f = P["flow"].detach()
    frac = f - torch.floor(f)
    assert bool(((frac >= 0.1) & (frac <= 0.9)).all())
    with torch.no_grad():
        offset, mask = wc.graph_offsets(P, cur)
    d = offset - torch.floor(offset)
    assert tuple(offset.shape) == (1, 2, 12, 16) and tuple(mask.shape) == (1, 1, 12, 16)
    assert float(torch.minimum(d, 1 - d).min()) >= 0.1   # where gradients are taken; the loss after the step is continuous in the offsets
    loss, grads, loss2 = wc.graph_reference()
    assert loss2 < loss and all(float(g.abs().max()) > 0 for g in grads.values())
    got = wc.measure_graph_e32()
    for k, e in wc.GRAPH_E32.items():
        assert wc.GRAPH_TOL[k] == 8.0 * max(e, 2.0 ** -23)
        assert e / 2 <= got[k] <= e * 2, (k, got[k], e)


# ---------------------------------------------------------------- the library, without a GPU
NEW_SYMBOLS = {
    "crfp_flow_warp_backward_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "crfp_flow_warp_backward_f32": (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "crfp_dcnv2_shared_backward_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "crfp_dcnv2_shared_backward_f32": (ctypes.c_int, [ctypes.c_void_p] * 10 + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
}


def test_new_symbols_are_exported_with_the_headers_signatures(lib):
    """The four new entry points: exported by the built library, bound in _lib with the argument lists of include/crfp_hip.h (whose
    prototypes are parsed here: pointers -> c_void_p, int, size_t)."""
    import re
    from crfp_amd import _lib
    raw = ctypes.CDLL(os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so"))
    header = open(os.path.join(ROOT, "include", "crfp_hip.h")).read()
    for name, (res, args) in NEW_SYMBOLS.items():
        assert hasattr(raw, name), name
        assert _lib.SIGNATURES[name] == (res, args), name
        m = re.search(r"(size_t|int)\s+" + name + r"\(([^)]*)\);", header)
        assert m, name
        assert {"size_t": ctypes.c_size_t, "int": ctypes.c_int}[m.group(1)] is res
        parsed = [ctypes.c_void_p if "*" in a else ctypes.c_size_t if a.split()[0] == "size_t" else ctypes.c_int
                  for a in (re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(2).split(","))]
        assert parsed == args, (name, parsed)


def test_size_queries(lib):
    for c in wc.CASES.values():
        assert lib.crfp_flow_warp_backward_workspace_bytes(c["n"], c["c"], c["h"], c["w"]) > 0
    assert lib.crfp_flow_warp_backward_workspace_bytes(1, 32, 360, 640) > 0 and lib.crfp_flow_warp_backward_workspace_bytes(1, 4, 1440, 2560) > 0
    for bad in ((0, 4, 9, 11), (1, 0, 9, 11), (1, 4, 0, 11), (1, 4, 9, 0), (70000, 4, 9, 11), (1, 4, 300000, 11), (1, 4, 9, (1 << 30) + 1),
                (65535, 1 << 20, 262140, 1 << 30)):
        assert lib.crfp_flow_warp_backward_workspace_bytes(*bad) == 0, bad
    for c in wc.SHARED_CASES.values():
        assert lib.crfp_dcnv2_shared_backward_workspace_bytes(c["n"], 4, c["h"], c["w"]) > 0
    # the compact route's scratch holds no tiled tensor: it does not grow with the frame beyond the per-workgroup weight slabs
    assert lib.crfp_dcnv2_shared_backward_workspace_bytes(1, 4, 1440, 2560) == lib.crfp_dcnv2_backward_workspace_bytes(1, 4, 4, 1440, 2560, 3, 1)
    assert lib.crfp_dcnv2_shared_backward_workspace_bytes(1, 4, 1440, 2560) < 1 << 20
    for bad in ((1, 8, 24, 40), (1, 3, 24, 40), (0, 4, 24, 40), (1, 4, 0, 40), (1, 4, 24, 0), (70000, 4, 24, 40), (1, 4, 300000, 40)):
        assert lib.crfp_dcnv2_shared_backward_workspace_bytes(*bad) == 0, bad


def test_argument_errors_come_before_any_hip_call(lib):
    """Every refusal is a negative CRFP_E_* code (a HIP call on a machine without a GPU would give a positive hipError_t or crash on the
    never-dereferenced pointers)."""
    p = ctypes.c_void_p(16)
    need = lib.crfp_flow_warp_backward_workspace_bytes(2, 5, 9, 11)

    def warp(x=p, flow=p, go=p, gx=p, gflow=p, n=2, c=5, h=9, w=11, mode=0, ws=p, nb=need):
        return lib.crfp_flow_warp_backward_f32(x, flow, go, gx, gflow, n, c, h, w, mode, ws, nb, None)

    assert warp(gx=None, gflow=None) == BADARG and b"nothing to do" in lib.crfp_last_error_string()
    assert warp(x=None) == BADARG and b"grad_flow" in lib.crfp_last_error_string()
    assert warp(flow=None) == BADARG and warp(go=None) == BADARG and b"null" in lib.crfp_last_error_string()
    assert warp(n=0) == BADARG and warp(c=0) == BADARG and warp(h=0) == BADARG and warp(w=0) == BADARG
    assert warp(mode=2) == UNSUPPORTED and b"padding_mode" in lib.crfp_last_error_string()
    assert warp(mode=-1) == UNSUPPORTED
    assert warp(n=70000, nb=1 << 40) == UNSUPPORTED and b"65535 images" in lib.crfp_last_error_string() and b"2^58" in lib.crfp_last_error_string()
    assert warp(h=300000, nb=1 << 40) == UNSUPPORTED
    assert warp(nb=need - 1) == WORKSPACE and warp(ws=None) == WORKSPACE and b"workspace" in lib.crfp_last_error_string()
    assert lib.crfp_flow_warp_backward_window_f32(p, p, p, p, p, 2, 5, 9, 11, 0, 2, p, need, None) == BADARG

    need = lib.crfp_dcnv2_shared_backward_workspace_bytes(1, 4, 24, 40)

    def shared(ins=(p,) * 5, outs=(p,) * 5, n=1, cin=4, cout=4, h=24, w=40, ws=p, nb=need):
        return lib.crfp_dcnv2_shared_backward_f32(*ins, *outs, n, cin, cout, h, w, ws, nb, None)

    for i in range(5):
        assert shared(ins=tuple(None if j == i else p for j in range(5))) == BADARG and b"null" in lib.crfp_last_error_string()
    assert shared(outs=(None,) * 5) == BADARG and b"nothing to do" in lib.crfp_last_error_string()
    assert shared(n=0) == BADARG and shared(h=0) == BADARG
    assert shared(cin=8, nb=1 << 40) == UNSUPPORTED and b"4 -> 4" in lib.crfp_last_error_string()
    assert shared(cout=3, nb=1 << 40) == UNSUPPORTED
    assert shared(n=70000, nb=1 << 40) == UNSUPPORTED and b"65535 images" in lib.crfp_last_error_string()
    assert shared(nb=need - 1) == WORKSPACE and shared(ws=None) == WORKSPACE
