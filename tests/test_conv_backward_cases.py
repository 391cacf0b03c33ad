"""CPU: pins the cases of tests/conv_backward_cases.py (their shapes, the |z| condition of the relu / lrelu cases, the written-down fp32
errors the GPU tolerances come from, the reference taken from a given `out`, the module graphs) and the host side of the two new C-ABI
entry points -- no GPU here."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import conv_backward_cases as cc
from conftest import ROOT

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
ACT = {"none": 0, "relu": 1, "lrelu": 2, "tanh": 3, "sigmoid": 4}


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


def test_case_shapes_are_what_they_claim():
    c = cc.CASES
    assert set(c) == {"odd", "cat66", "tanh", "sigmoid", "resid", "shuffle2", "shuffle4", "unshuffle4", "wide", "slabs", "line", "column"}
    assert all(v % 2 for v in (c["odd"]["cin"], c["odd"]["cin2"], c["odd"]["cout"], c["odd"]["h"], c["odd"]["w"])) and c["odd"]["n"] == 2
    assert (c["cat66"]["cin"], c["cat66"]["cin2"], c["cat66"]["cout"]) == (32, 34, 32) and c["cat66"]["cin2"] % 4
    assert (c["tanh"]["act"], c["tanh"]["s"], c["tanh"]["cout"]) == ("tanh", 10.0, 18) and c["sigmoid"]["act"] == "sigmoid"
    assert c["resid"]["resid"] and c["resid"]["act"] == "none" and c["resid"]["s"] == 0.7
    assert c["shuffle2"]["shuffle"] == 2 and c["shuffle2"]["act"] == "relu" and c["shuffle4"]["shuffle"] == 4
    assert c["wide"]["w"] > 2 * 64 and c["wide"]["w"] % 64 and (c["line"]["h"], c["column"]["w"]) == (1, 1)
    assert c["slabs"]["n"] == 3 and c["slabs"]["n"] * c["slabs"]["h"] > 2 * 4   # more row tiles than four per slab: J > 1, several tiles each
    for name, k in c.items():
        L, r = cc.leaves(name), k.get("shuffle", 1)
        xs = (k["n"], k["cin"] // 16, 4 * k["h"], 4 * k["w"]) if k.get("unshuffle") else (k["n"], k["cin"], k["h"], k["w"])
        assert tuple(L["x"].shape) == xs and tuple(L["weight"].shape) == (k["cout"], k["cin"] + k["cin2"], 3, 3)
        assert (L["x2"] is None) == (k["cin2"] == 0) and (L["residual"] is None) == (not k.get("resid"))
        assert tuple(L["grad_out"].shape) == (k["n"], k["cout"] // (r * r), k["h"] * r, k["w"] * r) == tuple(cc.reference_out(name).shape)
        ref = cc.reference(name)
        assert tuple(ref) == cc.tensors(name) == tuple(cc.E32[name])
        assert all(ref[t].shape == L[t].shape and float(ref[t].abs().max()) > 0 for t in ref)
    assert tuple(cc.leaves("unshuffle4")["x"].shape) == (1, 2, 20, 28)
    assert cc.ONE_INPUT == ("tanh", "sigmoid", "slabs", "line", "column")
    # some of the tanh case's outputs are saturated in float32
    sat = cc.reference_out("tanh").float().abs() == 10.0
    assert 0.005 < float(sat.double().mean()) < 0.2
    assert torch.equal(cc.reference("resid")["residual"], cc.leaves("resid")["grad_out"].double())


@pytest.mark.parametrize("name", cc.SIGNED)
def test_preactivations_stay_away_from_zero(name):
    """A condition, not a tolerance: every float64 pre-activation of a relu / lrelu case has |z| >= 2e-4 max|z|."""
    assert cc.SIGNED == ("odd", "cat66", "shuffle2", "slabs")
    z = cc.preactivations(name)
    assert float(z.abs().min()) >= 2e-4 * float(z.abs().max()), (float(z.abs().min()), float(z.abs().max()))
    assert 0.2 < float((z > 0).double().mean()) < 0.8   # both branches taken


@pytest.mark.parametrize("name", list(cc.CASES))
def test_written_down_fp32_error_is_the_measured_one(name):
    """TOL = 8 * max(E32, one ulp), and E32 is what measure_e32 gives here within a factor 2."""
    got = cc.measure_e32(name)
    for k in cc.tensors(name):
        e = cc.E32[name][k]
        assert cc.TOL[name][k] == 8.0 * max(e, 2.0 ** -23)
        assert e / 2 <= got[k] <= e * 2, (k, got[k], e)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_reference_from_out_is_the_autograd_reference(name):
    """the activation's derivative taken from the float64 forward rounded to float32: the autograd gradients within 8 ulp"""
    ref = cc.reference(name)
    got = cc.reference_from_out(name, cc.reference_out(name).float())
    for k in cc.tensors(name):
        assert cc.rel_err(got[k], ref[k]) <= 8 * 2.0 ** -23, (k, cc.rel_err(got[k], ref[k]))


@pytest.mark.parametrize("name", list(cc.MODULES))
def test_module_graphs_on_the_cpu(name):
    """The graphs of the GPU test: every relu / lrelu pre-activation meets the |z| condition, the DCN's offsets stay a tenth of a pixel
    from any integer, every parameter and input gets a non-zero gradient, one SGD step lowers the float64 loss, and MODULE_E32 is the
    measured fp32 error."""
    rec = cc.module_records(name)
    signed = [z for layer, z in rec if layer != "offset"]
    assert len(signed) == (2 if name == "resblock" else 3)
    for z in signed:
        assert float(z.abs().min()) >= 2e-4 * float(z.abs().max())
    for layer, z in rec:
        if layer == "offset":
            d = z - torch.floor(z)
            assert float(torch.minimum(d, 1 - d).min()) >= 0.1
    assert (name == "resblock") == (not any(layer == "offset" for layer, _ in rec))
    P, I, _ = cc.module_leaves(name)
    assert set(I) == set(cc.MODULE_INPUTS[cc.MODULES[name]["kind"]])
    if name == "dcn4":
        assert tuple(I["pre_offset"].shape) == (1, 32, 2, 3)
    for layer in ("dcn_offset", "dcn_mask"):
        if layer + ".weight" in P:
            assert float(P[layer + ".weight"].abs().min()) > 0
    loss, grads, loss2, _ = cc.module_reference(name)
    assert loss2 < loss and set(grads) == set(P) | set(I) == set(cc.MODULE_E32[name])
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads.values())
    got = cc.measure_module_e32(name)
    for k, e in cc.MODULE_E32[name].items():
        assert e / 2 <= got[k] <= e * 2, (k, got[k], e)
        assert cc.module_tol(name, k) == 8.0 * max(e, cc.MODULE_EFWD[name], 2.0 ** -23)


def test_module_state_dicts_load_strictly():
    from crfp_amd.model import CRFP
    mods = {"dcn8": CRFP.DCN_module(8, dg=2, pre_offset=True, interpolate="none"),
            "dcn4": CRFP.DCN_module(4, 1, repeat=True, pre_offset=True, interpolate="pixelshuffle"),
            "resblock": CRFP.ResidualBlocksWithInputConv(16, 8, 1)}
    for name, m in mods.items():
        m.load_state_dict(cc.module_leaves(name)[0], strict=True)
        assert {k for k, _ in m.named_parameters()} == set(cc.module_leaves(name)[0])


# ---------------------------------------------------------------- the library, without a GPU
NEW_SYMBOLS = {
    "crfp_conv3x3_ex_backward_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 8),
    "crfp_conv3x3_ex_backward_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 7 +
                                     [ctypes.c_int] * 5 + [ctypes.c_float] + [ctypes.c_int] * 2 + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
}


def test_new_symbols_are_exported_with_the_headers_signatures(lib):
    """The two new entry points: exported by the built library, bound in _lib with the argument lists of include/crfp_hip.h (whose
    prototypes are parsed here: pointers -> c_void_p, int, float, size_t)."""
    from crfp_amd import _lib
    raw = ctypes.CDLL(os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so"))
    header = open(os.path.join(ROOT, "include", "crfp_hip.h")).read()
    scalar = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "float": ctypes.c_float}
    for name, (res, args) in NEW_SYMBOLS.items():
        assert hasattr(raw, name), name
        assert _lib.SIGNATURES[name] == (res, args), name
        m = re.search(r"(size_t|int)\s+" + name + r"\(([^)]*)\);", header)
        assert m, name
        assert scalar[m.group(1)] is res
        parsed = [ctypes.c_void_p if "*" in a else scalar[a.split()[0]] for a in (re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(2).split(","))]
        assert parsed == args, (name, parsed)


def _size(lib, c):
    return lib.crfp_conv3x3_ex_backward_workspace_bytes(c["n"], c["cin"], c["cin2"], c["cout"], c["h"], c["w"], c.get("unshuffle", 0), c.get("shuffle", 0))


def test_size_queries(lib):
    q = lib.crfp_conv3x3_ex_backward_workspace_bytes
    for c in cc.CASES.values():
        assert _size(lib, c) > 0
    assert q(1, 66, 0, 32, 360, 640, 0, 0) > 0 and q(1, 4, 4, 4, 1440, 2560, 0, 0) > 0
    assert q(1, 128, 32, 288, 45, 80, 0, 0) > 0   # the mid_channels = 64 module table's widest counts
    # gz is the only part that grows with the frame: one plane per output channel, and the slabs on top
    assert 4 * 4 * 1440 * 2560 <= q(1, 4, 4, 4, 1440, 2560, 0, 0) < 4 * 4 * 1440 * 2560 + (4 << 20)
    for bad in ((0, 5, 3, 7, 9, 11, 0, 0), (2, 0, 3, 7, 9, 11, 0, 0), (2, 5, -1, 7, 9, 11, 0, 0), (2, 5, 3, 0, 9, 11, 0, 0), (2, 5, 3, 7, 0, 11, 0, 0),
                (2, 5, 3, 7, 9, 0, 0, 0), (-1, 5, 3, 7, 9, 11, 0, 0), (2, 5, 3, 7, 9, -11, 0, 0),
                (2, 5, 3, 7, 9, 11, 2, 0), (2, 5, 3, 7, 9, 11, 0, 3), (2, 24, 0, 7, 9, 11, 4, 0), (2, 16, 16, 7, 9, 11, 4, 0), (2, 5, 3, 7, 9, 11, 0, 2),
                (2, 1000, 25, 7, 9, 11, 0, 0), (2, 5, 3, 1025, 9, 11, 0, 0), (2, 2 ** 31 - 1, 2 ** 31 - 1, 7, 9, 11, 0, 0),
                (70000, 5, 3, 7, 9, 11, 0, 0), (1, 5, 3, 7, 300000, 11, 0, 0), (1, 5, 3, 7, 9, (1 << 30) + 1, 0, 0),
                (65535, 1024, 0, 1024, 262140, 1 << 30, 0, 0)):
        assert q(*bad) == 0, bad


def test_argument_errors_come_before_any_hip_call(lib):
    """Every refusal is a negative CRFP_E_* code (a HIP call on a machine without a GPU would give a positive hipError_t or crash on the
    never-dereferenced pointers)."""
    p = ctypes.c_void_p(16)
    need = lib.crfp_conv3x3_ex_backward_workspace_bytes(2, 5, 3, 7, 9, 11, 0, 0)
    err = lib.crfp_last_error_string

    def conv(x=p, x2=p, weight=p, out=p, go=p, gx=p, gx2=p, gw=p, gb=p, n=2, cin=5, cin2=3, cout=7, h=9, w=11, act=2, s=0.5, ur=0, sr=0, ws=p, nb=need):
        return lib.crfp_conv3x3_ex_backward_f32(x, cin, x2, cin2, weight, out, go, gx, gx2, gw, gb, n, cout, h, w, act, s, ur, sr, ws, nb, None)

    assert conv(gx=None, gx2=None, gw=None, gb=None) == BADARG and b"nothing to do" in err()
    assert conv(go=None) == BADARG and b"null" in err()
    assert conv(out=None) == BADARG and b"out is required" in err()
    assert conv(x=None) == BADARG and conv(x2=None) == BADARG and b"grad_weight" in err()
    assert conv(weight=None) == BADARG and b"weight is required" in err()
    assert conv(cin=8, cin2=0, x2=None) == BADARG and b"grad_x2" in err()
    assert conv(n=0) == BADARG and conv(h=0) == BADARG and conv(w=-1) == BADARG
    # the forward's own combination rules
    assert conv(cin=0) == UNSUPPORTED and conv(cin2=-1) == UNSUPPORTED and conv(cout=0) == UNSUPPORTED
    assert conv(act=5) == UNSUPPORTED and b"activation" in err() and conv(act=-1) == UNSUPPORTED
    assert conv(ur=2) == UNSUPPORTED and conv(sr=3) == UNSUPPORTED
    assert conv(cin=16, cin2=16, ur=4) == UNSUPPORTED and conv(cin=24, cin2=0, gx2=None, ur=4) == UNSUPPORTED
    assert conv(cout=8, sr=2, act=3, s=1.0) == UNSUPPORTED and conv(cout=7, sr=2) == UNSUPPORTED and b"pixel_shuffle" in err()
    # the scale the derivative is taken with
    for act in (1, 2):
        assert conv(act=act, s=0.0) == UNSUPPORTED and conv(act=act, s=-1.0) == UNSUPPORTED and b"post_scale > 0" in err()
        assert conv(act=act, s=float("nan")) == UNSUPPORTED
    for act in (3, 4):
        assert conv(act=act, s=0.0) == UNSUPPORTED and b"post_scale != 0" in err() and conv(act=act, s=float("nan")) == UNSUPPORTED
    # sizes the index math cannot hold
    assert conv(n=70000, nb=1 << 40) == UNSUPPORTED and b"65535 images" in err() and b"2^58" in err()
    assert conv(h=300000, nb=1 << 40) == UNSUPPORTED and conv(w=(1 << 30) + 1, nb=1 << 40) == UNSUPPORTED
    assert conv(cout=1025, nb=1 << 40) == UNSUPPORTED and conv(cin=1000, cin2=25, nb=1 << 40) == UNSUPPORTED and b"1024" in err()
    assert conv(nb=need - 1) == WORKSPACE and conv(ws=None) == WORKSPACE and b"workspace" in err()
