"""CPU: pins the cases of tests/dcn_backward_cases.py (their float64 reference, the condition their offsets are built to meet, the written-down
fp32 error the GPU tolerance comes from) and the host side of the new C-ABI entry points (symbols, sizes, argument errors) -- no GPU here."""
import ctypes
import os
import subprocess

import pytest
import torch

import dcn_backward_cases as dc
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


def test_oracle_gradients_agree_with_central_differences():
    """Case 1, L = sum(out * grad_out) in float64.  L is linear in x, mask, weight and bias and, inside a bilinear cell, linear in each
    offset, so a central difference has no truncation error; only the rounding of the two values of L remains.  L sums n*cout*h*w = 1188
    outputs of 72 products each, terms of order 1: sum|terms| < 1e6, so each L is good to 1e6 * 2^-53 = 1e-10 and the quotient, with
    step 1e-3 (every offset stays inside its cell: the fractions are in [0.1, 0.9]), to 1e-10 / 1e-3 = 1e-7 at the very worst; random
    rounding gives about 1e-10.  Bound: 1e-8 absolute, on gradients of order 1."""
    name, step = "odd", 1e-3
    L = dc.leaves(name)
    ref = dc.reference(name)
    base = {k: L[k].double() for k in dc.GRADS}
    go = L["grad_out"].double()
    dg = dc.CASES[name]["dg"]
    with torch.no_grad():
        def loss(t):
            return float((dc.oracle_fn(t["x"], t["offset"], t["mask"], t["weight"], t["bias"], dg) * go).sum())
        g = torch.Generator().manual_seed(5)
        for k in dc.GRADS:
            for i in torch.randperm(base[k].numel(), generator=g)[:12].tolist():
                vals = []
                for sgn in (1.0, -1.0):
                    t = dict(base)
                    t[k] = base[k].clone()
                    t[k].view(-1)[i] += sgn * step
                    vals.append(loss(t))
                fd = (vals[0] - vals[1]) / (2 * step)
                assert abs(fd - float(ref[k].view(-1)[i])) <= 1e-8, (k, i, fd, float(ref[k].view(-1)[i]))


@pytest.mark.parametrize("name", list(dc.CASES))
def test_every_sample_position_is_away_from_a_cell_boundary(name):
    """The condition the offsets are built to meet (a condition, not a tolerance): fractional parts in [0.1, 0.9] on both axes -- or, in
    the integer case, exactly integer positions."""
    py, px = dc.sample_positions(name)
    for p in (py, px):
        f = p - torch.floor(p)
        if dc.CASES[name]["kind"] == "integer":
            assert bool((f == 0).all())
        else:
            assert bool(((f >= 0.1) & (f <= 0.9)).all()), (float(f.min()), float(f.max()))


def test_case_shapes_are_what_they_claim():
    c = dc.CASES
    assert (c["odd"]["h"] % 4, c["odd"]["w"] % 64, c["odd"]["n"]) == (1, 11, 2)
    assert (c["g8"]["cin"], c["g8"]["cout"], c["g8"]["dg"]) == (32, 32, 8) and (c["shared"]["cin"], c["shared"]["dg"]) == (4, 1)
    assert dc.leaves("shared")["offset"].shape[1] == 2 and dc.leaves("shared")["mask"].shape[1] == 1
    # large motion: shifts up to +-(max(h, w) + 4); most samples fall outside, some straddle an edge with one corner row inside
    h, w = c["motion"]["h"], c["motion"]["w"]
    assert c["motion"]["shift"] == max(h, w) + 4
    py, px = dc.sample_positions("motion")
    inside = (py > -1) & (py < h) & (px > -1) & (px < w)
    assert 0.5 < float((~inside).float().mean()) < 0.95
    straddle = inside & (((py < 0) | (py > h - 1)) ^ ((px < 0) | (px > w - 1)))
    assert int(straddle.sum()) >= 4
    off = dc.leaves("integer")["offset"]
    assert float(off[0].abs().max()) == 0 and float(off[1].abs().max()) == c["integer"]["shift"]


def test_dropped_samples_have_zero_gradient_in_the_reference():
    h, w = dc.CASES["motion"]["h"], dc.CASES["motion"]["w"]
    py, px = dc.sample_positions("motion")
    dropped = ~((py > -1) & (py < h) & (px > -1) & (px < w))     # [n, dg, 9, h, w]
    ref = dc.reference("motion")
    n, dg = dropped.shape[:2]
    assert float(ref["mask"].reshape(n, dg, 9, h, w)[dropped].abs().max()) == 0.0
    assert float(ref["offset"].reshape(n, dg, 9, 2, h, w).permute(0, 1, 2, 4, 5, 3)[dropped].abs().max()) == 0.0


def test_identity_case_is_half_the_warp_on_the_cpu():
    """Case 6: the oracle's float64 gradients of the identity-initialised DCN against those of 0.5 * grid_sample(align_corners=True, zeros)."""
    ref = dc.reference("identity")
    gx, gflow = dc.identity_reference()
    assert float((ref["x"] - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    assert float((ref["offset"] - gflow).abs().max()) <= 1e-12 * float(gflow.abs().max())
    assert float(gflow.abs().max()) > 0.1


@pytest.mark.parametrize("name", list(dc.CASES))
def test_written_down_fp32_error_is_the_measured_one(name):
    """TOL = 8 * E32 and E32 is what measure_e32 gives here, up to the scatter of a maximum over rounding errors under another
    summation order of the CPU kernels (a factor 3 either way)."""
    got = dc.measure_e32(name)
    for k in dc.GRADS:
        assert dc.TOL[name][k] == 8.0 * dc.E32[name][k]
        assert dc.E32[name][k] / 3 <= got[k] <= dc.E32[name][k] * 3, (k, got[k], dc.E32[name][k])


def test_module_graph_on_the_cpu():
    """The module-level graph of the GPU test: its offsets stay away from cell boundaries (so float32 picks float64's cells), one SGD
    step lowers the float64 loss, and MODULE_E32 is the measured fp32 error of its parameter gradients."""
    P = dc.module_params()
    feat, x, target = dc.module_data()
    with torch.no_grad():
        offset, _ = dc.module_heads(P, feat)
    f = offset - torch.floor(offset)
    assert float(torch.minimum(f, 1 - f).min()) > 1e-4 and float(offset.abs().max()) > 3.0
    loss, grads, loss2 = dc.module_reference()
    assert loss2 < loss and all(float(g.abs().max()) > 0 for g in grads.values())
    got = dc.measure_module_e32()
    for k in P:
        assert dc.MODULE_TOL[k] == 8.0 * dc.MODULE_E32[k]
        assert dc.MODULE_E32[k] / 3 <= got[k] <= dc.MODULE_E32[k] * 3, (k, got[k], dc.MODULE_E32[k])


# ---------------------------------------------------------------- the library, without a GPU
def test_backward_symbols_are_exported_and_bound(lib):
    from crfp_amd import _lib
    raw = ctypes.CDLL(os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so"))
    for n in ("crfp_dcnv2_backward_workspace_bytes", "crfp_dcnv2_backward_f32"):
        assert hasattr(raw, n) and n in _lib.SIGNATURES
    assert lib.crfp_dcnv2_backward_workspace_bytes.restype is ctypes.c_size_t
    assert len(lib.crfp_dcnv2_backward_f32.argtypes) == 22


def test_backward_size_query(lib):
    for name in ("odd", "g8", "shared"):
        c = dc.CASES[name]
        assert lib.crfp_dcnv2_backward_workspace_bytes(c["n"], c["cin"], c["cout"], c["h"], c["w"], 3, c["dg"]) > 0
    assert lib.crfp_dcnv2_backward_workspace_bytes(1, 32, 32, 360, 640, 3, 8) > 0 and lib.crfp_dcnv2_backward_workspace_bytes(1, 4, 4, 1440, 2560, 3, 1) > 0
    for bad in ((0, 8, 6, 9, 11, 3, 2), (2, 8, 6, 9, 11, 5, 2), (2, 8, 6, 9, 11, 3, 3), (2, 65, 6, 9, 11, 3, 1), (2, 8, 65, 9, 11, 3, 2)):
        assert lib.crfp_dcnv2_backward_workspace_bytes(*bad) == 0, bad


def test_backward_argument_errors_come_before_any_hip_call(lib):
    """Every refusal is a negative CRFP_E_* code (a HIP call on a machine without a GPU would give a positive hipError_t or crash on the
    never-dereferenced pointers)."""
    p = ctypes.c_void_p(16)
    need = lib.crfp_dcnv2_backward_workspace_bytes(2, 8, 6, 9, 11, 3, 2)

    def call(ins=(p,) * 5, outs=(p,) * 5, n=2, cin=8, cout=6, h=9, w=11, k=3, pad=1, dil=1, dg=2, ws=p, nb=need):
        return lib.crfp_dcnv2_backward_f32(*ins, *outs, n, cin, cout, h, w, k, pad, dil, dg, ws, nb, None)

    BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
    for i in range(5):   # a null input
        assert call(ins=tuple(None if j == i else p for j in range(5))) == BADARG
        assert b"null" in lib.crfp_last_error_string()
    assert call(outs=(None,) * 5) == BADARG and b"nothing to do" in lib.crfp_last_error_string()
    assert call(n=0) == BADARG and call(h=0) == BADARG and call(cout=0) == BADARG and call(dg=0) == BADARG
    assert call(k=5, pad=2) == UNSUPPORTED and b"kernel 3" in lib.crfp_last_error_string()
    assert call(pad=0) == UNSUPPORTED and call(dil=2) == UNSUPPORTED
    assert call(dg=3) == UNSUPPORTED and b"deformable_groups" in lib.crfp_last_error_string()
    assert call(cin=128, dg=1, nb=1 << 40) == UNSUPPORTED and call(cout=65, nb=1 << 40) == UNSUPPORTED    # beyond 64 channels: an error
    assert call(nb=need - 1) == WORKSPACE and call(ws=None) == WORKSPACE
    assert b"workspace" in lib.crfp_last_error_string()
