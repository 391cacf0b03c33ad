"""CPU: the reference, the inputs and the host side of the conv probe tests (tests/conv_cases.py, tests/test_gpu_conv_probe.py).

The float64 reference is held to F.conv2d compositions; the exact-input method is replayed in numpy for both split-operand forms; every
case the GPU tests use is checked against the condition (sum |x| |w| + |b| <= 2^11) under which a correct kernel is exact; and the kernel
variant each GPU case means to test is asked of the launcher's own selection rule, which is host code."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "crfp_amd", "libcrfp_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "crfp_amd", "csrc"), "-j8"])
    from crfp_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------- the reference against F.conv2d compositions
def _compose(conv, inp):
    parts = []
    for s, t in zip(conv.srcs, inp["srcs"]):
        t = t.double()
        parts.append(F.pixel_unshuffle(t, 4) if s[0] == "unshuf4" else t.permute(0, 3, 1, 2) if s[0] == "flow2" else t)
    w, b = inp["weight"].double(), inp["bias"].double()
    if conv.cout_split:
        w, b = torch.cat([w, inp["weight2"].double()]), torch.cat([b, inp["bias2"].double()])
    v = F.conv2d(torch.cat(parts, 1), w, b, padding=1)
    if conv.store == "offmask":
        noff = 4 * conv.n_off_quads
        o = 10 * torch.tanh(v[:, :noff]) + inp["flow"].double().flip(-1).permute(0, 3, 1, 2).repeat(1, noff // 2, 1, 1)   # model/CRFP.py:338
        return [torch.cat([o, torch.sigmoid(v[:, noff:])], 1)]
    v = {"none": v, "relu": F.relu(v), "lrelu": F.leaky_relu(v, 0.1)}[conv.act] * conv.post_scale
    if conv.residual:
        v = v + inp["residual"].double()
    if conv.store == "ps":
        return [F.pixel_shuffle(v, conv.ps_r)]
    if conv.dsts is None:
        return [v]
    return [v[:, 4 * d[0]:min(4 * d[1], conv.cout)] for d in conv.dsts]


@pytest.mark.parametrize("name", ["block0", "unshuf4", "ps2", "ps4", "three_dsts", "residual", "cout30"])
def test_reference_equals_conv2d_composition_on_exact_inputs(name):
    case, inp, ref = cc.exact_case(name, "fine_x")
    want = _compose(case.conv, inp)
    assert len(want) == len(ref["out"])
    for a, b in zip(ref["out"], want):
        assert a.shape == b.shape and torch.equal(a, b)   # every sum is exact in float64: any order gives the same bits


@pytest.mark.parametrize("case", cc.NORMAL, ids=lambda c: c.name)
def test_reference_equals_conv2d_composition_on_ordinary_data(case):
    inp = cc.make_inputs(case.conv, case.n, case.h, case.w, "normal", seed=5)
    ref = cc.reference(case.conv, inp)
    for a, b in zip(ref["out"], _compose(case.conv, inp)):
        assert a.shape == b.shape and float((a - b).abs().max()) < 1e-12
    x = cc.concat_sources(case.conv, inp["srcs"])
    w, b = inp["weight"], inp["bias"]
    if case.conv.cout_split:
        w, b = torch.cat([w, inp["weight2"]]), torch.cat([b, inp["bias2"]])
    S = F.conv2d(x.abs(), w.double().abs(), b.double().abs(), padding=1)
    assert float((ref["S"] - S).abs().max()) < 1e-9


def test_rne_bf16_rounds_to_nearest_even():
    t = torch.tensor([1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -7, 65503.0, -0.3])
    got = cc.rne_bf16(t)
    assert got.tolist()[:5] == [1.0, 1.0, 1.0 + 2 ** -6, 1.0 + 2 ** -7, 65536.0]    # ties to even, both ways
    assert abs(got[5].item() + 0.3) <= 2 ** -10          # half an ulp of [1/4, 1/2)


# ---------------------------------------------------------------- the exact-input method
def _f16(v):
    return v.astype(np.float16).astype(np.float64)


def _emulate(x, w, order):
    """fp32 accumulation, in `order`, of the products the two f16x3 forms feed their MFMAs -> (two-accumulator result, single-accumulator
    result), as the kernels compute them (conv3x3_split_body: hi + lo / 2^11; conv3x3_split8_kernel: acc * 2^-11)."""
    f32 = np.float32
    x0 = _f16(x); x1s = _f16((x - x0) * 2048)
    w0 = _f16(w); w1s = _f16((w - w0) * 2048)
    A = _f16(w * 2048); B = _f16((w - A / 2048) * 2048); Cw = _f16(w)
    hi = lo = acc = f32(0)
    for i in order:
        hi = f32(hi + f32(x0[i] * w0[i]))
        lo = f32(lo + f32(x0[i] * w1s[i]))
        lo = f32(lo + f32(x1s[i] * w0[i]))
        for t in (x0[i] * A[i], x0[i] * B[i], x1s[i] * Cw[i]):
            acc = f32(acc + f32(t))
    return float(f32(hi + f32(lo / f32(2048)))), float(f32(acc * f32(2.0 ** -11)))


@pytest.mark.parametrize("nterms", [27, 288, 2880])
@pytest.mark.parametrize("which", ["fine_x", "fine_w"])
def test_exact_inputs_survive_both_split_forms_in_any_order(nterms, which):
    rs = np.random.RandomState(nterms)
    for _ in range(12 if nterms > 1000 else 40):
        a, b = cc.fine(rs, nterms), cc.coarse(rs, nterms)
        x, w = (a, b) if which == "fine_x" else (b, a)
        x, w = x.astype(np.float32).astype(np.float64), w.astype(np.float32).astype(np.float64)
        assert np.abs(x * w).sum() <= cc.SIGMA_MAX
        exact = float(np.dot(x, w))
        assert _emulate(x, w, rs.permutation(nterms)) == (exact, exact)


def test_a_dropped_product_breaks_exactness():
    """The other way round: without the x1s * w0 term (a mis-built split) fine x no longer comes back exactly -- the method can see it."""
    rs = np.random.RandomState(1)
    x, w = cc.fine(rs, 288), cc.coarse(rs, 288)
    x0 = _f16(x)
    assert float(np.dot(x0, w)) != float(np.dot(x, w))


def test_coarse_values_are_bf16_values_and_fine_values_split_cleanly():
    rs = np.random.RandomState(2)
    c, f = torch.from_numpy(cc.coarse(rs, 4096)), torch.from_numpy(cc.fine(rs, 4096))
    assert torch.equal(cc.rne_bf16(c), c) and torch.equal(c.float().double(), c) and torch.equal(f.float().double(), f)
    f0 = _f16(f.numpy())
    tail = (f.numpy() - f0) * 2048
    assert np.array_equal(_f16(tail), tail) and np.array_equal(f0 + tail / 2048, f.numpy())   # head + scaled tail hold all of it
    q = torch.from_numpy(cc.quarters(rs, 4096))
    assert torch.equal(cc.rne_bf16(q), q)


# ---------------------------------------------------------------- the condition on the inputs, for every case of the GPU tests
@pytest.mark.parametrize("case", cc.EXACT + (cc.EDGE_1,), ids=lambda c: c.name)
@pytest.mark.parametrize("which", ["fine_x", "fine_w", "coarse"])
def test_exact_cases_stay_inside_the_sigma_bound(case, which):
    case, inp, ref = cc.exact_case(case.name, which)
    assert cc.sigma_bound_ok(case.conv, ref), float(ref["S"].max())
    for t in ref["out"]:
        assert torch.equal(t.float().double(), t)                       # the expected output is an fp32 value
    assert all(len(t.unique()) > 3 for t in ref["out"])                 # and not a trivial one
    if case.conv.dst_f32:                                               # a float destination must be told from a bf16 one
        assert not torch.equal(cc.rne_bf16(ref["out"][0]), ref["out"][0])


def test_multi_launch_cases_stay_inside_the_sigma_bound():
    for name, *_ in cc.DUAL:
        for which in ("fine_x", "fine_w", "coarse"):
            _, _, _, _, refs = cc.dual_case(name, which)
            assert cc.sigma_bound_ok(cc.DUAL_A, refs[0]) and cc.sigma_bound_ok(cc.DUAL_B, refs[1])
    for which in ("fine_x", "fine_w"):
        _, _, ra, rb = cc.chain_case(which)
        assert cc.sigma_bound_ok(cc.CHAIN_A, ra)
        # conv b reads conv a's exact output: multiples of 2^-13 with a nonzero fp16 tail (that is the point: the tail planes of the S3 image
        # carry something), times coarse weights: products are multiples of 2^-14, so conv b is exact while its S <= 2^10
        mid = ra["full"]
        assert torch.equal(mid * 2 ** 13, (mid * 2 ** 13).round()) and float(mid.abs().max()) < 2 ** 11
        assert (mid.numpy() != mid.numpy().astype(np.float16).astype(np.float64)).mean() > 0.2
        assert float(rb["S"].max()) <= 2 ** 10
        assert torch.equal(rb["full"].float().double(), rb["full"])
    for (h, w) in cc.PAIR_GEOMETRY:
        for resid in (0, 1):
            conv_b, _, _, mid, ra, rb = cc.pair_case(h, w, resid)
            assert cc.sigma_bound_ok(cc.PAIR_A, ra)
            # stage b: bf16 values (multiples of 1/8) times multiples of 1/2, sums far below 2^24 / 16
            assert torch.equal(mid * 8, (mid * 8).round()) and float(rb["S"].max()) * 16 < 2 ** 24
            assert float(mid.abs().max()) > 4   # the middle tensor is really rounded somewhere
    assert any(not torch.equal(cc.pair_case(h, w, 0)[3], cc.pair_case(h, w, 0)[4]["full"]) for h, w in cc.PAIR_GEOMETRY)


# ---------------------------------------------------------------- the launcher's selection rule, asked on the host
def _desc(conv, own_sources=True):
    from crfp_amd import _lib
    d = _lib.ProbeConv()
    if own_sources:
        d.nsrc = len(conv.srcs)
        for i, s in enumerate(conv.srcs):
            d.src_kind[i], d.src_nch[i], d.src_pad[i] = _lib.PROBE_SRC[s[0]], s[1], s[2] if len(s) > 2 else 0
    d.cout, d.cout_split, d.store, d.ps_r = conv.cout, conv.cout_split, _lib.PROBE_STORE[conv.store], conv.ps_r
    d.act, d.post_scale, d.n_off_quads, d.strict, d.dst_f32 = {"none": 0, "relu": 1, "lrelu": 2}[conv.act], conv.post_scale, conv.n_off_quads, conv.strict, conv.dst_f32
    dsts = conv.dsts if conv.dsts is not None else ((0, (conv.cout + 3) // 4),)
    if conv.store == "ps":
        dsts = ((0, 0),)
    d.ndst = len(dsts)
    for i, t in enumerate(dsts):
        d.dst_q0[i], d.dst_q1[i], d.dst_pad[i] = t[0], t[1], t[2] if len(t) > 2 else 0
    return d


def _kernels(lib, storage, mode, a, b, n, h, w):
    from crfp_amd import _lib
    k = (ctypes.c_int * 2)()
    fn = getattr(lib, "crfp_conv_probe_kernel" + ("_bf16" if storage == "bf16" else ""))
    rc = fn(_lib.PROBE_MODES[mode], ctypes.byref(a), ctypes.byref(b) if b is not None else None, n, h, w, k)
    assert rc == 0, lib.crfp_last_error_string()
    return tuple(_lib.CONV_KERNELS[i] for i in k)


@pytest.mark.parametrize("case", cc.EXACT + cc.NORMAL + (cc.EDGE_513, cc.EDGE_1), ids=lambda c: c.name)
def test_every_gpu_case_reaches_the_kernel_it_names(lib, case):
    for i, storage in enumerate(("f32", "bf16")):
        assert _kernels(lib, storage, "single", _desc(case.conv), None, case.n, case.h, case.w) == (case.kernel[i], "none"), storage


def test_dispatch_edges_of_the_multi_launch_modes(lib):
    for name, n, h, w, k32, k16 in cc.DUAL:
        assert _kernels(lib, "f32", "dual", _desc(cc.DUAL_A), _desc(cc.DUAL_B), n, h, w) == k32, name
        assert _kernels(lib, "bf16", "dual", _desc(cc.DUAL_A), _desc(cc.DUAL_B), n, h, w) == k16, name
    for h, w in cc.PAIR_GEOMETRY:
        assert _kernels(lib, "bf16", "pair", _desc(cc.PAIR_A), _desc(cc.PAIR_B, False), 2, h, w) == ("bf16_pair", "bf16_pair")
    assert _kernels(lib, "f32", "s3_chain", _desc(cc.CHAIN_A), _desc(cc.CHAIN_B, False), 2, 9, 70) == ("split8", "split4")
    # the 512-slot rule of the bf16 build's 8-wave kernel, on both sides: 19 * 27 = 513 tiles and 512 = 16 * 32
    q = _desc(cc.EDGE_513.conv)
    assert _kernels(lib, "bf16", "single", q, None, 16, 64, 256) == ("bf16_x8", "none")
    assert _kernels(lib, "bf16", "single", q, None, 19, 72, 192) == ("bf16_4w", "none")


def test_probe_refuses_what_it_cannot_run(lib):
    from crfp_amd import _lib
    a, b = _desc(cc.PAIR_A), _desc(cc.PAIR_B, False)
    k = (ctypes.c_int * 2)()
    ws = lib.crfp_conv_probe_workspace_bytes
    assert lib.crfp_conv_probe_kernel(_lib.PROBE_MODES["pair"], ctypes.byref(a), ctypes.byref(b), 2, 8, 62, k) == -3      # fp32 build: no pair kernel
    assert b"bf16 build only" in lib.crfp_last_error_string()
    assert lib.crfp_conv_probe_kernel_bf16(_lib.PROBE_MODES["s3_chain"], ctypes.byref(a), ctypes.byref(b), 2, 8, 62, k) == -3
    assert ws(0, ctypes.byref(a), None, 2, 8, 62) == 0 and b"destinations" in lib.crfp_last_error_string()               # conv a alone needs one
    q = _desc(cc.EXACT[1].conv)
    assert ws(0, ctypes.byref(q), None, 3, 3, 63) > 0 and lib.crfp_conv_probe_workspace_bytes_bf16(0, ctypes.byref(q), None, 3, 3, 63) > 0
    assert ws(0, ctypes.byref(q), None, 3, 3, 63) > lib.crfp_conv_probe_workspace_bytes_bf16(0, ctypes.byref(q), None, 3, 3, 63)
    assert ws(7, ctypes.byref(q), None, 3, 3, 63) == 0 and ws(0, None, None, 3, 3, 63) == 0 and ws(1, ctypes.byref(q), None, 3, 3, 63) == 0
    assert ws(0, ctypes.byref(q), None, 0, 3, 63) == 0 and ws(0, ctypes.byref(q), None, 3, 3, -1) == 0
    for field, bad in (("nsrc", 5), ("cout", 0), ("act", 9), ("store", 2), ("ndst", 4), ("cout_split", 32)):
        d = _desc(cc.EXACT[1].conv)
        setattr(d, field, bad)
        assert ws(0, ctypes.byref(d), None, 3, 3, 63) == 0, field
    d = _desc(cc.EXACT[1].conv); d.dst_q1[0] = 9
    assert ws(0, ctypes.byref(d), None, 3, 3, 63) == 0
    d = _desc(cc.EXACT[1].conv); d.src_kind[0] = 2; d.src_nch[0] = 24      # pixel_unshuffle(4) of 24 channels
    assert ws(0, ctypes.byref(d), None, 3, 3, 63) == 0
    d = _desc(dataclasses.replace(cc.EXACT[13].conv, ps_r=3))
    assert ws(0, ctypes.byref(d), None, 3, 3, 63) == 0
    # the call itself: null tensors and a short workspace are refused before anything is enqueued
    p16 = ctypes.c_void_p(16)
    assert lib.crfp_conv_probe(0, ctypes.byref(q), None, 3, 3, 63, p16, k, p16, 1 << 40, None) == -1 and b"null" in lib.crfp_last_error_string()
    for f in ("weight", "bias"):
        setattr(q, f, 16)
    q.src[0] = 16
    q.dst[0] = 16
    assert lib.crfp_conv_probe(0, ctypes.byref(q), None, 3, 3, 63, p16, k, p16, 1024, None) == -2
    assert lib.crfp_conv_probe(0, ctypes.byref(q), None, 3, 3, 63, None, k, p16, 1 << 40, None) == -1
