"""GPU: the fp32 build's pair kernel (conv3x3_pair_kernel: conv a -> conv b in one launch, the tensor between them in LDS, one 16-channel
half at a time) against the two launches it replaces, bit for bit -- through the probe (crfp_conv_probe mode 4) on the two shapes the
engines fuse, and through the four engines with CRFP_CONV_PAIR=0 against =2.  Cases, inputs and the exactness argument:
tests/helpers/conv_pair_f32_cases.py."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

import conv_cases as cc
from helpers import conv_pair_f32_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GEOM_ID = lambda g: f"{g[0]}x{g[1]}"  # noqa: E731


def same_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements unwritten (the probe's NaN pre-fill) or not finite"
    if not torch.equal(got, want):
        bad = got != want
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, max |d| = {float((got - want).abs().max()):.3e}, "
                             f"first at {idx}: got {got[tuple(idx)].item()!r}, want {want[tuple(idx)].item()!r}")


def run_pair(conv_a, conv_b, ia, ib):
    from crfp_amd import ops
    r = ops.conv_probe(cc.probe_spec(conv_a, ia, DEV), cc.probe_spec(conv_b, ib, DEV), mode="pair_f32", storage="f32")
    assert r["kernel"] == ("split_pair", "split_pair")
    return r


def run_two_launches(conv_a, conv_b, ia, ib):
    """conv a alone (its output stored as fp32 Q4), then conv b alone on that tensor -> (a's result, b's result)."""
    from crfp_amd import ops
    a = ops.conv_probe(cc.probe_spec(dataclasses.replace(conv_a, dsts=None), ia, DEV), storage="f32")
    b = ops.conv_probe(cc.probe_spec(conv_b, dict(ib, srcs=[a["out"][0][0]]), DEV), storage="f32")
    assert a["kernel"] == ("split8", "none") and b["kernel"] == ("split8", "none")
    return a, b


# ---------------------------------------------------------------- a. pair == conv a, then conv b on a's output
@pytest.mark.parametrize("which", pc.EXACT_KINDS + ("normal",))
@pytest.mark.parametrize("shape", ["res", "block", "block_relu"])
@pytest.mark.parametrize("hw", pc.GEOMETRY, ids=GEOM_ID)
def test_pair_equals_its_two_launches(hw, shape, which):
    """Every destination element written and equal to the two launches' bit for bit, on exact inputs and on ordinary data; on exact inputs
    with exact activations (res, block_relu) also equal to the float64 result (the lrelu form: see the helper's docstring)."""
    h, w = hw
    conv_a, conv_b, ia, ib = pc.pair_inputs(shape, h, w, which)
    r = run_pair(conv_a, conv_b, ia, ib)
    a, b = run_two_launches(conv_a, conv_b, ia, ib)
    assert len(r["out"][1]) == len(b["out"][0]) == (1 if conv_b.dsts is None else len(conv_b.dsts))
    for d, (got, want) in enumerate(zip(r["out"][1], b["out"][0])):
        same_bits(got, want, f"{shape} {h}x{w} {which}: destination {d} against two launches")
    assert torch.equal(r["status"].cpu()[0], a["status"].cpu()[0]) and torch.equal(r["status"].cpu()[1], b["status"].cpu()[0])
    assert int(r["status"].abs().sum()) == 0
    if which != "normal" and pc.exact_ok(shape, h, w, which):
        ra, rb = pc.exact_reference(shape, h, w, which)
        same_bits(a["out"][0][0], ra["full"].float(), "conv a alone against float64")
        for d, (got, want) in enumerate(zip(r["out"][1], rb["out"])):
            same_bits(got, want.float(), f"{shape} {h}x{w} {which}: destination {d} against float64")


# ---------------------------------------------------------------- b. the fp16-operand range guard
@pytest.mark.parametrize("shape", ["res", "block"])
def test_guard_raises_the_words_the_two_launches_raise(shape):
    """conv a's input scaled until its activated output passes 65504: the pair raises conv a's word (and conv b's, whose input then holds
    infinite fp16 heads) exactly where the two launches do; in range, every word stays 0."""
    h, w = 9, 63
    for scale, fires in ((3.0e4, True), (1.0, False)):
        conv_a, conv_b, ia, ib = pc.overflow_inputs(shape, h, w, scale)
        r = run_pair(conv_a, conv_b, ia, ib)
        a, b = run_two_launches(conv_a, conv_b, ia, ib)
        if fires:
            assert bool(torch.isfinite(a["out"][0][0]).all()) and float(a["out"][0][0].abs().max()) > 65504
        sa, sb = a["status"].cpu()[0], b["status"].cpu()[0]
        assert bool((sa != 0).all()) == fires and bool((sa != 0).any()) == fires
        assert torch.equal(r["status"].cpu()[0], sa), (scale, r["status"], sa)
        assert torch.equal(r["status"].cpu()[1], sb), (scale, r["status"], sb)
        if not fires:
            assert int(r["status"].abs().sum()) == 0


# ---------------------------------------------------------------- c. the engines: CRFP_CONV_PAIR=0 against =2
def _engine_runs(h, w):
    script = os.path.join(os.path.dirname(__file__), "helpers", "run_pair_engine_check.py")
    procs = []
    for mode in ("0", "2"):   # the switch is read once per process; the two children run side by side
        procs.append(subprocess.Popen([sys.executable, script, str(h), str(w)], env=dict(os.environ, CRFP_CONV_PAIR=mode),
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    res = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-3000:]
        res.append({l.split()[1]: tuple(l.split()[2:]) for l in out.splitlines() if l.startswith("RUN ")})
    return res


@pytest.mark.parametrize("hw", [(20, 36), (33, 47)], ids=GEOM_ID)
def test_engines_are_bit_identical_with_and_without_pairs(hw):
    """3-frame clips (2x maps 40 x 72 and 66 x 94: two column tiles, ragged last rows; level 0's dcn_block.2 writes its SRC_S3 image from
    the pair kernel): outputs and status of DSV, CRA, simple, dense, a DSV lock-step batch of 2 and 3 streamed DSV frames."""
    two, one = _engine_runs(*hw)
    assert set(two) == {"dsv", "dsv_batch2", "dsv_stream", "cra", "simple", "dense"}
    assert one == two
    assert all(v[1] == "0" for v in one.values())
