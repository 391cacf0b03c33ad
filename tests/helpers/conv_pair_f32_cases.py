"""Cases, inputs and references of the fp32 pair-kernel tests (test_conv_pair_f32_cases.py on the CPU, test_gpu_conv_pair_f32.py on the GPU).

conv3x3_pair_kernel runs conv a (32 couts) and conv b (32 -> 32) in one launch on 8-row x 60-column output tiles; the tensor between them
never leaves LDS.  Two shapes, the two sites the engines fuse:

  res    a: 32 -> 32 relu;  b: 32 -> 32, no activation, + residual, destinations quads [0, 6) plain and [6, 8) in padded planes
  block  a: Q24 | Q8 | Q32 | flow2 -> 32 lrelu (66 channels: five 16-channel chunks, the last one masked);  b: 32 -> 32 lrelu -> Q4

Exact inputs.  conv a takes conv_cases' "fine_x" / "fine_w" inputs (one operand fine, the other coarse), so its sums are multiples of 2^-13
and exact while sum |x| |w| + |b| <= 2^11.  Its output v (after relu) is a multiple of 2^-13, and the split conv b applies keeps 11 + 11
bits of it: v = fp16(v) + 2^-11 fp16(2^11 (v - fp16(v))) holds while the tail (a multiple of 2^-13 below half an fp16 ulp of v) has at
most 11 bits, i.e. |v| < 2^10.  conv b's weights are coarse (fp16 values, no tail), its products multiples
of 2^-14, and its sums exact while S_b = sum |v| |w| + |b| (+ |residual|) <= 2^10 (24 bits over 2^-14).  Coarse weights on 288 taps of
a tensor with |v| ~ 4 sum to about 2^10, so conv b's weights are thinned to a quarter of their taps (every tap and channel still occurs);
`exact_ok` asserts all of this for every case the GPU test runs.
LeakyReLU multiplies by 0.1f: not exact in binary, and a negative v no longer splits into 11 + 11 bits.  The float64 equality of the block
shape therefore runs with relu in both convs ("block_relu"); the lrelu form itself ("block") runs on the same exact inputs and on ordinary
data against its two launches, which is the check that does not depend on the activation."""
import dataclasses
import functools

import numpy as np
import torch

import conv_cases as cc

# cc.PAIR_GEOMETRY is built around 62-column tiles; the fp32 kernel's tiles are 60 wide: its own edges (59 / 60 / 61, 120 / 121) are added
GEOMETRY = cc.PAIR_GEOMETRY + ((19, 130), (3, 5), (8, 59), (9, 60), (8, 121))
N = 2

RES_A = cc.Conv((cc.Q(32),), 32, act="relu", dsts=())
RES_B = cc.Conv((cc.Q(32),), 32, act="none", residual=True, dsts=((0, 6), (6, 8, 1)))
BLOCK_SRCS = (cc.Q(24), cc.Q(8), cc.Q(32), ("flow2", 2))
BLOCK_A = cc.Conv(BLOCK_SRCS, 32, act="lrelu", dsts=())
BLOCK_B = cc.Conv((cc.Q(32),), 32, act="lrelu")
SHAPES = {
    "res": (RES_A, RES_B),
    "block": (BLOCK_A, BLOCK_B),
    "block_relu": (dataclasses.replace(BLOCK_A, act="relu"), dataclasses.replace(BLOCK_B, act="relu")),
}
EXACT_KINDS = ("fine_x", "fine_w")
S_B_MAX = 2.0 ** 10


@functools.lru_cache(maxsize=None)
def pair_inputs(shape, h, w, which):
    """-> (conv a, conv b, inputs a, inputs b); which: "fine_x" / "fine_w" / "normal"."""
    conv_a, conv_b = SHAPES[shape]
    seed = 1000 + 7 * h + w + sum(map(ord, shape))
    ia = cc.make_inputs(conv_a, N, h, w, which, seed=seed)
    ib = cc.make_inputs(conv_b, N, h, w, "coarse" if which != "normal" else "normal", seed=seed + 1)
    ib.pop("srcs")   # conv b's only source is conv a's output
    if which != "normal":
        keep = np.random.RandomState(seed + 2).randint(0, 4, tuple(ib["weight"].shape)) == 0
        ib["weight"] = ib["weight"] * torch.from_numpy(keep.astype(np.float32))
    return conv_a, conv_b, ia, ib


@functools.lru_cache(maxsize=None)
def exact_reference(shape, h, w, which):
    """float64: -> (reference of a, reference of b on a's output)."""
    conv_a, conv_b, ia, ib = pair_inputs(shape, h, w, which)
    ra = cc.reference(dataclasses.replace(conv_a, dsts=None), ia)
    return ra, cc.reference(conv_b, ib, x_override=ra["full"])


def exact_ok(shape, h, w, which):
    """The conditions of the module docstring under which a correct pair returns the float64 result bit for bit."""
    conv_a, conv_b, ia, ib = pair_inputs(shape, h, w, which)
    if conv_a.act == "lrelu" or conv_b.act == "lrelu":
        return False
    ra, rb = exact_reference(shape, h, w, which)
    mid = ra["full"]
    s_b = float(rb["S"].max()) + (2.0 if conv_b.residual else 0.0)
    return cc.sigma_bound_ok(conv_a, ra) and float(mid.abs().max()) < 2.0 ** 10 and bool(torch.equal(mid * 2 ** 13, (mid * 2 ** 13).round())) and s_b <= S_B_MAX


def overflow_inputs(shape, h, w, scale):
    """Ordinary data with conv a's input scaled by `scale` and clamped to +-3e4: the input itself stays an fp16 operand, and with
    scale = 3e4 conv a's activated output (standard deviation about 1.5 x the input's) passes 65504 in every batch item."""
    conv_a, conv_b, ia, ib = pair_inputs(shape, h, w, "normal")
    ia = dict(ia, srcs=[(t * scale).clamp(-3.0e4, 3.0e4) for t in ia["srcs"]])
    return conv_a, conv_b, ia, ib
