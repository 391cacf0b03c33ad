"""Cases, inputs and the float64 reference of the conv probe tests (test_conv_cases.py on the CPU, test_gpu_conv_probe.py on the GPU).

The reference restates the whole operator of one conv launch in torch CPU double: the virtual concat of the sources (plain tensors,
pixel_unshuffle(4), the (dx, dy) flow channels), 3x3 conv + bias as nine shifted matrix products, activation, post_scale, residual, and the
store: channel ranges, pixel_shuffle(r), or the DCN offset / mask epilogue (10 tanh + flow flipped to (y, x) on the offset quads, sigmoid on
the rest; model/CRFP.py:337-340).

Exact inputs.  "Coarse" values are k / 2, k in -2 .. 2; "fine" values are coarse + m 2^-12, m in -3 .. 3; bias and residual are multiples
of 1/4, post_scale a power of two, the activation none or relu.  With one operand coarse the x1 w1 term the f16x3 scheme drops is zero, and
every product of the three that remain is a multiple of 2^-13 in true scale (fine operand: fp16 head a multiple of 2^-11, scaled tail a
multiple of 1/2; coarse operand: a multiple of 1/2).  A partial sum of such terms, in any order, is bounded by S = sum |x| |w| + |b|, so it
needs at most log2(S) + 13 bits: it is an fp32 value while S <= 2^11 -- in the two-accumulator form (head and scaled tail apart) and in the
single-accumulator form (everything scaled by 2^11) alike.  Then no addition rounds and a correct kernel returns the float64 result bit for
bit.  (2^11 is half of what one accumulator of heads alone would allow; it is what the single-accumulator form and the final hi + lo / 2^11
need, so it is the bound every case is held to: `sigma_bound_ok`.)  bf16 build: both operands coarse, bf16-exact, products multiples of
1/4 -- exact with 2^24 of headroom; the one rounding left is the store's, so the expected output is rne_bf16(reference)."""
import dataclasses
import functools

import numpy as np
import torch

SIGMA_MAX = 2.0 ** 11


@dataclasses.dataclass(frozen=True)
class Conv:
    srcs: tuple                 # ((kind, channels[, pad]), ...): kind "q4" / "unshuf4" / "flow2"
    cout: int
    store: str = "q4"           # "q4" / "ps" / "offmask"
    ps_r: int = 0
    act: str = "none"
    post_scale: float = 1.0
    residual: bool = False
    dsts: tuple = None          # ((q0, q1[, pad]), ...); None: one destination with every quad
    cout_split: int = 0         # > 0: rows >= cout_split come from a second weight / bias pair
    n_off_quads: int = 0
    strict: bool = False
    dst_f32: bool = False

    @property
    def cin(self):
        return sum(s[1] for s in self.srcs)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    conv: Conv
    n: int
    h: int
    w: int
    kernel: tuple               # the variant the launcher must choose: (fp32 build, bf16 build)


def Q(c, pad=0):
    return ("q4", c, pad)


# ---------------------------------------------------------------- the cases of the GPU tests
# exactness: a list, not a cross product -- every geometry of the issue ((1,1) (3,63) (4,64) (5,65) (8,64) (9,130) (17,33) (7,129), n in 1, 3)
# and every channel plan appear at least once
EXACT = (
    Case("q16_to_32", Conv((Q(16),), 32), 1, 1, 1, ("split8", "bf16_4w")),                       # one chunk
    Case("q32_to_32", Conv((Q(32),), 32), 3, 3, 63, ("split8", "bf16_x8")),                      # even chunks
    Case("block0", Conv((Q(24), Q(8), Q(32), ("flow2", 2)), 32), 3, 4, 64, ("split8", "bf16_4w")),   # 5 chunks
    Case("q32_q16", Conv((Q(32), Q(16)), 32, act="relu"), 1, 5, 65, ("split8", "bf16_4w")),
    Case("cout2", Conv((Q(32),), 2), 1, 8, 64, ("split8", "bf16_x8")),
    Case("cout30", Conv((Q(32),), 30), 3, 9, 130, ("split8", "bf16_x8")),
    Case("cout33", Conv((Q(32),), 33), 1, 17, 33, ("split4", "bf16_4w")),
    Case("cout64", Conv((Q(32),), 64, act="relu"), 1, 7, 129, ("split4", "bf16_4w")),
    Case("cout216", Conv((Q(32),), 216), 1, 5, 65, ("split4", "bf16_4w")),
    Case("q256_to_256", Conv((Q(256),), 256), 1, 3, 63, ("split4", "bf16_4w")),
    Case("q320", Conv((Q(320),), 32), 1, 8, 64, ("split8", "bf16_x8")),                           # kq = CRFP_MAX_KQ
    Case("q324", Conv((Q(324),), 32), 1, 4, 64, ("mfma_rows4", "mfma_rows4")),                    # over the table: fp32-MFMA fallback
    Case("unshuf4", Conv((("unshuf4", 64),), 32), 3, 5, 65, ("split8", "bf16_x8")),
    Case("ps2", Conv((Q(32),), 64, store="ps", ps_r=2), 3, 9, 130, ("split4", "bf16_4w")),
    Case("ps4", Conv((Q(24),), 64, store="ps", ps_r=4, post_scale=2.0), 1, 17, 33, ("split4", "bf16_4w")),
    Case("three_dsts", Conv((Q(32),), 40, dsts=((0, 3), (3, 4, 1), (4, 10))), 3, 7, 129, ("split4", "bf16_4w")),
    Case("p4_source", Conv((Q(32, 1),), 32), 3, 8, 64, ("split8", "bf16_x8")),
    Case("residual", Conv((Q(32),), 32, act="relu", residual=True), 3, 5, 65, ("split8", "bf16_x8")),
    Case("strict", Conv((Q(32),), 32, strict=True), 1, 9, 130, ("mfma_rows4", "mfma_rows4")),
    Case("dst_f32", Conv((Q(320),), 32, dst_f32=True), 3, 3, 63, ("split8", "bf16_x8")),          # bf16 build: float quads, no storage rounding
)
# dispatch edge: N * 8-row tiles = 19 * 9 * 3 = 513 leaves the bf16 build's 8-wave kernel (one round of 512 slots); n = 1 stays on it
EDGE_513 = Case("edge513", Conv((Q(32),), 32), 19, 72, 192, ("split8", "bf16_4w"))
EDGE_1 = Case("edge513_n1", Conv((Q(32),), 32), 1, 72, 192, ("split8", "bf16_x8"))
# dual launch: 4-row tiles * cout tiles a multiple of 8 (4 tiles * 2) -> one launch in the fp32 build; 3 tiles * 2 -> two launches
DUAL_A = Conv((Q(32),), 64, act="relu")
DUAL_B = Conv((Q(32), Q(16)), 48, store="q4")
DUAL = (("dual_fused", 2, 8, 65, ("split_dual", "split_dual"), ("bf16_4w", "bf16_4w")),
        ("dual_two_launches", 2, 9, 64, ("split4", "split4"), ("bf16_4w", "bf16_4w")))
# pair kernel (bf16 build): 62-column tiles of 8 rows
PAIR_A = Conv((Q(256), Q(64)), 32, act="relu", post_scale=0.5, dsts=())   # 320 channels: outputs past 8 significant bits, so the middle tensor really rounds
PAIR_B = Conv((Q(32),), 32)
PAIR_GEOMETRY = ((7, 61), (8, 62), (9, 63), (8, 124), (7, 125))
# S3 chain (fp32 build)
CHAIN_A = Conv((Q(16),), 32, act="relu", dsts=())
CHAIN_B = Conv((Q(32),), 64)
# bounded error on ordinary data
NORMAL = (
    Case("lrelu_1tile", Conv((Q(32), Q(32), ("flow2", 2)), 32, act="lrelu"), 2, 9, 70, ("split8", "bf16_4w")),
    Case("lrelu_2tiles", Conv((Q(64),), 64, act="lrelu"), 1, 9, 70, ("split4", "bf16_4w")),
    Case("offmask", Conv((Q(32),), 216, store="offmask", cout_split=144, n_off_quads=36), 2, 9, 70, ("split4", "bf16_4w")),
)


# ---------------------------------------------------------------- number formats
def rne_bf16(t):
    """float tensor -> nearest bf16 value (ties to even), as float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def coarse(rs, shape):
    return rs.randint(-2, 3, shape) * 0.5


def fine(rs, shape):
    return coarse(rs, shape) + rs.randint(-3, 4, shape) * 2.0 ** -12


def quarters(rs, shape):
    return rs.randint(-8, 9, shape) * 0.25


def src_shape(s, n, h, w):
    kind, c = s[0], s[1]
    return {"q4": (n, c, h, w), "unshuf4": (n, c // 16, 4 * h, 4 * w), "flow2": (n, h, w, 2)}[kind]


def make_inputs(conv, n, h, w, which, seed=0):
    """float32 CPU tensors of one conv.  which: "fine_x" / "fine_w" (the other operand coarse), "coarse" (both), or "normal"
    (standard-normal x, weights * 1.5 / sqrt(9 cin): both operands with full mantissas)."""
    rs = np.random.RandomState(seed)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if which == "normal":
        gx = lambda shp: rs.randn(*shp)
        gw = lambda shp: rs.randn(*shp) * 1.5 / np.sqrt(9 * conv.cin)
        gb = lambda shp: rs.randn(*shp) * 0.5
    else:
        gx = (lambda shp: fine(rs, shp)) if which == "fine_x" else (lambda shp: coarse(rs, shp))
        gw = (lambda shp: fine(rs, shp)) if which == "fine_w" else (lambda shp: coarse(rs, shp))
        gb = lambda shp: quarters(rs, shp)
    d = {"srcs": [T(gx(src_shape(s, n, h, w))) for s in conv.srcs]}
    c1 = conv.cout_split if conv.cout_split else conv.cout
    d["weight"], d["bias"] = T(gw((c1, conv.cin, 3, 3))), T(gb((c1,)))
    if conv.cout_split:
        d["weight2"], d["bias2"] = T(gw((conv.cout - c1, conv.cin, 3, 3))), T(gb((conv.cout - c1,)))
    if conv.residual:
        d["residual"] = T(gb((n, conv.cout, h, w)))
    if conv.store == "offmask":
        d["flow"] = T(gx((n, h, w, 2)) * (4.0 if which == "normal" else 1.0))
    return d


# ---------------------------------------------------------------- the reference
def concat_sources(conv, srcs):
    parts = []
    for s, t in zip(conv.srcs, srcs):
        t = t.double()
        if s[0] == "unshuf4":   # channel c of the 4x tensor -> channels 16 c + 4 i + j, (i, j) the position inside the 4 x 4 cell
            nn_, c, H4, W4 = t.shape
            t = t.reshape(nn_, c, H4 // 4, 4, W4 // 4, 4).permute(0, 1, 3, 5, 2, 4).reshape(nn_, 16 * c, H4 // 4, W4 // 4)
        elif s[0] == "flow2":
            t = t.permute(0, 3, 1, 2)
        parts.append(t)
    return torch.cat(parts, dim=1)


def conv3x3_f64(x, w):
    """3x3, stride 1, zero padding 1, as nine shifted matrix products -> (conv, sum |x| |w|) in float64."""
    n, c, H, W = x.shape
    xp = torch.zeros((n, c, H + 2, W + 2), dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    out = torch.zeros((n, w.shape[0], H, W), dtype=torch.float64)
    mag = torch.zeros_like(out)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + H, kx:kx + W]
            out += torch.einsum("oc,nchw->nohw", w[:, :, ky, kx], win)
            mag += torch.einsum("oc,nchw->nohw", w[:, :, ky, kx].abs(), win.abs())
    return out, mag


def pixel_shuffle_f64(t, r):
    n, c, H, W = t.shape
    return t.reshape(n, c // (r * r), r, r, H, W).permute(0, 1, 4, 2, 5, 3).reshape(n, c // (r * r), H * r, W * r)


def reference(conv, inp, x_override=None):
    """-> dict: out (list of float64 destination tensors), full (the [n, cout, h, w] result before the store's layout step),
    pre (conv + bias, before the activation), S (sum |x| |w| + |b| per element of full).  x_override: the concatenated input."""
    x = concat_sources(conv, inp["srcs"]) if x_override is None else x_override.double()
    w = inp["weight"].double()
    b = inp["bias"].double()
    if conv.cout_split:
        w, b = torch.cat([w, inp["weight2"].double()], 0), torch.cat([b, inp["bias2"].double()], 0)
    pre, mag = conv3x3_f64(x, w)
    pre = pre + b.view(1, -1, 1, 1)
    S = mag + b.abs().view(1, -1, 1, 1)
    if conv.store == "offmask":
        fl = inp["flow"].double()
        full = torch.sigmoid(pre)
        noff = 4 * conv.n_off_quads
        off = 10.0 * torch.tanh(pre[:, :noff])
        off[:, 0::2] += fl[..., 1].unsqueeze(1)   # (dy, dx) pairs: + flow flipped to (y, x)
        off[:, 1::2] += fl[..., 0].unsqueeze(1)
        full[:, :noff] = off
    else:
        v = {"none": pre, "relu": pre.clamp(min=0), "lrelu": torch.where(pre > 0, pre, 0.1 * pre)}[conv.act]
        full = v * conv.post_scale
        if conv.residual:
            full = full + inp["residual"].double()
    if conv.store == "ps":
        out = [pixel_shuffle_f64(full, conv.ps_r)]
    elif conv.dsts is None:
        out = [full]
    else:
        out = [full[:, 4 * d[0]:min(4 * d[1], conv.cout)] for d in conv.dsts]
    return {"out": out, "full": full, "pre": pre, "S": S}


def sigma_bound_ok(conv, ref):
    """The condition on exact inputs under which a correct kernel is exact: every partial sum an fp32 value."""
    s = ref["S"].max().item() * max(conv.post_scale, 1.0)
    if conv.residual:
        s += 2.0
    return s <= SIGMA_MAX


@functools.lru_cache(maxsize=None)
def exact_case(name, which):
    """(case, inputs, reference) of an EXACT / EDGE case: computed once, shared by the tests, never modified."""
    case = {c.name: c for c in EXACT + (EDGE_513, EDGE_1)}[name]
    inp = make_inputs(case.conv, case.n, case.h, case.w, which, seed=sum(map(ord, name)))
    return case, inp, reference(case.conv, inp)


def probe_spec(conv, inp, dev):
    """The dict crfp_amd.ops.conv_probe takes for one conv, tensors on `dev`."""
    spec = {"srcs": [(s[0], t.to(dev)) + ((s[2],) if len(s) > 2 else ()) for s, t in zip(conv.srcs, inp.get("srcs", []))],
            "store": conv.store, "ps_r": conv.ps_r, "act": conv.act, "post_scale": conv.post_scale, "n_off_quads": conv.n_off_quads,
            "strict": conv.strict, "dst_f32": conv.dst_f32}
    if conv.dsts is not None:
        spec["dsts"] = conv.dsts
    for k in ("weight", "bias", "weight2", "bias2", "residual", "flow"):
        if k in inp:
            spec[k] = inp[k].to(dev)
    return spec


@functools.lru_cache(maxsize=None)
def dual_case(name, which):
    """-> (n, h, w, (inputs a, inputs b), (reference a, reference b)) of a DUAL geometry."""
    _, n, h, w, _, _ = {d[0]: d for d in DUAL}[name]
    ia, ib = make_inputs(DUAL_A, n, h, w, which, seed=11), make_inputs(DUAL_B, n, h, w, which, seed=12)
    return n, h, w, (ia, ib), (reference(DUAL_A, ia), reference(DUAL_B, ib))


@functools.lru_cache(maxsize=None)
def pair_case(h, w, resid):
    """bf16 pair kernel, exact inputs -> (conv b, inputs a, inputs b, middle tensor, reference of b on the middle tensor); n = 2.
    The middle tensor is what conv a stores: rne_bf16(relu(a) * post_scale)."""
    conv_b = dataclasses.replace(PAIR_B, residual=bool(resid), act="relu" if resid else "none")
    ia, ib = make_inputs(PAIR_A, 2, h, w, "coarse", seed=100 + h + w), make_inputs(conv_b, 2, h, w, "coarse", seed=200 + h + w)
    ra = reference(dataclasses.replace(PAIR_A, dsts=None), ia)
    mid = rne_bf16(ra["full"])
    return conv_b, ia, ib, mid, ra, reference(conv_b, ib, x_override=mid)


@functools.lru_cache(maxsize=None)
def chain_case(which):
    """fp32 S3 chain on a 9 x 70 map, n = 2 -> (inputs a, inputs b, reference a, reference b on a's output)."""
    ia, ib = make_inputs(CHAIN_A, 2, 9, 70, which, seed=31), make_inputs(CHAIN_B, 2, 9, 70, "coarse" if which != "normal" else "normal", seed=32)
    ib.pop("srcs")   # conv b's only source is conv a's output
    ra = reference(dataclasses.replace(CHAIN_A, dsts=None), ia)
    return ia, ib, ra, reference(CHAIN_B, ib, x_override=ra["full"])
