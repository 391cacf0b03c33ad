"""Cases, inputs and the float64 reference of the narrow-conv probe tests (test_narrow_cases.py on the CPU, test_gpu_narrow_probe.py on the GPU).

The reference restates the whole operator of one launch of csrc/conv_narrow.hip in torch CPU double: the virtual concat of the sources (Q4
tensors, the flow field as (dx, dy)), 3x3 conv + bias, the activation as the kernels compute it -- max(v, slope v) with slope the fp32 value
0.1f and the product rounded once to fp32 --, post_scale, residual, and the four epilogues:
  plain     act(conv) * post_scale (+ residual), channels >= cout zero
  blend     lrelu(mask ? conv : centre value of source 0's first quad)                                   (model/CRFP.py:1672-1675)
  last      conv + x8 bilinear (align_corners False) of base_lr, y_only: + its luma 0.299 / 0.587 / 0.114 (model/CRFP.py:1678-1683)
  offmask3  (10 tanh(o0) + flow_y, 10 tanh(o1) + flow_x, sigmoid(o2), 0)                                 (model/CRFP.py:337-347)
and dst2 = lrelu of what dst receives.  A pair is a -> b, a chain a -> b -> c (c may read one more global quad, `res`: c adds a's output);
the tensor between two stages has four channels (those >= cout zero) and is zero outside the image.

bf16 storage (storage="bf16"): rne_bf16 wherever the build stores an activation -- Q4 sources and the residual on their way in
(launch_nchw_to_q4), the weights (narrow_pack_kernel; the bias stays fp32), the tensors between the stages of a pair / chain (quad_to_bits in the
pair and chain kernels), dst of the plain and blend epilogues (stq), dst2 computed from the ROUNDED dst and rounded again
(narrow_store_state).  Flow fields, base_lr, and the float destinations of last and offmask3 stay fp32.

Exact inputs (fp32): "coarse" values are k / 2, "fine" values coarse + m 2^-12 (conv_cases.py); one operand of the first stage fine, the other
coarse, every later stage's weights coarse.  The narrow kernels accumulate in true fp32 (v_mfma_f32_4x4x1 / v_fma_f32, -ffp-contract=off), so a
stage whose inputs are multiples of 2^-i and whose weights are multiples of 2^-j rounds nothing while its partial sums, multiples of
2^-(i+j) bounded by S = sum |x| |w| + |b|, fit 24 bits: log2(S) + i + j <= 24.  Its output is then a multiple of 2^-(i+j) (2^-(i+j+1) after
post_scale 0.5), which is the next stage's i.  `exact_ok` asserts that stage by stage; later stages use sparse weights so that S stays small.
bf16: every operand coarse (bf16-exact), products multiples of 1/4, and rne_bf16 of a multiple of 2^-i is one again: the same rule holds with
2^24 of headroom, and the expected output is the reference with its storage roundings."""
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conv_cases import coarse, conv3x3_f64, fine, quarters, rne_bf16

SLOPE = float(np.float32(0.1))
LUMA = (np.float32(0.299), np.float32(0.587), np.float32(0.114))
TILE_W, TILE_H = 64, 16
# fp32 build: fine x against coarse weights, and coarse x against fine weights; bf16 build: both coarse (bf16 values)
EXACT_RUNS = (("f32", "fine_x"), ("f32", "fine_w"), ("bf16", "coarse"))


@dataclasses.dataclass(frozen=True)
class Stencil:
    srcs: tuple                 # (("q4", channels) / ("flow2", 2), ...): the global sources this stencil brings itself
    cout: int
    act: str = "none"
    post_scale: float = 1.0
    residual: bool = False
    epi: str = "plain"
    y_only: bool = False
    cout_split: int = 0
    src_pad: int = 0
    dst_pad: int = 0
    dst2: bool = False
    gate_h: int = None

    def cin(self, fed):
        return (4 if fed else 0) + sum(s[1] for s in self.srcs)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    mode: str                   # "single" / "pair" / "chain"
    st: tuple                   # 1 .. 3 stencils
    n: int
    h: int
    w: int
    which: str = "fine_x"       # exact inputs of the fp32 build: which operand of stage a is fine (the exactness tests run both)
    res: bool = False
    kern: tuple = (None, None)  # the variant the launcher must choose, as variant() spells it: (fp32 build, bf16 build); None: refused there


def Q(c):
    return ("q4", c)


FLOW = ("flow2", 2)


def variant(rep):
    """A probe report as `family<template arguments>`."""
    k = rep["kernel"]
    if k == "narrow":
        return f"narrow<{rep['kq']},{rep['epi']}" + (",gate" if rep["gate"] else "") + (",st2" if rep["st2"] else "") + ">"
    if k == "seq":
        return f"seq<{rep['kq']}>"
    if k == "pair":
        return f"pair<{rep['kq']},{rep['epi']}>"
    return f"chain<{rep['kq']},{rep['kqg']},{'res' if rep['res'] else 'nores'}>"


def S1(srcs, cout, kq, epi="plain", extra="", **kw):
    """A single stencil and the variants it must reach: the fp32 build's plain stencils take the quad-sequential form."""
    plain = epi == "plain" and not kw.get("dst2") and kw.get("gate_h") is None
    tail = ("," + extra if extra else "")
    return Stencil(srcs, cout, epi=epi, **kw), (f"seq<{kq}>" if plain else f"narrow<{kq},{epi}{tail}>", f"narrow<{kq},{epi}{tail}>")


def _single(name, n, h, w, which, st_kern):
    return Case(name, "single", (st_kern[0],), n, h, w, which, kern=st_kern[1])


# ---------------------------------------------------------------- the cases of the GPU tests
# exactness: a list, not a cross product -- every geometry of the issue ((1,1) (15,63) (16,64) (17,65) (16,60) (17,61) (49,193) (49,181),
# n in 1, 3), every source table of the engines (3 + 3, 4, 4 + 4, 4 + 4 + flow, 2), cout 1 .. 4, act none / relu, post_scale 0.5, residual,
# P4 planes, a window of pitch excess 37, the epilogues, dst2, and the pair / chain forms appear at least once
EXACT = (
    _single("k1_1x1", 1, 1, 1, "fine_x", S1((Q(4),), 4, 1)),
    _single("k1_src2_cout1", 3, 15, 63, "fine_w", S1((Q(2),), 1, 1, act="relu")),
    _single("k2_3_3_cout2_half", 1, 16, 64, "fine_x", S1((Q(3), Q(3)), 2, 2, post_scale=0.5)),
    _single("k2_4_4_cout3_res", 3, 17, 65, "fine_w", S1((Q(4), Q(4)), 3, 2, act="relu", residual=True)),
    _single("k3_flow_interior", 1, 49, 193, "fine_x", S1((Q(4), Q(4), FLOW), 4, 3)),
    _single("k1_res_interior", 1, 49, 193, "fine_w", S1((Q(4),), 4, 1, residual=True)),
    _single("k2_ragged_interior", 3, 49, 181, "fine_x", S1((Q(4), Q(4)), 4, 2, act="relu")),
    _single("k3_chain_geometry", 1, 17, 61, "fine_w", S1((Q(4), Q(4), Q(4)), 4, 3)),
    _single("p4_planes", 3, 17, 65, "fine_x", S1((Q(4),), 4, 1, src_pad=1, dst_pad=1)),
    _single("window37", 3, 17, 65, "fine_w", S1((Q(4),), 4, 1, act="relu", src_pad=37, dst_pad=37)),
    _single("window37_k2", 1, 16, 60, "fine_x", S1((Q(4), Q(4)), 4, 2, src_pad=37, dst_pad=37)),
    _single("blend_k2", 3, 17, 65, "fine_x", S1((Q(4), Q(4)), 4, 2, epi="blend")),
    _single("blend_k2_interior", 1, 49, 193, "fine_w", S1((Q(4), Q(4)), 4, 2, epi="blend")),
    _single("last_rgb", 3, 16, 64, "fine_x", S1((Q(4),), 3, 1, epi="last")),
    _single("last_rgb_interior", 1, 48, 192, "fine_w", S1((Q(4),), 3, 1, epi="last")),
    _single("last_y", 1, 48, 192, "fine_x", S1((Q(4),), 1, 1, epi="last", y_only=True)),
    _single("dst2", 3, 17, 65, "fine_x", S1((Q(4),), 4, 1, extra="st2", residual=True, dst2=True)),
    _single("dst2_interior", 1, 49, 193, "fine_w", S1((Q(4),), 4, 1, extra="st2", dst2=True)),
    # pairs: KQA 1 .. 3, b plain, with and without residual and dst2
    Case("pair_k1_res_dst2", "pair", (Stencil((Q(4),), 4, act="relu"), Stencil((), 4, residual=True, dst2=True)), 3, 17, 65, "fine_x",
         kern=("pair<1,plain>", "pair<1,plain>")),
    Case("pair_k2", "pair", (Stencil((Q(3), Q(3)), 4, act="relu"), Stencil((), 4)), 1, 15, 63, "fine_w", kern=("pair<2,plain>", "pair<2,plain>")),
    Case("pair_k3_half_res", "pair", (Stencil((Q(4), Q(4), FLOW), 4, act="relu", post_scale=0.5), Stencil((), 3, residual=True)), 1, 49, 193,
         "fine_x", kern=("pair<3,plain>", "pair<3,plain>")),
    Case("pair_k1_cout2_dst2", "pair", (Stencil((Q(4),), 2), Stencil((), 4, act="relu", dst2=True)), 1, 16, 64, "fine_w",
         kern=("pair<1,plain>", "pair<1,plain>")),
) + tuple(
    # chains: the three shapes of the fp32 launcher for KQA 1 .. 3; the bf16 launcher takes res for KQA <= 2 and the second global quad
    Case(f"chain_k{kq}_{shape}", "chain",
         (Stencil(srcs, 4, act="relu"), Stencil((), 4, act="relu", post_scale=0.5 if kq == 2 else 1.0),
          Stencil((Q(4),) if shape == "g" else (), 4 if kq != 3 else 3, dst2=(shape == "res" and kq != 2))),
         n, h, w, which, res=shape == "res",
         kern=(f"chain<{kq},{1 if shape == 'g' else 0},{'res' if shape == 'res' else 'nores'}>",
               f"chain<{kq},{1 if shape == 'g' else 0},{'res' if shape == 'res' else 'nores'}>" if (shape == "g" or (shape == "res" and kq <= 2)) else None))
    for kq, srcs in ((1, (Q(4),)), (2, (Q(4), Q(4))), (3, (Q(4), Q(4), FLOW)))
    for shape, (n, h, w, which) in (("res", ((3, 17, 61, "fine_x"), (1, 49, 181, "fine_w"), (1, 16, 60, "fine_x"))[kq - 1]),
                                    ("g", ((1, 49, 181, "fine_w"), (3, 16, 60, "fine_x"), (1, 17, 61, "fine_w"))[kq - 1]),
                                    ("plain", ((1, 16, 60, "fine_x"), (1, 17, 61, "fine_w"), (3, 15, 63, "fine_x"))[kq - 1]))
)

# the persistent walk: one stencil per kernel family; the GPU test grows the map until the launcher reports workgroups < tiles
WALK = (
    _single("walk_narrow_blend", 1, 0, 2040, "fine_x", S1((Q(4), Q(4)), 4, 2, epi="blend")),
    _single("walk_plain_k3", 1, 0, 2040, "fine_w", S1((Q(4), Q(4), Q(4)), 4, 3)),          # fp32: seq<3>, bf16: narrow<3,plain>
    Case("walk_pair", "pair", (Stencil((Q(4),), 4, act="relu"), Stencil((), 4, residual=True)), 1, 0, 2040, "fine_x",
         kern=("pair<1,plain>", "pair<1,plain>")),
    Case("walk_chain", "chain", (Stencil((Q(4),), 4, act="relu"), Stencil((), 4, act="relu"), Stencil((), 4)), 1, 0, 2040, "fine_w", res=True,
         kern=("chain<1,0,res>", "chain<1,0,res>")),
)
WALK_HEIGHTS = (330, 650, 970, 1290, 1610)   # ragged on both axes with w = 2040: 31.9 tile columns, 20.6 .. 100.6 tile rows

# bounded error on ordinary data: every epilogue, lrelu
NORMAL = (
    _single("n_plain_k3_flow", 2, 17, 65, "normal", S1((Q(4), Q(4), FLOW), 4, 3, act="lrelu")),
    _single("n_plain_k1_res", 2, 17, 65, "normal", S1((Q(4),), 4, 1, act="lrelu", residual=True)),
    _single("n_blend", 2, 17, 65, "normal", S1((Q(4), Q(4)), 4, 2, epi="blend")),
    _single("n_last_rgb", 2, 16, 64, "normal", S1((Q(4),), 3, 1, epi="last")),
    _single("n_last_y", 2, 16, 64, "normal", S1((Q(4),), 1, 1, epi="last", y_only=True)),
    _single("n_offmask3", 2, 17, 65, "normal", S1((Q(4),), 3, 1, epi="offmask3", cout_split=2)),
    Case("n_pair_offmask3", "pair", (Stencil((Q(4), Q(4)), 4, act="lrelu"), Stencil((), 3, epi="offmask3", cout_split=2)), 2, 17, 65, "normal",
         kern=("pair<2,offmask3>", "pair<2,offmask3>")),
)
# pair and chain = the composition of their single launches, bit for bit, on ordinary data with lrelu between the stages
COMPOSE = (
    Case("c_pair_k2", "pair", (Stencil((Q(4), Q(4)), 4, act="lrelu"), Stencil((), 4, act="lrelu", residual=True, dst2=True)), 2, 17, 65, "normal",
         kern=("pair<2,plain>", "pair<2,plain>")),
    Case("c_chain_k2_res", "chain", (Stencil((Q(4), Q(4)), 4, act="lrelu"), Stencil((), 4, act="relu"), Stencil((), 4, dst2=True)), 2, 17, 61,
         "normal", res=True, kern=("chain<2,0,res>", "chain<2,0,res>")),
    Case("c_chain_k3_g", "chain", (Stencil((Q(4), Q(4), FLOW), 4, act="lrelu"), Stencil((), 4, act="lrelu"), Stencil((Q(4),), 4, act="lrelu")), 2, 17,
         61, "normal", kern=("chain<3,1,nores>", "chain<3,1,nores>")),
)
# the gated forms of the engines
GATED = (
    ("g_k1_plain", S1((Q(4),), 4, 1, extra="gate", act="lrelu")[0]),
    ("g_k2_plain", S1((Q(3), Q(3)), 4, 2, extra="gate", act="lrelu")[0]),
    ("g_k2_blend", S1((Q(4), Q(4)), 4, 2, epi="blend", extra="gate")[0]),
)
GATE_N, GATE_H, GATE_W = 2, 72, 328          # 5 x 6 tiles, ragged on both axes, w a multiple of 4
GATE_MASKS = {                               # rectangles (item, y0, y1, x0, x1) of set mask pixels
    "corner": ((0, 0, 3, 0, 5), (1, 69, 72, 320, 328)),
    "interior": ((0, 34, 40, 140, 150),),
    "straddle": ((0, 30, 34, 120, 136), (1, 15, 17, 63, 65)),
    "empty": (),
}


# ---------------------------------------------------------------- inputs
def lrelu32(v):
    """max(v, fl32(0.1f v)): the kernels' leaky ReLU on an fp32 value held in float64."""
    return torch.maximum(v, (v * SLOPE).float().double())


def activate(v, act):
    return {"none": v, "relu": v.clamp(min=0), "lrelu": lrelu32(v)}[act]


def make_inputs(case, storage, seed=None, which=None):
    """float32 CPU tensors of every stencil of a case -> list of dicts.  Exact inputs: stage a has its `which` operand fine (fp32 build) and
    the other coarse, later stages coarse x sparse-coarse; bf16 build: everything coarse."""
    rs = np.random.RandomState(sum(map(ord, case.name)) if seed is None else seed)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    n, h, w = case.n, case.h, case.w
    which = which or case.which
    normal = which == "normal"
    out = []
    for k, st in enumerate(case.st):
        cin = st.cin(k > 0)
        if normal:
            gx = lambda shp: rs.randn(*shp)
            gw = lambda shp: rs.randn(*shp) * 1.5 / np.sqrt(9 * cin)
            gb = lambda shp: rs.randn(*shp) * 0.5
        else:
            fx = which == "fine_x" and storage == "f32" and k == 0
            fw = which == "fine_w" and storage == "f32" and k == 0
            gx = (lambda shp: fine(rs, shp)) if fx else (lambda shp: coarse(rs, shp))
            keep = 1.0 if k == 0 else 0.25   # later stages: sparse weights keep S inside the exactness bound
            gw = (lambda shp: fine(rs, shp)) if fw else (lambda shp: coarse(rs, shp) * (rs.rand(*shp) < keep))
            gb = lambda shp: quarters(rs, shp)
        d = {"srcs": [T(gx((n, s[1], h, w) if s[0] == "q4" else (n, h, w, 2))) for s in st.srcs]}
        c1 = st.cout_split if st.cout_split else st.cout
        d["weight"], d["bias"] = T(gw((c1, cin, 3, 3))), T(gb((c1,)))
        if st.cout_split:
            d["weight2"], d["bias2"] = T(gw((st.cout - c1, cin, 3, 3))), T(gb((st.cout - c1,)))
        if st.residual:
            d["residual"] = T(gb((n, 4, h, w)))
        if st.epi == "offmask3":
            d["flow"] = T(gx((n, h, w, 2)) * (4.0 if normal else 1.0))
        if st.epi == "blend":
            d["mask"] = torch.from_numpy((rs.rand(n, 1, h, w) < 0.5).astype(np.uint8))
        if st.epi == "last":   # multiples of 1/4 (exact cases) / [0, 1] data
            d["base_lr"] = T(rs.rand(n, 3, h // 8, w // 8) if normal else rs.randint(0, 5, (n, 3, h // 8, w // 8)) * 0.25)
        out.append(d)
    return out


# ---------------------------------------------------------------- the reference
def bilinear_x8(lr):
    """[n, c, h, w] float64 -> [n, c, 8h, 8w]: PyTorch's align_corners=False source index, the arithmetic of narrow_src_index."""
    def taps(size_out, size_in):
        d = torch.arange(size_out, dtype=torch.float64)
        src = (0.125 * (d + 0.5) - 0.5).clamp(min=0)
        i0 = src.floor().long().clamp(max=size_in - 1)
        i1 = (i0 + 1).clamp(max=size_in - 1)
        l1 = (src - i0).clamp(0, 1)
        return i0, i1, 1 - l1, l1
    n, c, h, w = lr.shape
    y0, y1, ly0, ly1 = taps(8 * h, h)
    x0, x1, lx0, lx1 = taps(8 * w, w)
    top = lr[:, :, y0][:, :, :, x0] * lx0 + lr[:, :, y0][:, :, :, x1] * lx1
    bot = lr[:, :, y1][:, :, :, x0] * lx0 + lr[:, :, y1][:, :, :, x1] * lx1
    return ly0.view(-1, 1) * top + ly1.view(-1, 1) * bot


def luma32(base):
    """0.299f r + 0.587f g + 0.114f b in fp32, the products and the two additions rounded as the kernel rounds them -> float64."""
    b = base.float()
    return ((b[:, 0] * float(LUMA[0]) + b[:, 1] * float(LUMA[1])) + b[:, 2] * float(LUMA[2])).double().unsqueeze(1)


def concat_sources(st, srcs, storage):
    parts = []
    for s, t in zip(st.srcs, srcs):
        if s[0] == "flow2":
            parts.append(t.double().permute(0, 3, 1, 2))
            parts.append(torch.zeros_like(parts[-1]))         # the flow quad is (dx, dy, 0, 0)
        else:
            t = rne_bf16(t) if storage == "bf16" else t.double()
            parts.append(t)
            if s[1] % 4:
                parts.append(torch.zeros(t.shape[0], 4 - s[1] % 4, *t.shape[2:], dtype=torch.float64))
    return torch.cat(parts, dim=1) if parts else None


def expand_weight(st, w, fed):
    """[cout, cin, 3, 3] -> [4, 4 * quads, 3, 3]: every source padded to a whole quad as concat_sources pads it, rows >= cout zero."""
    cols, c = [], 0
    if fed:
        cols.append(w[:, :4]); c = 4
    for s in st.srcs:
        cols.append(w[:, c:c + s[1]]); c += s[1]
        if s[1] % 4:
            cols.append(torch.zeros(w.shape[0], 4 - s[1] % 4, 3, 3, dtype=torch.float64))
    w = torch.cat(cols, dim=1)
    return torch.cat([w, torch.zeros(4 - w.shape[0], *w.shape[1:], dtype=torch.float64)], 0) if w.shape[0] < 4 else w


def stage_reference(st, inp, storage, fed=None, res=None):
    """One stencil in float64 -> dict: out (what dst receives, [n, 4 | 3 | 1, h, w]), out2 (dst2 or None), unrounded (out before the bf16
    build's storage rounding of dst), pre (conv + bias, 4 channels), S (sum |x| |w| + |b|), x (the concatenated input), wq (the expanded weight).  fed: the 4-channel tensor the stage before left; res: the tensor a
    residual chain adds."""
    x = concat_sources(st, inp["srcs"], storage)
    if fed is not None:
        x = fed if x is None else torch.cat([fed, x], 1)
    w, b = inp["weight"].double(), inp["bias"].double()
    if st.cout_split:
        w, b = torch.cat([w, inp["weight2"].double()], 0), torch.cat([b, inp["bias2"].double()], 0)
    if storage == "bf16":
        w = rne_bf16(w)
    wq = expand_weight(st, w, fed is not None)
    b = torch.cat([b, torch.zeros(4 - b.shape[0], dtype=torch.float64)])
    pre, mag = conv3x3_f64(x, wq)
    pre = pre + b.view(1, -1, 1, 1)
    S = mag + b.abs().view(1, -1, 1, 1)
    store = (lambda t: rne_bf16(t)) if storage == "bf16" else (lambda t: t)
    out2 = None
    if st.epi == "plain":
        out = activate(pre, st.act) * st.post_scale
        out[:, st.cout:] = 0
        if st.residual:
            out = out + (rne_bf16(inp["residual"]) if storage == "bf16" else inp["residual"].double())
        if res is not None:
            out = out + res
        unrounded = out
        out = store(out)
        if st.dst2:
            out2 = store(lrelu32(out))
    elif st.epi == "blend":
        unrounded = lrelu32(torch.where(inp["mask"].bool(), pre, x[:, :4]))
        out = store(unrounded)
    elif st.epi == "last":
        base = bilinear_x8(inp["base_lr"].double())
        out = pre[:, :1] + luma32(base) if st.y_only else pre[:, :3] + base
    else:
        fl = inp["flow"].double()
        out = torch.stack([10.0 * torch.tanh(pre[:, 0]) + fl[..., 1], 10.0 * torch.tanh(pre[:, 1]) + fl[..., 0], torch.sigmoid(pre[:, 2]),
                           torch.zeros_like(pre[:, 3])], 1)
    return {"out": out, "out2": out2, "unrounded": unrounded if st.epi in ("plain", "blend") else out, "pre": pre, "S": S, "x": x, "wq": wq}


def reference(case, inputs, storage):
    """-> list of stage_reference dicts, one per stencil; the last one holds the launch's destinations."""
    refs, fed = [], None
    for k, (st, inp) in enumerate(zip(case.st, inputs)):
        last = k == len(case.st) - 1
        refs.append(stage_reference(st, inp, storage, fed=fed, res=refs[0]["out"] if (last and case.res) else None))
        fed = refs[-1]["out"]
    return refs


def _bits(t):
    """smallest i with every element of t a multiple of 2^-i."""
    for i in range(0, 40):
        if bool(((t * 2.0 ** i) == (t * 2.0 ** i).round()).all()):
            return i
    return 99


def exact_ok(case, inputs, refs):
    """The condition on exact inputs under which a correct kernel is exact: at every stage the partial sums, multiples of 2^-(i+j) bounded by
    S (+ what the epilogue adds), are fp32 values: S 2^(i+j) <= 2^24."""
    for st, inp, r in zip(case.st, inputs, refs):
        i, j = _bits(r["x"]), _bits(r["wq"])
        s = r["S"].max().item() * max(st.post_scale, 1.0)
        if st.residual:
            s += 2.0
        if r is refs[-1] and case.res:
            s += refs[0]["out"].abs().max().item()
        if st.epi == "last":
            s += 1.0
        if s * 2.0 ** (i + j + (1 if st.post_scale == 0.5 else 0)) > 2.0 ** 24:
            return False
    return True


@functools.lru_cache(maxsize=None)
def case_data(name, storage, which=None, h=None):
    """(case, inputs, reference) of a named case: computed once, shared by the tests, never modified.  which: "fine_x" / "fine_w" instead of
    the case's own; h: the height of a WALK case."""
    case = {c.name: c for c in EXACT + WALK + NORMAL + COMPOSE}[name]
    if h is not None:
        case = dataclasses.replace(case, h=h)
    inputs = make_inputs(case, storage, which=which)
    return case, inputs, reference(case, inputs, storage)


def probe_specs(case, inputs, dev):
    """The dicts crfp_amd.ops.narrow_probe takes, tensors on `dev`."""
    specs = []
    for st, inp in zip(case.st, inputs):
        spec = {"srcs": [(s[0], t.to(dev)) for s, t in zip(st.srcs, inp["srcs"])], "act": st.act, "post_scale": st.post_scale, "epi": st.epi,
                "y_only": st.y_only, "src_pad": st.src_pad, "dst_pad": st.dst_pad, "dst2": st.dst2, "gate_h": st.gate_h}
        for k in ("weight", "bias", "weight2", "bias2", "residual", "flow", "base_lr", "mask"):
            if k in inp:
                spec[k] = inp[k].to(dev)
        specs.append(spec)
    return specs


def plan_specs(case):
    """The same stencils for crfp_amd.ops.narrow_probe_plan: channel counts in place of tensors."""
    return [{"srcs": [(s[0], s[1]) for s in st.srcs], "cout": st.cout, "cout_split": st.cout_split, "act": st.act, "post_scale": st.post_scale,
             "epi": st.epi, "y_only": st.y_only, "src_pad": st.src_pad, "dst_pad": st.dst_pad, "dst2": st.dst2, "gate_h": st.gate_h} for st in case.st]


# ---------------------------------------------------------------- error bounds on ordinary data
def conv_bound(st, r, storage):
    """|kernel - reference| of conv + bias per element, [n, 4, h, w]: (n_add + 3) 2^-24 S with n_add = 9 * 4 * kq + 1 fp32 additions; bf16
    build: + 2^-16 sum |flow| |w| for what the hi / lo split of a flow quad leaves (two bf16 pieces carry at least 16 bits)."""
    kq = r["x"].shape[1] // 4
    e = (9 * 4 * kq + 1 + 3) * 2.0 ** -24 * r["S"]
    if storage == "bf16":
        c = 0
        for s in st.srcs:
            if s[0] == "flow2":
                fx = torch.zeros_like(r["x"])
                fx[:, c:c + 2] = r["x"][:, c:c + 2]
                e = e + 2.0 ** -16 * conv3x3_f64(fx.abs(), r["wq"].abs())[0]
            c += 4
    return e


# ---------------------------------------------------------------- the mask gate, from its definition (crfp_common.h, launch_mask_gate)
def gate_flags(mask, gate_h):
    """uint8 [n, 1, h, w] -> bool [n, tiles_y, tiles_x]: a tile at most gate_h tiles away (Chebyshev) holds a set mask pixel."""
    m = np.asarray(mask)[:, 0] != 0
    n, h, w = m.shape
    ty, tx = (h + TILE_H - 1) // TILE_H, (w + TILE_W - 1) // TILE_W
    any_ = np.zeros((n, ty, tx), dtype=bool)
    for y in range(ty):
        for x in range(tx):
            any_[:, y, x] = m[:, y * TILE_H:(y + 1) * TILE_H, x * TILE_W:(x + 1) * TILE_W].any(axis=(1, 2))
    out = np.zeros_like(any_)
    for y in range(ty):
        for x in range(tx):
            out[:, y, x] = any_[:, max(y - gate_h, 0):y + gate_h + 1, max(x - gate_h, 0):x + gate_h + 1].any(axis=(1, 2))
    return out


def gate_mask(name):
    m = np.zeros((GATE_N, 1, GATE_H, GATE_W), dtype=np.uint8)
    for i, y0, y1, x0, x1 in GATE_MASKS[name]:
        m[i, 0, y0:y1, x0:x1] = 1
    return torch.from_numpy(m)
