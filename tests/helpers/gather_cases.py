"""Cases, inputs, float64 references and error bounds of the gather probe tests (test_gather_cases.py on the CPU, test_gpu_gather_probe.py on
the GPU): one launch of flow_warp_p4_kernel, flow_warp_p4_dual(_split)_kernel, dcn_g8_pipe_kernel, dcn_fused_kernel<8> (one-tile and
persistent) and dcn3_kernel<false | true> through crfp_gather_probe.  Pure numpy / torch on the CPU; test infrastructure only.

References.  ``motion_cases.warp_ref64`` and ``dcn_ref64`` sample at index + displacement directly in float64; the fused references compose them
with the head in float64: 3x3 conv with zero padding (``conv_cases.conv3x3_f64``), 10 tanh + flow flipped to (y, x) on the offset rows, sigmoid
on the mask rows.  An axis of one pixel is the reference model's own special case: flow_warp scales the normalised coordinate by (size - 1) / 2
= 0, so every sample of that axis lands on pixel 0 whatever the flow says (``warp_ref``).  bf16 build: ``rne_bf16`` where the build stores --
sources, weights (dcn_g8_pack16_kernel rounds to bf16 first, then splits), destination.

Exact inputs (fp32 build: bit for bit; bf16 build: rne_bf16 of the reference).  x and every weight are "coarse" (k / 2, |k| <= 2), flows,
offsets and masks multiples of 1/4, biases multiples of 1/4:
  * coordinates index + offset are multiples of 1/4 far below 2^22: exact in fp32; the warps' normalisation 2 (x + f) / (W - 1) - 1 and back is
    exact when W - 1 and H - 1 are powers of two (divisions and products by powers of two; the sum with 1 keeps a granularity of 2^-(k+3) at
    magnitudes below 2^12): EXACT_WARP_SHAPES;
  * bilinear weights are multiples of 1/16, times a mask 1/64, times x 1/128, four of them: a sampled value is a multiple of 2^-7 with |v| <= 1
    -- 8 bits: an fp32 sum without rounding, and an fp16 head with a zero tail in the split-fp16 GEMM;
  * every product w v is a multiple of 2^-8 and every partial sum is bounded by S = sum |w| |v| + |b|: an fp32 value while S <= 2^11, the
    bound conv_cases holds its exact cases to (``exact_ok`` asks for 2^10; 2^16 would do);
  * fine weights (dcn_g8, "fine_w": coarse + m 2^-12, the low fp16 part of the weight image live): x in {-1, 0, 1}, masks in {0, 1}, offsets
    multiples of 1/2 -- sampled values multiples of 1/4, the head products multiples of 2^-12 and the scaled tail products of 2^-3, the final
    hi + lo 2^-11 a multiple of 2^-14: fp32 values while S <= 2^10 (``exact_ok``);
  * saturated heads: head weights zero, head biases +-200.  tanh10_plus returns f + 10 / f - 10 and fast_sigmoid 1 / 0 exactly there
    (crfp_common.h), so (dy, dx) = +-10 + flow and mask in {0, 1} by the bias signs, and the rest is the argument above.

Ordinary data and the bounds: ``sampler_bound`` / ``fused_bound`` / ``warp_bound`` below; DESIGN.md section 4 has the table."""
import functools

import numpy as np
import torch

from conv_cases import SIGMA_MAX, coarse, conv3x3_f64, fine, quarters, rne_bf16
from helpers import motion_cases as mc

MODES = ("warp", "warp_dual", "dcn_g8", "dcn_fused", "dcn3", "dcn3_fused")
KERNEL = {"warp": "flow_warp_p4", "warp_dual": "flow_warp_p4_dual_split", "dcn_g8": "dcn_g8_pipe", "dcn_fused": "dcn_fused", "dcn3": "dcn3",
          "dcn3_fused": "dcn3_fused"}
# the smallest maps that straddle each kernel's tile (4 rows x 64 px; 4 x 32; 8 x 32; strips of 12 x 64)
SHAPES = {
    "warp": ((1, 1), (3, 5), (4, 64), (5, 65), (9, 130), (17, 33)),
    "warp_dual": ((1, 1), (3, 5), (4, 64), (5, 65), (9, 130), (17, 33)),
    "dcn_g8": ((1, 1), (4, 32), (5, 33), (9, 70), (23, 45)),
    "dcn_fused": ((1, 1), (7, 31), (8, 32), (9, 33), (17, 65), (20, 36)),
    "dcn3": ((1, 1), (11, 63), (12, 64), (13, 65), (25, 130)),
    "dcn3_fused": ((1, 1), (11, 63), (12, 64), (13, 65), (25, 130)),
}
EXACT_WARP_SHAPES = ((17, 33), (5, 65), (3, 5))   # W - 1 and H - 1 powers of two
N = 3
RANGES = (9.0, 64.0, 2058.0)   # batch item b of a case draws its displacements from U(-R, R), R = RANGES[b % 3]
HUGE = 3e9
ROWS = [(m, s) for m in MODES for s in SHAPES[m]]
EXACT_ROWS = [(m, s) for m, s in ROWS if not m.startswith("warp") or s in EXACT_WARP_SHAPES]
DG = {"dcn_g8": 8, "dcn_fused": 8, "dcn3": 1, "dcn3_fused": 1}
T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731


# ---------------------------------------------------------------- displacements
def _plant(d_x, d_y, h, w, gx, gy, shift):
    """Edge targets (motion_cases.edge_targets) on every third pixel of a map too small for planted_flow's 6 x 5 blocks: pixel p gets an x
    target (p % 3 == 0), a y target (1) or both (2), walking the ten targets with p and the batch item; (gx, gy): the tap's own grid displacement."""
    tx, ty = mc.edge_targets(w), mc.edge_targets(h)
    for p in range(h * w):
        y, x = divmod(p, w)
        kind = p % 3
        if kind in (0, 2):
            d_x[..., y, x] = tx[(3 * p + 4 * shift) % 10] - (x + gx)
        if kind in (1, 2):
            d_y[..., y, x] = ty[(7 * p + 4 * shift + 5) % 10] - (y + gy)


def flow_field(seed, n, h, w, exact=False, shift10=False):
    """flow[n, h, w, 2] (dx, dy): item b from ``planted_flow`` with R = RANGES[b % 3] (maps below 6 x 5: the same draws with ``_plant``), a few
    vectors of +-3e9 in the last item.  exact: rounded to multiples of 1/4, which moves the targets 2^-10 beside a border onto it -- so every
    seventh pixel is sent to size - 1/2 (x or y in turn; shift10: through the +-10 a saturated head adds)."""
    out = np.zeros((n, h, w, 2), np.float32)
    for b in range(n):
        R = RANGES[b % 3]
        if h >= 6 and w >= 5:
            out[b] = mc.planted_flow(seed + b, 1, h, w, R)[0]
        else:
            rs = np.random.RandomState(seed + b)
            xs, ys = np.broadcast_to(np.arange(w, dtype=np.float64), (h, w)), np.broadcast_to(np.arange(h, dtype=np.float64).reshape(h, 1), (h, w))
            keep = rs.uniform(0, 1, (h, w)) < 0.45
            dx, dy = mc._draw(rs, R, xs, w, keep), mc._draw(rs, R, ys, h, keep)
            _plant(dx, dy, h, w, 0, 0, b)
            out[b] = np.stack([dx, dy], -1)
    if exact:
        out = np.round(out * 4.0) / 4.0
        for p in range(3, h * w, 7):
            y, x = divmod(p, w)
            ten = (10.0 if (p // 14) % 2 else -10.0) if shift10 else 0.0
            if (p // 7) % 2 == 0:
                out[:, y, x, 0] = w - 0.5 - x - ten
            else:
                out[:, y, x, 1] = h - 0.5 - y - ten
    if h * w >= 4:
        flat = out[n - 1].reshape(h * w, 2)
        flat[1], flat[h * w - 2] = (HUGE, -HUGE), (-HUGE, HUGE)
    return out.astype(np.float32)


def offset_field(seed, n, groups, h, w, exact=False):
    """DCN offsets [n, 2 groups, h, w] (dy, dx per (group, tap)) as ``flow_field``: ``planted_offsets`` where the map allows."""
    out = np.zeros((n, 2 * groups, h, w), np.float32)
    for b in range(n):
        R = RANGES[b % 3]
        if h >= 6 and w >= 5:
            out[b] = mc.planted_offsets(seed + b, 1, groups, h, w, R)[0]
        else:
            rs = np.random.RandomState(seed + b)
            xs, ys = np.broadcast_to(np.arange(w, dtype=np.float64), (h, w)), np.broadcast_to(np.arange(h, dtype=np.float64).reshape(h, 1), (h, w))
            for gk in range(groups):
                k = gk % 9 if groups > 1 else 4
                gy, gx = k // 3 - 1, k % 3 - 1
                keep = rs.uniform(0, 1, (h, w)) < 0.45
                dy, dx = mc._draw(rs, R, ys + gy, h, keep), mc._draw(rs, R, xs + gx, w, keep)
                _plant(dx, dy, h, w, gx, gy, b + gk)
                out[b, 2 * gk], out[b, 2 * gk + 1] = dy, dx
    if exact:
        out = np.round(out * 4.0) / 4.0
    if h * w >= 4:
        flat = out[n - 1].reshape(2 * groups, h * w)
        flat[0::2, 1], flat[1::2, 1], flat[0::2, h * w - 2], flat[1::2, h * w - 2] = HUGE, -HUGE, -HUGE, HUGE
    return out.astype(np.float32)


# ---------------------------------------------------------------- references
def warp_ref(x, flow):
    """``warp_ref64`` with the reference model's one-pixel axes: (size - 1) / 2 = 0 sends every sample of such an axis to pixel 0."""
    flow = np.array(flow, np.float64)
    if x.shape[3] == 1:
        flow[..., 0] = 0.0
    if x.shape[2] == 1:
        flow[..., 1] = 0.0
    return mc.warp_ref64(x, flow)


def head_ref(feat, flow, hw, hb, noff):
    """The offset / mask head in float64 -> (offsets [n, noff, h, w] as (dy, dx) pairs with the flow added flipped, masks, conv bound operand
    S = sum |x| |w| + |b| per row, raw sums)."""
    pre, mag = conv3x3_f64(torch.as_tensor(feat, dtype=torch.float64), torch.as_tensor(hw, dtype=torch.float64))
    b = torch.as_tensor(hb, dtype=torch.float64).view(1, -1, 1, 1)
    pre, S = (pre + b).numpy(), (mag + b.abs()).numpy()
    fl = np.asarray(flow, np.float64)
    off = 10.0 * np.tanh(pre[:, :noff])
    off[:, 0::2] += fl[..., 1][:, None]
    off[:, 1::2] += fl[..., 0][:, None]
    msk = 1.0 / (1.0 + np.exp(-pre[:, noff:]))
    return off, msk, S, pre


def tile9(a):
    return np.tile(a, (1, 9, 1, 1))


def dcn_parts(x, offset, mask, weight, dg):
    """Per output element of a DCN (offset / mask in ops.dcnv2 layout): gain = sum |w| mask (the sum over a group's channels of |w|, times the
    position's mask), wv = sum |w| |bilinear sample| (unmasked), S = sum |w| |masked sample|, and the float64 sample coordinates (py, px)
    [n, dg * 9, h, w]."""
    x, offset, mask, weight = (np.asarray(a, np.float64) for a in (x, offset, mask, weight))
    B, C, H, W = x.shape
    O, cpg = weight.shape[0], C // dg
    k = np.arange(dg * 9) % 9
    py = np.arange(H).reshape(1, 1, H, 1) + (k // 3 - 1).reshape(1, -1, 1, 1) + offset[:, 0::2]
    px = np.arange(W).reshape(1, 1, 1, W) + (k % 3 - 1).reshape(1, -1, 1, 1) + offset[:, 1::2]
    aw = np.abs(weight).reshape(O, dg, cpg, 9)
    gain = np.einsum("oj,bjyx->boyx", aw.sum(2).reshape(O, dg * 9), np.abs(mask))
    wv, S = np.zeros((B, O, H, W)), np.zeros((B, O, H, W))
    for b in range(B):
        for g in range(dg):
            for t in range(9):
                j = g * 9 + t
                v = np.abs(mc._bilinear64(x[b, g * cpg:(g + 1) * cpg], px[b, j], py[b, j], False))
                a = np.einsum("oc,cyx->oyx", aw[:, g, :, t], v)
                wv[b] += a
                S[b] += a * np.abs(mask[b, j])
    return {"gain": gain, "wv": wv, "S": S, "py": py, "px": px}


def dcn_ref64_batched(x, offset, mask, weight, bias, dg):
    """``motion_cases.dcn_ref64`` vectorised over the batch (thousands of small maps: the persistent tile walk); test_gather_cases.py holds the
    two together."""
    x, offset, mask, weight, bias = (np.asarray(a, np.float64) for a in (x, offset, mask, weight, bias))
    B, C, H, W = x.shape
    O, cpg = weight.shape[0], C // dg
    out = np.zeros((B, O, H * W)) + bias.reshape(1, O, 1)
    ys, xs = np.arange(H, dtype=np.float64).reshape(1, H, 1), np.arange(W, dtype=np.float64).reshape(1, 1, W)
    for g in range(dg):
        xg = x[:, g * cpg:(g + 1) * cpg].reshape(B, cpg, H * W)
        for k in range(9):
            j = g * 9 + k
            py, px = ys + (k // 3 - 1) + offset[:, 2 * j], xs + (k % 3 - 1) + offset[:, 2 * j + 1]
            y0, x0 = np.floor(py), np.floor(px)
            ly, lx = py - y0, px - x0
            val = np.zeros((B, cpg, H * W))
            for dy, dx, wt in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
                yy, xx = y0 + dy, x0 + dx
                ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                idx = (np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)).astype(np.int64).reshape(B, 1, H * W)
                val += np.take_along_axis(xg, np.broadcast_to(idx, (B, cpg, H * W)), 2) * (wt * ok).reshape(B, 1, H * W)
            out += np.einsum("oc,bcp->bop", weight[:, g * cpg:(g + 1) * cpg, k // 3, k % 3], val * mask[:, j].reshape(B, 1, H * W))
    return out.reshape(B, O, H, W)


def coord_term(x, py, px):
    """1/2 ulp32(max in-frame |coordinate|) * max |adjacent-pixel difference| (motion_cases.coord_rounding_term), per batch item."""
    return np.array([mc.coord_rounding_term(x[b:b + 1], px[b], py[b])[0] for b in range(x.shape[0])]).reshape(-1, 1, 1, 1)


N_GEMM = 9 * 32 + 3


def sampler_bound(x, parts, bias, split, n_add=N_GEMM):
    """A DCN launch on given offsets and masks: the fp32 coordinate sum moves a sample by at most half an ulp of the coordinate, i.e. the result
    by 1/2 ulp32(max in-frame |coord|) max |adjacent difference| sum |w mask|; the split-fp16 GEMM drops less than 2^-22 of every product and
    accumulates n = 9 * 32 + 3 terms in fp32: (2^-22 + n 2^-24) S, S = sum |w| |sample| + |b|.  split = False (the bf16 build's one MFMA product;
    dcn3_kernel's fp32 MFMAs, n = 9 * 4 + 3): n 2^-24 S."""
    S = parts["S"] + np.abs(np.asarray(bias, np.float64)).reshape(1, -1, 1, 1)
    return coord_term(x, parts["py"], parts["px"]) * parts["gain"] + ((2.0 ** -22 if split else 0.0) + n_add * 2.0 ** -24) * S


def fused_bound(x, parts, bias, split, S_head, noff, n_head, n_add=N_GEMM):
    """The sampler's bound plus what the head's own error does: e_h = (2^-22 + n 2^-24) S_head (bf16: n 2^-24 S_head) per head row enters as
    (3e-6 + 10 e_h) max |adjacent difference| sum |w mask| through the coordinates and as (3e-7 + e_h / 4) sum |w bilinear| through the mask
    (the activation constants of the offset / mask row of the conv table).  e_h: the largest over the rows of a pixel."""
    e_h = ((2.0 ** -22 if split else 0.0) + n_head * 2.0 ** -24) * S_head
    e_off, e_m = e_h[:, :noff].max(1, keepdims=True), e_h[:, noff:].max(1, keepdims=True)
    adj = np.array([mc.max_adjacent_diff(x[b:b + 1]) for b in range(x.shape[0])]).reshape(-1, 1, 1, 1)
    return sampler_bound(x, parts, bias, split, n_add) + (3e-6 + 10.0 * e_off) * adj * parts["gain"] + (3e-7 + e_m / 4.0) * parts["wv"]


def warp_bound(x, flow):
    """The P4 warps restate the reference's normalisation in fp32: x + f, 2 (.) / (W - 1), - 1, + 1, (.) (W - 1) / 2 -- five roundings, each at
    most 2^-24 of an intermediate that is, in pixels, at most |coordinate| + size for a sample in the frame: the coordinate moves by at most
    5 2^-24 (c + size) on each axis, c = max in-frame |coordinate|, the interpolant by (max |adjacent difference|) per pixel and axis.  The
    blend's four weights (two roundings each), four products and three sums add 8 2^-24 max |x|.  Per batch item."""
    x, flow = np.asarray(x, np.float64), np.asarray(flow, np.float64)
    n, _, h, w = x.shape
    out = np.zeros((n, 1, 1, 1))
    for b in range(n):
        px = np.arange(w).reshape(1, w) + (flow[b, ..., 0] if w > 1 else np.zeros((h, w)))
        py = np.arange(h).reshape(h, 1) + (flow[b, ..., 1] if h > 1 else np.zeros((h, w)))
        inside = (px > -1) & (px < w) & (py > -1) & (py < h)
        c = float(max(np.abs(px[inside]).max(), np.abs(py[inside]).max())) if inside.any() else 0.0
        out[b] = 2.0 * 5.0 * 2.0 ** -24 * (c + max(h, w)) * mc.max_adjacent_diff(x[b:b + 1]) + 8.0 * 2.0 ** -24 * np.abs(x[b]).max()
    return out


# ---------------------------------------------------------------- saturated heads
def sign_codes():
    """72 distinct 9-bit codes, one per (group, tap): bits (3 t, 3 t + 1, 3 t + 2) = the signs of (dy, dx, mask) in sign table t; every code has
    its mask on in at least one table, so that no position is silent in all three."""
    codes = [c for c in range(512) if c & 0b100100100][::6][:72]
    assert len(set(codes)) == 72
    return codes


def saturated_bias(mode, table):
    """Head biases of +-200: dcn_fused [216] by ``sign_codes`` and the table 0 .. 2; dcn3_fused [3]: tables 0 .. 3 = the four (dy, dx) sign
    pairs with the mask on, table 4 = the mask off."""
    if mode == "dcn3_fused":
        sy, sx, sm = ((1, 1, 1), (1, -1, 1), (-1, 1, 1), (-1, -1, 1), (1, -1, -1))[table]
        return np.array([sy, sx, sm], np.float32) * 200.0
    b = np.zeros(216, np.float32)
    for P, c in enumerate(sign_codes()):
        bits = (c >> (3 * table)) & 7
        b[2 * P], b[2 * P + 1], b[144 + P] = (200.0 if bits & 1 else -200.0), (200.0 if bits & 2 else -200.0), (200.0 if bits & 4 else -200.0)
    return b


SAT_TABLES = {"dcn_fused": (0, 1, 2), "dcn3_fused": (0, 1, 2, 3, 4)}


# ---------------------------------------------------------------- cases
def _seed(mode, h, w):
    return 1000 * MODES.index(mode) + 31 * h + w


def _rb(a):
    return rne_bf16(torch.as_tensor(np.asarray(a, np.float32))).numpy()


def _seen(d, storage, keys):
    """The inputs as the build stores them."""
    return {k: (_rb(v) if storage == "bf16" and k in keys and v is not None else (None if v is None else np.asarray(v, np.float64))) for k, v in d.items()}


def make_inputs(mode, h, w, which, n=N, table=0, head_scale=1.0, seed=None):
    """float32 numpy inputs of one launch.  which: "exact" (see the module text; the fused modes: a saturated head, sign table `table`) or
    "normal" (standard-normal x, DCN weights * 1.5 / sqrt(9 cin), head weights the same times head_scale: raw sums ~ N(0, 1.5 head_scale))."""
    rs = np.random.RandomState(_seed(mode, h, w) if seed is None else seed)
    fw = which == "fine_w"
    assert not fw or mode == "dcn_g8"
    ex = which == "exact" or fw
    gx = (lambda s: rs.randint(-1, 2, s) * 1.0) if fw else (lambda s: coarse(rs, s)) if ex else (lambda s: rs.standard_normal(s))
    gw = (lambda s: fine(rs, s)) if fw else (lambda s: coarse(rs, s)) if ex else (lambda s: rs.standard_normal(s) * 1.5 / np.sqrt(9 * s[1]))
    gb = (lambda s: quarters(rs, s)) if ex else (lambda s: rs.standard_normal(s) * 0.5)
    d = {"x2": None, "aux": None, "mask": None, "flow": None, "head_w": None, "head_b": None, "weight": None, "bias": None}
    sd = rs.randint(1 << 30)
    if mode in ("warp", "warp_dual"):
        d["x"] = gx((n, 32, h, w))
        d["x2"] = gx((n, 24, h, w)) if mode == "warp_dual" else None
        d["flow"] = flow_field(sd, n, h, w, ex)
    else:
        c = 32 if DG[mode] == 8 else 4
        d["x"], d["weight"], d["bias"] = gx((n, c, h, w)), gw((c, c, 3, 3)), gb((c,))
        groups = 72 if c == 32 else 1
        if mode in ("dcn_g8", "dcn3"):
            off = offset_field(sd, n, groups, h, w, ex)
            msk = rs.randint(0, 5, (n, groups, h, w)) * 0.25 if ex else rs.uniform(0, 1, (n, groups, h, w))
            if fw:
                off, msk = np.round(off * 2.0) / 2.0, rs.randint(0, 2, (n, groups, h, w)) * 1.0
            d["aux"], d["mask"] = (off, msk) if mode == "dcn_g8" else (np.concatenate([off, msk], 1), None)
        else:
            d["aux"], d["flow"] = gx((n, c, h, w)), flow_field(sd, n, h, w, ex, ex)
            rows = 3 * groups
            if ex:
                d["head_w"], d["head_b"] = np.zeros((rows, c, 3, 3)), saturated_bias(mode, table)
            else:
                d["head_w"], d["head_b"] = gw((rows, c, 3, 3)) * head_scale, gb((rows,))
    return {k: (None if v is None else np.ascontiguousarray(v, dtype=np.float32)) for k, v in d.items()}


def reference(mode, inp, storage):
    """-> dict: out (float64, bf16 build: before the destination's rounding), out2, and for the DCN modes parts (``dcn_parts``), off / msk
    (ops.dcnv2 layout), S_head / pre (fused modes)."""
    s = _seen(inp, storage, ("x", "x2", "weight", "head_w") + (("aux",) if mode.endswith("fused") else ()))
    if mode in ("warp", "warp_dual"):
        return {"out": warp_ref(s["x"], s["flow"]), "out2": warp_ref(s["x2"], s["flow"]) if mode == "warp_dual" else None}
    dg = DG[mode]
    r = {"out2": None}
    if mode == "dcn_g8":
        off, msk = s["aux"], s["mask"]
    elif mode == "dcn3":
        off, msk = tile9(s["aux"][:, :2]), tile9(s["aux"][:, 2:3])
    else:
        noff = 144 if dg == 8 else 2
        o, m, r["S_head"], r["pre"] = head_ref(s["aux"], s["flow"], s["head_w"], s["head_b"], noff)
        off, msk = (o, m) if dg == 8 else (tile9(o), tile9(m))
    r["off"], r["msk"] = off, msk
    r["out"] = mc.dcn_ref64(s["x"], off, msk, s["weight"], s["bias"], dg)
    r["parts"] = dcn_parts(s["x"], off, msk, s["weight"], dg)
    r["x"] = s["x"]
    return r


def bound(mode, inp, ref, storage):
    """The error bound of an ordinary-data case per output element, before the bf16 destination's 2^-8 |ref|."""
    if mode in ("warp", "warp_dual"):
        return warp_bound(ref_x(inp, storage, "x"), inp["flow"]), (warp_bound(ref_x(inp, storage, "x2"), inp["flow"]) if mode == "warp_dual" else None)
    dg = DG[mode]
    # the 4 -> 4 mix and the 4 -> 3 head of dcn3_kernel run on fp32 MFMAs (no split, n = 9 * 4 + 3): their terms are the accumulation's alone
    split, n_add = dg == 8 and storage == "f32", N_GEMM if dg == 8 else 9 * 4 + 3
    if mode in ("dcn_g8", "dcn3"):
        return sampler_bound(ref["x"], ref["parts"], inp["bias"], split, n_add), None
    return fused_bound(ref["x"], ref["parts"], inp["bias"], split, ref["S_head"], 144 if dg == 8 else 2, n_add, n_add), None


def ref_x(inp, storage, key):
    return _rb(inp[key]) if storage == "bf16" else np.asarray(inp[key], np.float64)


def expected(ref_out, storage):
    """What a destination holds: the reference, through the bf16 store in the bf16 build."""
    t = torch.as_tensor(ref_out)
    return (rne_bf16(t) if storage == "bf16" else t).float()


def exact_ok(mode, ref):
    """The power-of-two condition of the exact DCN cases: every partial sum of the GEMM an fp32 value (S + |b| <= 2^10: what the fine-weight
    case needs, half of conv_cases.SIGMA_MAX; the coarse cases would do with 2^16)."""
    if mode in ("warp", "warp_dual"):
        return True
    return float(ref["parts"]["S"].max()) + 2.0 <= SIGMA_MAX / 2.0


@functools.lru_cache(maxsize=None)
def case(mode, h, w, which, storage, table=0, head_scale=1.0, n=N):
    """(inputs, reference) of one case: computed once, shared by the tests, never modified."""
    inp = make_inputs(mode, h, w, which, n, table, head_scale)
    return inp, reference(mode, inp, storage)


# ---------------------------------------------------------------- conditions on the inputs
def coords(mode, inp, ref):
    """Float64 sample coordinates (py, px) of a case, every tap of every position."""
    if mode in ("warp", "warp_dual"):
        n, _, h, w = inp["x"].shape
        fl = inp["flow"].astype(np.float64)
        return np.arange(h).reshape(1, h, 1) + fl[..., 1], np.arange(w).reshape(1, 1, w) + fl[..., 0]
    return ref["parts"]["py"], ref["parts"]["px"]


def coverage(p, size):
    """Which regions of an axis the samples p reach: inside, in (-1, 0), in (size - 1, size), clamped below, clamped above."""
    return {"inside": bool(((p >= 0) & (p <= size - 1)).any()), "low_edge": bool(((p > -1) & (p < 0)).any()),
            "high_edge": bool(((p > size - 1) & (p < size)).any()), "below": bool((p <= -1).any()), "above": bool((p >= size).any())}


def regular_share(off, h, w):
    """dcn3_kernel's branch: share of the 64-pixel wave rows whose lanes are all `regular` (the integer parts of the three clamped tap
    coordinates advance by one per tap, on both axes).  off [n, 2, h, w] = the shared (dy, dx)."""
    off = np.asarray(off, np.float64)
    n = off.shape[0]
    iy = [np.floor(np.clip(np.arange(h).reshape(1, h, 1) - 1 + q + off[:, 0], -1, h)) for q in range(3)]
    ix = [np.floor(np.clip(np.arange(w).reshape(1, 1, w) - 1 + q + off[:, 1], -1, w)) for q in range(3)]
    reg = (iy[1] == iy[0] + 1) & (iy[2] == iy[0] + 2) & (ix[1] == ix[0] + 1) & (ix[2] == ix[0] + 2)
    rows = [reg[b, y, x0:x0 + 64].all() for b in range(n) for y in range(h) for x0 in range(0, w, 64)]
    return float(np.mean(rows))


def branch_inputs(mode, h, w, mixed, n=N):
    """dcn3 / dcn3_fused on ordinary data with a displacement field that steers dcn3_kernel's branch: offsets of 0.5 +- 0.3 everywhere keep
    every lane regular (share 1.0); mixed: the wave rows with (y + x block) odd keep the planted field of ``make_inputs``."""
    inp = make_inputs(mode, h, w, "normal", n, head_scale=0.001)
    rs = np.random.RandomState(h + w)
    smooth = (0.5 + rs.uniform(-0.25, 0.25, (n, 2, h, w))).astype(np.float32)
    take = np.ones((n, 1, h, w), bool)
    if mixed:
        take[:] = ((np.arange(h).reshape(h, 1) + np.arange(w).reshape(1, w) // 64) % 2 == 0)[None, None]
    if mode == "dcn3":
        inp["aux"][:, :2] = np.where(take, smooth, inp["aux"][:, :2])
    else:   # a head without bias adds 10 tanh(~N(0, 0.0015)) to the flow: within +-0.1 of it
        inp["head_b"][:] = 0.0
        fl = np.moveaxis(inp["flow"], 3, 1)
        inp["flow"] = np.ascontiguousarray(np.moveaxis(np.where(take, smooth, fl), 1, 3))
    return inp


BRANCH_SHAPE = (25, 130)


# ---------------------------------------------------------------- the fp32 restatement (the cap on the reference)
def restate32(mode, inp, storage):
    """The same launch restated in fp32 on the CPU: oracle.flow_warp / oracle.dcnv2, the fused modes behind an fp32 head (F.conv2d, 10 tanh +
    flow, sigmoid), on the inputs as the build stores them.  -> (out, out2) float64."""
    from oracle import crfp_oracle as orc
    keys = ("x", "x2", "weight", "head_w") + (("aux",) if mode.endswith("fused") else ())
    s = {k: (None if v is None else (torch.as_tensor(_rb(v)).float() if storage == "bf16" and k in keys else T(v))) for k, v in inp.items()}
    if mode in ("warp", "warp_dual"):
        return orc.flow_warp(s["x"], s["flow"]).double().numpy(), (orc.flow_warp(s["x2"], s["flow"]).double().numpy() if mode == "warp_dual" else None)
    dg = DG[mode]
    if mode == "dcn_g8":
        off, msk = s["aux"], s["mask"]
    elif mode == "dcn3":
        off, msk = s["aux"][:, :2].repeat(1, 9, 1, 1), s["aux"][:, 2:3].repeat(1, 9, 1, 1)
    else:
        noff = 144 if dg == 8 else 2
        pre = torch.nn.functional.conv2d(s["aux"], s["head_w"], s["head_b"], padding=1)
        off = 10.0 * torch.tanh(pre[:, :noff])
        off[:, 0::2] += s["flow"][..., 1].unsqueeze(1)
        off[:, 1::2] += s["flow"][..., 0].unsqueeze(1)
        msk = torch.sigmoid(pre[:, noff:])
        if dg == 1:
            off, msk = off.repeat(1, 9, 1, 1), msk.repeat(1, 9, 1, 1)
    return orc.dcnv2(s["x"], off.contiguous(), msk.contiguous(), s["weight"], s["bias"], dg).double().numpy(), None
