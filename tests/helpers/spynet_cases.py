"""Cases for ``crfp_spynet_forward`` (csrc/spynet.hip) and the per-operator SPyNet route: a reference that runs in float64, weight sets that
separate the six pyramid levels without reading any intermediate buffer, frames, and the host's split / direct rule restated.  CPU only;
tests/test_spynet_cases.py checks all of it against the reference alone, tests/test_gpu_spynet.py runs the cases on the GPU.

Levels are numbered as in the state dict: level 0 is the coarsest map (1/32 of the padded frame), level 5 the padded frame itself.

Weight sets (all from ``synth.make_spynet_state_dict(WEIGHT_SEED)``; the last conv of a basic module is j = 4, 16 -> 2 channels):
    plain             the seeded weights
    only<L>           j = 4 weight and bias zero at every level but L: flow_up is exactly 0 up to L, L adds its conv chain on the unwarped
                      frames, every later level adds exactly 0 -- the output is level L's chain, upsampled.  A miss names one map size.
    push:<regime>     push(L, bx, by): j = 4 weight zero at levels <= L, bias zero below L and (bx, by) at L, levels > L as seeded: level L's
                      flow is exactly the constant, i.e. a uniform 2^(5 - L) (bx, by) px motion at the finest level plus the later residuals.

Regimes, by ``clamped_share``: the share of the finest level's warp samples (pixel + flow_up) that lie outside the frame, i.e. whose position the
border clamp changes:  inside = 0,  0.1 < partial < 0.9,  off_frame >= 0.99.  Any uniform motion other than zero moves a whole edge row or column
of samples off the frame, so a share of exactly 0 needs flow_up = 0 at the finest level: `inside` is push(4, 0, 0), the warp at integer positions
with nothing clamped (its x1 = min(x0 + 1, W - 1) corner carries weight 0 in the last column).  PUSHES holds (L, bx, by) per padded shape.
"""
import collections
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BOUND = 1e-4            # the project's stage bound (helpers/dsv_stage_cases.bound_of)
WEIGHT_SEED = 11        # the seed of tests/golden/spynet_small.npz
LEVELS = 6
CHANS = (8, 32, 64, 32, 16, 2)
REGIMES = ("inside", "partial", "off_frame")


def bound_of(flow64):
    return BOUND * max(1.0, float(np.abs(np.asarray(flow64, np.float64)).max()))


def up32(v):
    return v if v % 32 == 0 else 32 * (v // 32 + 1)


def _key(level, j, what):
    return f"basic_module.{level}.basic_module.{j}.conv.{what}"


# ----------------------------------------------------------------------------- the reference
def reference(sd, ref, supp, dtype):
    """SPyNet.forward(ref, supp) as ``oracle.crfp_oracle.spynet`` states it, in ``dtype`` (torch.float64 or torch.float32): weights, mean / std
    and the frames are cast, the warp is ``oracle.flow_warp``.  Returns (flow [n, 2, h, w], taps) with taps[level] = {"flow_up", "warped",
    "flow"} of that level (level 0 coarsest)."""
    import torch
    import torch.nn.functional as F
    from oracle import crfp_oracle as orc
    T = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).to(dtype)   # noqa: E731
    P = {k: T(v) for k, v in sd.items()}
    ref, supp = T(ref), T(supp)
    n, _, h, w = ref.shape
    w_up, h_up = up32(w), up32(h)
    mean, std = P["mean"].view(1, 3, 1, 1), P["std"].view(1, 3, 1, 1)
    pyr = []
    with torch.no_grad():
        for x in (ref, supp):
            x = F.interpolate(x, size=(h_up, w_up), mode="bilinear", align_corners=False)
            levels = [(x - mean) / std]
            for _ in range(5):
                levels.append(F.avg_pool2d(levels[-1], 2, 2, count_include_pad=False))
            pyr.append(levels[::-1])
        flow = ref.new_zeros(n, 2, h_up // 32, w_up // 32)
        taps = []
        for level in range(LEVELS):
            flow_up = flow if level == 0 else F.interpolate(flow, scale_factor=2, mode="bilinear", align_corners=True) * 2.0
            warped = orc.flow_warp(pyr[1][level], flow_up.permute(0, 2, 3, 1), padding_mode="border")
            x = torch.cat([pyr[0][level], warped, flow_up], 1)
            for j in range(5):
                x = F.conv2d(F.relu(x), P[_key(level, j, "weight")], P[_key(level, j, "bias")], stride=1, padding=3)
            flow = flow_up + x
            taps.append({"flow_up": flow_up, "warped": warped, "flow": flow})
        flow = F.interpolate(flow, size=(h, w), mode="bilinear", align_corners=False)
        flow = flow.clone()
        flow[:, 0] *= float(w) / float(w_up)
        flow[:, 1] *= float(h) / float(h_up)
    return flow, taps


def clamped_share(taps):
    """Share of the finest level's warp samples, pixel + flow_up, that lie outside [0, W - 1] x [0, H - 1]: the samples whose position the border
    clamp changes.  From the float64 taps."""
    f = taps[LEVELS - 1]["flow_up"].double().numpy()
    n, _, H, W = f.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx, sy = xx[None] + f[:, 0], yy[None] + f[:, 1]
    out = (sx < 0) | (sx > W - 1) | (sy < 0) | (sy > H - 1)
    return float(out.mean())


def regime_of(share):
    if share == 0.0:
        return "inside"
    if 0.1 < share < 0.9:
        return "partial"
    if share >= 0.99:
        return "off_frame"
    return None


# ----------------------------------------------------------------------------- weight sets
@functools.lru_cache(maxsize=None)
def _seeded():
    from crfp_amd import synth
    return synth.make_spynet_state_dict(WEIGHT_SEED)


def plain():
    return collections.OrderedDict((k, v.copy()) for k, v in _seeded().items())


def only_level(L):
    assert 0 <= L < LEVELS
    sd = plain()
    for level in range(LEVELS):
        if level != L:
            sd[_key(level, 4, "weight")][...] = 0.0
            sd[_key(level, 4, "bias")][...] = 0.0
    return sd


def push(L, bx, by):
    assert 0 <= L < LEVELS
    sd = plain()
    for level in range(L + 1):
        sd[_key(level, 4, "weight")][...] = 0.0
        sd[_key(level, 4, "bias")][...] = (bx, by) if level == L else 0.0
    return sd


# (L, bx, by) per padded shape and regime.  partial: a uniform shift of (sx, sy) px clamps 1 - (1 - |sx| / W)(1 - |sy| / H) of the samples
# (0.2 .. 0.55 for the rows below, before the later levels' residuals); off_frame: +-96 px on frames at most 96 px wide.
_SMALL = {"inside": (4, 0.0, 0.0), "partial": (1, -0.75, 0.5), "off_frame": (0, 3.0, -3.0)}
_LARGE = {"partial": (0, 2.0, -1.5)}
PUSHES = {(32, 64): _SMALL, (32, 32): _SMALL, (64, 64): _SMALL, (64, 96): _SMALL, (192, 320): _LARGE, (128, 256): _LARGE}


def weight_set(name, h, w):
    """The state dict of a weight-set name of CASES at an h x w frame."""
    if name == "plain":
        return plain()
    if name.startswith("only"):
        return only_level(int(name[4:]))
    kind, regime = name.split(":")
    assert kind == "push"
    return push(*PUSHES[(up32(h), up32(w))][regime])


# ----------------------------------------------------------------------------- frames
@functools.lru_cache(maxsize=None)
def frames(kind, n, h, w):
    """(ref, supp) float32 [n, 3, h, w] in [0, 1]: "smooth" = frames 1 and 0 of ``synth.make_clip`` (n different scenes), "noise" = uniform noise."""
    seed = 1000 + 7 * h + w + n
    if kind == "smooth":
        from crfp_amd import synth
        clip = synth.make_clip(seed, n, 2, h, w, fv_size=32)[0]
        ref, supp = clip[:, 1], clip[:, 0]
    else:
        assert kind == "noise"
        rs = np.random.RandomState(seed)
        ref, supp = (rs.uniform(0.0, 1.0, (n, 3, h, w)).astype(np.float32) for _ in range(2))
    ref, supp = np.ascontiguousarray(ref), np.ascontiguousarray(supp)
    ref.setflags(write=False)
    supp.setflags(write=False)
    return ref, supp


# ----------------------------------------------------------------------------- the cases
Case = collections.namedtuple("Case", "h w n kind wset")
Case.id = property(lambda c: f"{c.h}x{c.w}n{c.n}-{c.kind}-{c.wset}")

ALL_SETS = ("plain",) + tuple(f"only{L}" for L in range(LEVELS)) + tuple("push:" + r for r in REGIMES)
LARGE_SETS = ("plain", "only5", "push:partial")
# h, w, n: why
SMALL_SHAPES = (
    (24, 40, 2),     # both axes resized (32 x 64), coarsest level 1 x 2
    (32, 32, 2),     # coarsest level 1 x 1, no resize
    (33, 47, 1),     # odd sizes, resized to 64 x 64
    (64, 96, 2),     # no resize: compute_flow comparable; two different pairs in the batch
)
LARGE_SHAPES = (
    (180, 320, 1, "smooth"),    # padded 192 x 320: cout 16 / 2 go direct at the finest level (every real LR frame)
    (128, 256, 2, "noise"),     # the smallest batch shape that does the same with n = 2: 4 * 32 * 2 = 256 workgroups >= 228
)
KINDS = ("smooth", "noise")
CASES = tuple(Case(h, w, n, kind, s) for h, w, n in SMALL_SHAPES for kind in KINDS for s in ALL_SETS) + \
    tuple(Case(h, w, n, kind, s) for h, w, n, kind in LARGE_SHAPES for s in LARGE_SETS)
# shapes whose branch table does not depend on n (test_spynet_cases asserts it): one n = 2 call == two n = 1 calls, bit for bit
BATCH_SHAPES = ((24, 40), (32, 32), (64, 96))


@functools.lru_cache(maxsize=None)
def case_reference(case, double=True):
    """(flow, taps) of a case, as numpy-backed torch tensors nobody may change; cached per case."""
    import torch
    ref, supp = frames(case.kind, case.n, case.h, case.w)
    return reference(weight_set(case.wset, case.h, case.w), ref, supp, torch.float64 if double else torch.float32)


# ----------------------------------------------------------------------------- the host's branch rule (spy_conv7_mfma, launch_conv_mfma)
ConvRow = collections.namedtuple("ConvRow", "level j H W cin cout ctiles ct2 wgs branch")


def conv_table(n, h, w):
    """One row per 7x7 conv of a crfp_spynet_forward call on n pairs of h x w frames, in launch order.  The host rules restated: the frame is
    padded to multiples of 32 (px pixels); a conv on an H x W map is `split` (ConvArgs::ksplit = 9 plus spy_sum9_kernel) when
    ceil(W / 64) ceil(H / 4) ceil(cout / 32) n 9 <= 2048 and 9 n cout H W <= 9 * 64 * (px / 4) * n, i.e. cout H W <= 16 px, else `direct`;
    an even count of 32-channel cout tiles runs the two-tile kernel (CT2) in either branch."""
    hu, wu = up32(h), up32(w)
    px = hu * wu
    rows = []
    for level in range(LEVELS):
        H, W = hu >> (5 - level), wu >> (5 - level)
        for j in range(5):
            cin, cout = CHANS[j], CHANS[j + 1]
            ctiles = (cout + 31) // 32
            wgs = ((W + 63) // 64) * ((H + 3) // 4) * ctiles * n
            partial_floats = 9 * 64 * (px // 4) * n
            split = wgs * 9 <= 2048 and 9 * n * cout * H * W <= partial_floats
            rows.append(ConvRow(level, j, H, W, cin, cout, ctiles, ctiles % 2 == 0, wgs, "split" if split else "direct"))
    return rows


def conv_branches(n, h, w):
    """{(level, j): "split" | "direct"} for the 30 convs of a call (level 0 coarsest, j = 0..4)."""
    return {(r.level, r.j): r.branch for r in conv_table(n, h, w)}


def launch_counts(n, h, w):
    """(direct, split) launch counts of a call: what the library's profiler reports under `spynet_conv7_mfma` / `spynet_conv7_mfma_ksplit`."""
    b = list(conv_branches(n, h, w).values())
    return b.count("direct"), b.count("split")
