"""GPU (-m gpu): a clip's state-independent per-frame work runs in groups of frames (engine.hip, prework_group / Runner::frame_pre with items) --
the same kernels on the same values, only more items per launch -- so every output bit and every status word must equal the one-frame-per-launch
order, which the lab library keeps behind its own call crfp_lab_prework_groups(0) (no environment name: the helper makes the call when
PREWORK_ORDER=per_frame is set for it).

The cases (tests/helpers/prework_cases.py) run once per library and switch setting, each set in one child process (the library and its switches
are fixed at load time); the tests below compare the recorded digests.  The masks differ frame by frame, the workspaces start as NaN bytes."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB_LIB = os.path.join(ROOT, "crfp_amd", "libcrfp_hip_lab.so")
HELPER = os.path.join(ROOT, "tests", "helpers", "prework_cases.py")

# (lab library?, environment, case-id prefixes or None = all)
RUNS = {
    "product": (False, {}, None),
    "per_frame": (True, {"PREWORK_ORDER": "per_frame"}, None),
    "lab_groups": (True, {}, ["base.dsv", "base.cra", "t.dsv.f32", "t.cra"]),
    "product_dense": (False, {"CRFP_MASK_GATE": "0"}, ["base.dsv", "base.cra", "t.dsv", "t.cra"]),
    "per_frame_dense": (True, {"CRFP_MASK_GATE": "0", "PREWORK_ORDER": "per_frame"}, ["base.dsv", "base.cra", "t.dsv", "t.cra"]),
    "product_side0": (False, {"CRFP_SIDE_STREAM": "0"}, ["base.dsv", "t.dsv", "t.cra"]),
}
_cache = {}


def results(name, tmp_path_factory):
    if name not in _cache:
        lab, env, only = RUNS[name]
        assert os.path.exists(LAB_LIB) or not lab, "lab library not built (make -C crfp_amd/csrc lab)"
        e = dict(os.environ)
        for k in ("PREWORK_ORDER", "CRFP_MASK_GATE", "CRFP_SIDE_STREAM", "CRFP_HIP_LIB"):
            e.pop(k, None)
        e.update(env)
        if lab:
            e["CRFP_HIP_LIB"] = LAB_LIB
        out = str(tmp_path_factory.mktemp("prework") / f"{name}.json")
        r = subprocess.run([sys.executable, HELPER, out] + (["--only", ",".join(only)] if only else []), env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        _cache[name] = json.load(open(out))
    return _cache[name]


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    return results("product", tmp_path_factory)


@pytest.fixture(scope="module")
def per_frame(tmp_path_factory):
    return results("per_frame", tmp_path_factory)


def _same(a, b, what):
    assert a.keys() == b.keys() and a, what
    for cid in a:
        assert a[cid] == b[cid], (what, cid, a[cid], b[cid])


def test_every_wiring_and_storage_equals_the_per_frame_order(product, per_frame):
    """W_DSV (both y_only settings), W_CRA, W_SIMPLE, W_DENSE x fp32 / bf16 storage x LR 20 x 36 and 33 x 47 (ragged tiles), t = 3: outputs and
    status words of the product equal the lab library's one-frame-per-launch order; nothing overflowed, nothing read the NaN prefill."""
    base = {k: v for k, v in product.items() if k.startswith("base.")}
    assert len(base) == 20
    _same(base, {k: v for k, v in per_frame.items() if k.startswith("base.")}, "base")
    for cid, d in base.items():
        assert d["finite"] and d["status"] == [0], cid


def test_frame_counts_around_every_rule_boundary(product, per_frame):
    """LR 8 x 16, n = 1: t = 1, 2, 3, 8 (one full group), 9 (a one-frame tail group), 17 (a third group on the first one's slots); n = 2: t = 3 (whole
    clips as one group) and t = 17 (34 frames: chunked clip-level stages and one frame per launch).  Both storages, W_CRA for the cases that
    reuse the fovea encoder's temporaries; the two-stream and the single-stream schedule, all equal to the per-frame order."""
    pick = lambda r: {k: v for k, v in r.items() if k.startswith(("t.", "t1s."))}
    got = pick(product)
    assert len(got) == 2 * (2 * 8 + 3)
    _same(got, pick(per_frame), "frame counts")
    for cid, d in got.items():
        assert d["finite"] and not any(d["status"]), cid
        if cid.startswith("t1s."):
            assert d == got["t." + cid[4:]], ("single stream", cid)
    # the clips are not degenerate: frames differ from one another, and the empty-mask and the all-mask frame are there
    d = got["t.dsv.f32.n1.t9"]["frames"][0]
    assert len(set(d)) == 9


def test_lab_library_groups_like_the_product(product, tmp_path_factory):
    """The lab library without the switch takes the grouped order too (its bf16 engine is the product's object; the switch lives in the
    once-compiled runtime unit, so both storages follow it)."""
    lab = results("lab_groups", tmp_path_factory)
    _same(lab, {k: product[k] for k in lab}, "lab default")


def test_dense_launches_equal_the_per_frame_order(tmp_path_factory):
    """CRFP_MASK_GATE=0: the same launches without the tile gate (other kernels' early-outs, every tile of every slot written)."""
    a, b = results("product_dense", tmp_path_factory), results("per_frame_dense", tmp_path_factory)
    _same(a, b, "dense")
    assert all(d["finite"] for d in a.values())


def test_dense_and_gated_outputs_are_the_same_bits(product, tmp_path_factory):
    a = results("product_dense", tmp_path_factory)
    _same(a, {k: product[k] for k in a}, "gate off vs on")


def test_side_stream_switch_keeps_the_bits(product, tmp_path_factory):
    """CRFP_SIDE_STREAM=0 (every call on the caller's stream, groups in front of their first frame)."""
    a = results("product_side0", tmp_path_factory)
    _same(a, {k: product[k] for k in a}, "CRFP_SIDE_STREAM=0")


def test_swapped_masks_change_exactly_the_frames_that_read_them(product, per_frame):
    """The check can see a slot mix-up: with the masks of frames 1 and 2 exchanged in the input, frame 0 keeps its bits and frames 1 and 2 do not."""
    base, swap = product["base.dsv.f32.y0.20x36"]["frames"][0], product["swap.dsv.f32"]["frames"][0]
    assert swap[0] == base[0] and swap[1] != base[1] and swap[2] != base[2]
    assert product["swap.dsv.f32"] == per_frame["swap.dsv.f32"]


@pytest.mark.parametrize("wiring", ["dsv", "cra"])
def test_second_call_on_a_used_workspace_equals_a_fresh_one(product, per_frame, wiring):
    """9 frames, then 3 frames on the same workspace: the slots hold the longer clip's frames, and the short clip's result equals a fresh-workspace
    call (and the per-frame order's)."""
    d = product[f"reuse.{wiring}.f32"]
    assert d["finite"] and d["frames"] == d["fresh"]["frames"] and d["status"] == d["fresh"]["status"] == [0]
    assert d == per_frame[f"reuse.{wiring}.f32"]
    if wiring == "dsv":
        assert d["frames"] == product["t.dsv.f32.n1.t3"]["frames"]


def test_overflow_raises_the_word_of_its_own_clip(product, per_frame):
    """n = 2, t = 3, whole clips as one group (item k = clip k / 3): a value >= 65504 in frame 1 of clip 1 raises clip 1's status word and not
    clip 0's -- in the LR frame through the input conversion, in the fovea frame through the grouped launches' own item -> clip mapping."""
    for cid in ("ovf_lr.dsv.f32", "ovf_fv.dsv.f32"):
        d = product[cid]
        assert d["status"] == [0, 1], (cid, d["status"])
        assert d["clip0_finite"], cid
        assert d == per_frame[cid], cid
    assert product["ovf_lr.dsv.f32"]["frames"][0] == product["ovf_fv.dsv.f32"]["frames"][0]     # clip 0 is untouched by either


def test_workspace_one_byte_short_is_refused(product):
    assert product["short.dsv.f32"] == {"n1.t3": -2, "n1.t9": -2, "n2.t3": -2, "n1.t1": -2}


def test_two_calls_in_flight_equal_the_calls_alone(product, per_frame):
    d = product["flight.dsv.f32"]
    assert d["a"] == d["a_alone"] and d["b"] == d["b_alone"] and d["a"] != d["b"]
    assert d == per_frame["flight.dsv.f32"]
    assert d["a_alone"]["frames"] == product["t.dsv.f32.n1.t9"]["frames"]


# crfp_<wiring>_batch_workspace_bytes[_bf16](n, 1, h, w) before the frame slots existed: the one-frame-per-call layout keeps its two sets
T1_BYTES = {
    ("dsv", ""): {(1, 20, 36): 26636544, (1, 33, 47): 57471488, (4, 20, 36): 97627904},
    ("dsv", "_bf16"): {(1, 20, 36): 15366144, (1, 33, 47): 33146112, (4, 20, 36): 56968448},
    ("cra", ""): {(1, 20, 36): 29585664, (1, 33, 47): 63824384, (4, 20, 36): 109424384},
    ("cra", "_bf16"): {(1, 20, 36): 16840704, (1, 33, 47): 36323584, (4, 20, 36): 62866688},
    ("simple", ""): {(1, 20, 36): 27005184, (1, 33, 47): 58265088, (4, 20, 36): 99102464},
    ("simple", "_bf16"): {(1, 20, 36): 15550464, (1, 33, 47): 33542400, (4, 20, 36): 57705728},
    ("dense", ""): {(1, 20, 36): 27005184, (1, 33, 47): 58265088, (4, 20, 36): 99102464},
    ("dense", "_bf16"): {(1, 20, 36): 15550464, (1, 33, 47): 33542400, (4, 20, 36): 57705728},
}


@pytest.mark.parametrize("wiring,sfx", sorted(T1_BYTES))
def test_one_frame_per_call_workspace_keeps_its_size(wiring, sfx):
    from crfp_amd import _lib
    lib = _lib.lib()
    fn = getattr(lib, f"crfp_{wiring}_batch_workspace_bytes{sfx}")
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int] * 4
    for (n, h, w), want in T1_BYTES[(wiring, sfx)].items():
        assert fn(n, 1, h, w) == want, (n, h, w)
    if wiring == "dsv":
        one = getattr(lib, "crfp_dsv_workspace_bytes" + sfx)
        one.restype, one.argtypes = C.c_size_t, [C.c_int] * 3
        assert one(1, 20, 36) == T1_BYTES[(wiring, sfx)][(1, 20, 36)]
        assert one(8, 20, 36) > one(3, 20, 36) > one(2, 20, 36)     # a clip of up to 8 frames holds a slot per frame
        assert one(9, 20, 36) < one(8, 20, 36)                      # a longer one goes in pairs of frames: four slots whatever its length
