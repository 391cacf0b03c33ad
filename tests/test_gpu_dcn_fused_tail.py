"""GPU (-m gpu): the 8x state warp in the idle last round of the fused offset head + DCN launches (crfp_amd/csrc/dcn_fused.inc, DcnWarpPlan).

The one-tile form of dcn_fused_kernel<8> pays its last round of the chip in full although only `tiles % CUs` CUs have a tile in it.  The
workgroups behind the launch's tiles, one per idle CU, carry a row band of flow_warp_p4_kernel's work (state_hr, flow8 -> prevhrw) with that
kernel's own per-pixel program (gather.hip flow_warp_p4_pixels), so every bit of both outputs must equal the stand-alone launches.

Operator level: crfp_dcn_tail_probe (include/crfp_hip.h) against itself with bands = 0 (the fused launch, then the stand-alone warp).  Engine
level: the product against the lab library after crfp_lab_warp_tail_bands(0), one child process per library (tests/helpers/dcn_tail_cases.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB_LIB = os.path.join(ROOT, "crfp_amd", "libcrfp_hip_lab.so")
HELPER = os.path.join(ROOT, "tests", "helpers", "dcn_tail_cases.py")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# 2x maps (n, h, w): fewer tiles than CUs -- every warp workgroup starts at once; ragged in both directions; 272 tiles on 256 CUs -- one short
# round, the warp workgroups wait for a tile round; N = 2 with every tensor on its own batch stride
SHAPES = [(1, 20, 36), (1, 33, 47), (1, 128, 544), (2, 33, 47)]
_cases = {}


def op_case(storage, n, h, w):
    """The buffers of a geometry and its bands = 0 reference run, built once and shared by the band counts."""
    from tests.helpers import dcn_tail_cases as tc
    key = (storage, n, h, w)
    if key not in _cases:
        c = tc.OpCase(storage, n, h, w)
        _cases[key] = (c, c.run(0))
    return _cases[key]


def check_outputs(c, ref, got):
    """out, dst and the status words of `got` equal `ref` byte for byte (gaps between batch items and guard bytes included); the guards are
    intact, every owned element was written over its 0xFF prefill, the gaps were not."""
    import torch
    from tests.helpers import dcn_tail_cases as tc
    (_, out0, dst0, st0), (_, out, dst, st) = ref, got
    assert torch.equal(out, out0), "DCN output differs from the launch without a plan"
    assert torch.equal(dst, dst0), "warped state differs from the stand-alone warp"
    assert torch.equal(st, st0)
    for buf, stride, count in ((out, c.out_b, 32 * c.h * c.w), (dst, c.dst_b, 64 * c.h * c.w)):
        assert bool((buf[-tc.GUARD:] == tc.GUARD_BYTE).all()), "guard bytes behind an output were written"
        own = c.written(buf[:-tc.GUARD], stride, count)
        body = buf[:-tc.GUARD]
        assert bool((body[~own] == 0xFF).all()), "bytes between batch items were written"
        el = body[own].view(torch.int16 if c.esz == 2 else torch.int32)
        assert bool((el != -1).all()), "an element of an output kept its 0xFF prefill"
        vals = body[own].view(torch.bfloat16 if c.esz == 2 else torch.float32)
        assert bool(torch.isfinite(vals.float()).all())


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("n,h,w", SHAPES)
@pytest.mark.parametrize("bands", [1, 2, 3])
def test_fused_launch_with_warp_bands_equals_the_stand_alone_launches(storage, n, h, w, bands):
    """k fused launches, launch b carrying band b of k of the 4h x 4w warp (flow of +-9 px and a few vectors far outside the image, the
    destination prefilled with 0xFF bytes): the union of the bands is the one-launch warp, the DCN output is the launch's without a plan."""
    c, ref = op_case(storage, n, h, w)
    got = c.run(bands)
    r0, r = ref[0], got[0]
    tiles = n * ((w + 31) // 32) * ((h + 7) // 8)
    assert r0["plan_taken"] == 0 and r0["grid"] == tiles and r0["tiles"] == tiles
    assert r["plan_taken"] == 1 and r["persistent"] == 0 and r["warp_wgs"] == r["cus"] - tiles % r["cus"] and r["grid"] == tiles + r["warp_wgs"]
    check_outputs(c, ref, got)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_a_full_last_round_refuses_the_plan(storage):
    """64 x 256 with N = 4 is 256 tiles: where the device's CU count divides them (an MI355X: 256) no CU is idle in the last round, the plan is
    refused and the stand-alone path taken whole.  On another CU count the launch has a tail and carries the plan like the cases above."""
    c, ref = op_case(storage, 4, 64, 256)
    got = c.run(3)
    r = got[0]
    assert r["tiles"] == 256 and r["persistent"] == 0
    idle = r["cus"] - 256 % r["cus"] if 256 % r["cus"] else 0
    assert r["warp_wgs"] == idle and r["plan_taken"] == (1 if idle else 0) and r["grid"] == 256 + idle
    check_outputs(c, ref, got)


# ---------------------------------------------------------------- engine level
_runs = {}


def engine_results(name, tmp_path_factory):
    if name not in _runs:
        e = dict(os.environ)
        for k in ("CRFP_HIP_LIB", "WARP_TAIL_BANDS", "CRFP_DCN_FUSED"):
            e.pop(k, None)
        if name == "product_fused0":
            e["CRFP_DCN_FUSED"] = "0"
        elif name != "product":
            assert os.path.exists(LAB_LIB), "lab library not built (make -C crfp_amd/csrc lab)"
            e["CRFP_HIP_LIB"] = LAB_LIB
            e["WARP_TAIL_BANDS"] = name[len("lab_bands"):]
        out = str(tmp_path_factory.mktemp("dcn_tail") / f"{name}.json")
        r = subprocess.run([sys.executable, HELPER, out], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        _runs[name] = json.load(open(out))
    return _runs[name]


def test_engines_equal_the_stand_alone_warp_schedule(tmp_path_factory):
    """CRFP_DSV and CRFP_DSV_CRA, fp32 and bf16 storage: 3-frame clips at 20 x 36 and 33 x 47 LR (output frames, status word, debug_fetch of
    prevhrw, aligned and state_hr), a lock-step batch of 2 and three streamed frames.  The product (three bands) equals, bit for bit,
      * the lab library with the knob off (crfp_lab_warp_tail_bands(0): the stand-alone launch) (the switch lives in the once-compiled runtime unit, so the lab
        library's product-built bf16 engine follows it too);
      * the product under CRFP_DCN_FUSED=0, the two-kernel path, which takes no plan and is bit-identical to the fused launch in both builds
        (tests/test_gpu_parity.py, tests/test_gpu_bf16.py): a second stand-alone reference, from the product library itself."""
    a = engine_results("product", tmp_path_factory)
    assert len(a) == 2 * 2 * (2 + 1 + 1)
    for other in ("lab_bands0", "product_fused0"):
        b = engine_results(other, tmp_path_factory)
        assert a.keys() == b.keys()
        for cid in a:
            assert a[cid] == b[cid], (other, cid, a[cid], b[cid])
    for cid, d in a.items():
        assert not any(d["status"]), cid
        assert d.get("finite", True), cid
    assert len(set(a["clip.dsv.f32.20x36"]["frames"])) == 3
