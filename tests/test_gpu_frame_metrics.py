"""GPU (-m gpu): the fused frame metrics table (crfp_frame_metrics_f32 through crfp_amd.utils.frame_metrics_table, evalrig.eval_clip(fused=)
and gaze.run_gaze_video(fused_metrics=)) against tests/golden/ops_small.npz and the float64 yardstick tests/frame_metrics_ref.py.

Parity follows the project's rule: per figure max(1e-4 dB or 2e-6 SSIM, 4 x |fp32 oracle - float64 yardstick|) on that case,
the second term computed here from the two CPU evaluations.  Every comparison prints the measured distance and its bound (the table of
DESIGN 3.5; the worst case is SSIM-Y of unconverted luma near 125: 1.6e-3 against a bound of 1.3e-2)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frame_metrics_ref as fref

pytestmark = pytest.mark.gpu

T = torch.from_numpy
PSNR_TOL, SSIM_TOL = 1e-4, 2e-6
COLS = ("psnr", "ssim", "psnr_y", "ssim_y")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def orc():
    from oracle import crfp_oracle
    return crfp_oracle


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def ragged(orc):
    """The n = 5 batch with its yardstick, oracle and GPU tables, computed once."""
    from crfp_amd import utils as U
    sr, hr, masks = fref.ragged_case()
    yard, ora = fref.table(sr, hr, masks, luma_on=True), fref.oracle_table(orc, sr, hr, masks, luma_on=True)
    d_sr, d_hr, d_m = sr.to(dev()), hr.to(dev()), masks.to(dev())
    got = U.frame_metrics_table(d_sr, d_hr, d_m, luma=True)
    return dict(sr=sr, hr=hr, masks=masks, yard=yard, ora=ora, d_sr=d_sr, d_hr=d_hr, d_m=d_m, got=got)


def check(name, got, yard, ora):
    """Every (frame, region, column) under the rule; prints the worst distance per frame and column with its bound."""
    got = got.cpu()
    assert got.shape == yard.shape and got.dtype == torch.float64
    assert torch.equal(torch.isnan(got), torch.isnan(yard)), f"{name}: NaN pattern differs"
    bound = fref.bounds(yard, ora)
    dist = torch.nan_to_num((got - yard).abs(), nan=0.0)
    bad = []
    for i in range(got.shape[0]):
        for col in range(4):
            k = int(torch.argmax(dist[i, :, col] / bound[i, :, col]))
            print(f"{name} frame {i} {COLS[col]:7s}: |gpu - yardstick| {float(dist[i, k, col]):.3e}  bound {float(bound[i, k, col]):.3e}  (region {k})")
            if bool((dist[i, :, col] >= bound[i, :, col]).any()):
                bad.append((i, col, float(dist[i, k, col]), float(bound[i, k, col])))
    assert not bad, f"{name}: (frame, column, distance, bound) {bad}"


def test_golden_rows_and_luma_in_one_call(ops_golden):
    from crfp_amd import utils as U
    g = ops_golden
    sr, hr = T(g["metric_sr"]).to(dev()), T(g["metric_hr"]).to(dev())
    t = U.frame_metrics_table(sr, hr, [T(g["metric_box"]).to(dev()), T(g["metric_ring"]).to(dev())], luma=True).cpu()
    assert t.shape == (1, 3, 4)
    for row, tag in enumerate(("", "_box", "_ring")):
        dp, ds = abs(float(t[0, row, 0]) - float(g["metric_psnr" + tag])), abs(float(t[0, row, 1]) - float(g["metric_ssim" + tag]))
        print(f"golden{tag or '_whole'}: psnr {dp:.3e} (1e-4)  ssim {ds:.3e} (2e-6)")
        assert dp < PSNR_TOL and ds < SSIM_TOL, tag
    dp, ds = abs(float(t[0, 0, 2]) - float(g["metric_psnr_y"])), abs(float(t[0, 0, 3]) - float(g["metric_ssim_y"]))
    print(f"golden_y: psnr {dp:.3e} (1e-4)  ssim {ds:.3e} (2e-6)")
    assert dp < PSNR_TOL and ds < SSIM_TOL


def test_ragged_batch_every_branch_and_region(ragged):
    hr = ragged["hr"]
    span = [float(hr[i].max() - hr[i].min()) for i in range(5)]
    yspan = [float(fref.luma(hr[i:i + 1]).max() - fref.luma(hr[i:i + 1]).min()) for i in range(5)]
    assert span[0] <= 0.9 and span[1] >= 2.2 and 1.1 <= span[2] <= 1.8                   # the three RGB branches
    assert min(yspan[:3]) >= 2.2 and yspan[3] <= 0.9 and 1.1 <= yspan[4] <= 1.8           # the three luma branches
    check("ragged", ragged["got"], ragged["yard"], ragged["ora"])


def test_small_and_odd_shapes(orc):
    from crfp_amd import utils as U
    shapes = []
    for name, sr, hr in fref.small_cases():
        luma = sr.shape[1] == 3
        got = U.frame_metrics_table(sr.to(dev()), hr.to(dev()), None, luma=luma)
        if not luma:
            assert torch.isnan(got[0, 0, 2:]).all() and not torch.isnan(got[0, 0, :2]).any()
        check(name, got, fref.table(sr, hr, None, luma), fref.oracle_table(orc, sr, hr, None, luma))
        shapes.append(tuple(sr.shape[1:]))
    assert shapes == [(1, 7, 9), (3, 16, 64), (3, 17, 65)]


def test_identical_images_floor_value_and_ssim_one(ragged):
    from crfp_amd import utils as U
    for i in (0, 1, 3):     # no conversion, /255, unconverted luma
        a = ragged["d_hr"][i:i + 1]
        t = U.frame_metrics_table(a, a.clone(), ragged["d_m"][i:i + 1], luma=True).cpu()[0]
        assert abs(float(t[0, 0]) - -20 * math.log10(math.sqrt((1 / 255.0) ** 2 / (3 * 70 * 150)))) < 1e-9
        assert abs(float(t[0, 2]) - -20 * math.log10(math.sqrt((1 / 255.0) ** 2 / (70 * 150)))) < 1e-9
        assert torch.equal(t[:, 0], t[0, 0].expand(4)) and torch.equal(t[:, 2], t[0, 2].expand(4))    # numel is the frame's in every region
        assert torch.equal(t[:, 1], torch.ones(4, dtype=torch.float64)) and torch.equal(t[:, 3], torch.ones(4, dtype=torch.float64))


def test_empty_region_is_nan_in_its_row_only(ragged):
    from crfp_amd import utils as U
    m = ragged["d_m"][:2].clone()
    m[:, 1] = False
    t = U.frame_metrics_table(ragged["d_sr"][:2], ragged["d_hr"][:2], m, luma=True)
    assert torch.isnan(t[:, 2]).all() and not torch.isnan(t[:, [0, 1, 3]]).any()
    assert torch.equal(t[:, [0, 1, 3]], ragged["got"][:2][:, [0, 1, 3]])
    as_float = U.frame_metrics_table(ragged["d_sr"][:2], ragged["d_hr"][:2], m.float() * 3.0, luma=True)   # non-zero = inside
    assert torch.equal(torch.nan_to_num(as_float), torch.nan_to_num(t))


def test_bit_identity_batch_repeat_dirty_workspace_and_order(ragged):
    from crfp_amd import _lib, utils as U
    sr, hr, m, got = ragged["d_sr"], ragged["d_hr"], ragged["d_m"], ragged["got"]
    for i in range(5):
        assert torch.equal(U.frame_metrics_table(sr[i:i + 1], hr[i:i + 1], m[i:i + 1], luma=True)[0], got[i]), i
    assert torch.equal(U.frame_metrics_table(sr, hr, m, luma=True), got)
    L = _lib.lib()
    wsb = L.crfp_frame_metrics_workspace_bytes(5, 3, 70, 150)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev())
    out = torch.full((5, 4, 4), -1.0, dtype=torch.float64, device=dev())
    m8 = m.contiguous().view(torch.uint8)
    rc = L.crfp_frame_metrics_f32(sr.data_ptr(), hr.data_ptr(), m8.data_ptr(), out.data_ptr(), 5, 3, 3, 70, 150, 1, ws.data_ptr(), wsb,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(out, got)
    perm = torch.tensor([1, 0], device=dev())
    swapped = U.frame_metrics_table(sr[:2].index_select(0, perm), hr[:2].index_select(0, perm), m[:2].index_select(0, perm), luma=True)
    assert torch.equal(swapped, got[:2].index_select(0, perm))


@pytest.mark.parametrize("i_batch,C", [(0, 3), (1, 3), (0, 1)])
def test_eval_clip_fused_equals_per_frame(i_batch, C):
    from crfp_amd import evalrig
    g = torch.Generator().manual_seed(5 + i_batch + C)
    N, H, W = 4, 40, 72
    hr = torch.rand(1, N, 3, H, W, generator=g)
    batch = {"HR": hr.to(dev()), "LR_sr": (hr + 0.04 * torch.randn(1, N, 3, H, W, generator=g)).to(dev())}
    sr = (hr + 0.02 * torch.randn(1, N, 3, H, W, generator=g))[:, :, :C].contiguous().to(dev())
    if C == 1:   # a y_only model's output: the luma of HR plus noise; eval_clip merges it with LR_sr's chroma
        y = 0.299 * hr[:, :, 0:1] + 0.587 * hr[:, :, 1:2] + 0.114 * hr[:, :, 2:3]
        sr = (y + 0.01 * torch.randn(1, N, 1, H, W, generator=g)).contiguous().to(dev())
    ref = evalrig.eval_clip(None, batch, i_batch, sr=sr, fused=False)
    got = evalrig.eval_clip(None, batch, i_batch, sr=sr, fused=True)
    assert len(got) == len(ref) == (N - 1 if i_batch == 0 else N) and all(isinstance(r, tuple) and len(r) == 4 for r in got)
    for f, (a, b) in enumerate(zip(got, ref)):
        d = [abs(x - y) for x, y in zip(a, b)]
        print(f"eval_clip i_batch {i_batch} C {C} frame {f}: " + "  ".join(f"{c} {v:.3e}" for c, v in zip(COLS, d)))
        assert d[0] < PSNR_TOL and d[1] < SSIM_TOL and d[2] < PSNR_TOL and d[3] < SSIM_TOL
    psnrs = evalrig.eval_clip(None, batch, i_batch, with_ssim=False, sr=sr, fused=True)
    assert [len(r) for r in psnrs] == [2] * len(ref) and all(abs(p[0] - r[0]) < PSNR_TOL and abs(p[1] - r[2]) < PSNR_TOL for p, r in zip(psnrs, ref))


def test_gaze_rig_fused_metrics_equal_the_per_region_calls():
    from crfp_amd import gaze, synth
    from crfp_amd.model import CRFP
    sd = synth.make_state_dict(7)
    h, w, N, fv = 16, 24, 5, 32
    lr = T(synth.make_clip(21, 1, N, h, w, fv_size=fv)[0][0])
    rs = np.random.RandomState(4)
    gt = torch.clamp(F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False) +
                     T(rs.normal(0, 0.02, (N, 3, 8 * h, 8 * w)).astype(np.float32)), 0, 1)
    m = CRFP.MRCF_simple_v18(device=dev(), mid_channels=32)
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev()).eval()
    run = lambda fused: gaze.run_gaze_video(m, lr.to(dev()), gt.to(dev()), sigma=6.0, fv_size=fv, seed=11, fv_start=1, regional_dcn=True,   # noqa: E731
                                            rg=96, fused_metrics=fused)
    ref, got = run(False), run(True)
    assert got["trajectory"] == ref["trajectory"] and got["frames"] == N and set(got) == set(ref)
    for r in ("whole", "fovea", "outskirt", "past"):
        assert len(got["per_frame"][r]) == len(ref["per_frame"][r]) == (N - 1 if r == "past" else N), r
        for f, (a, b) in enumerate(zip(got["per_frame"][r], ref["per_frame"][r])):
            print(f"rig {r} entry {f}: psnr {abs(a[0] - b[0]):.3e}  ssim {abs(a[1] - b[1]):.3e}")
            assert abs(a[0] - b[0]) < PSNR_TOL and abs(a[1] - b[1]) < SSIM_TOL, (r, f)
        assert abs(got[f"psnr_{r}"] - ref[f"psnr_{r}"]) < PSNR_TOL and abs(got[f"ssim_{r}"] - ref[f"ssim_{r}"]) < SSIM_TOL


def test_argument_errors_through_ctypes_leave_the_library_usable(ragged):
    from crfp_amd import _lib, utils as U
    L = _lib.lib()
    sr, hr, m = ragged["d_sr"], ragged["d_hr"], ragged["d_m"].contiguous().view(torch.uint8)
    wsb = L.crfp_frame_metrics_workspace_bytes(5, 3, 70, 150)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev())
    out = torch.zeros(5, 4, 4, dtype=torch.float64, device=dev())
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(sr=sr.data_ptr(), hr=hr.data_ptr(), masks=m.data_ptr(), out=out.data_ptr(), n=5, c=3, m=3, h=70, w=150, flags=1,
              ws=ws.data_ptr(), wsb=wsb)
    cases = [(dict(sr=None), -1), (dict(hr=None), -1), (dict(out=None), -1), (dict(n=0), -1), (dict(c=0), -1), (dict(c=5), -1),
             (dict(m=-1), -1), (dict(m=8), -1), (dict(masks=None), -1), (dict(c=1), -1), (dict(c=4), -1), (dict(wsb=wsb - 1), -2),
             (dict(ws=None), -2)]
    for change, code in cases:
        a = dict(ok, **change)
        rc = L.crfp_frame_metrics_f32(a["sr"], a["hr"], a["masks"], a["out"], a["n"], a["c"], a["m"], a["h"], a["w"], a["flags"], a["ws"],
                                      ctypes.c_size_t(a["wsb"]), s)
        assert rc == code and len(L.crfp_last_error_string()) > 0, (change, rc)
    with pytest.raises(RuntimeError, match="LUMA"):
        U.frame_metrics_table(sr[:, :1].contiguous(), hr[:, :1].contiguous(), None, luma=True)
    assert torch.equal(out, torch.zeros_like(out))                                       # no refused call wrote anything
    assert torch.equal(U.frame_metrics_table(sr, hr, ragged["d_m"], luma=True), ragged["got"])
