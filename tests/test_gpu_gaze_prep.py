"""GPU (-m gpu): crfp_gaze_prep_f32 (through ctypes and through gaze.FusedRegionMasks / run_gaze_video(fused_masks=)) against the composed
gaze.RegionMasks and `gt * mk` on the device, bit for bit, and against the NumPy restatement of its definition (tests/gaze_rects_ref.py) for rows
no trajectory produces.  Every call writes into buffers carved out of larger allocations, pre-filled with 0xFF bytes (NaN as fp32), with 256
guard bytes on both sides that must come back untouched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gaze_rects_ref as gref

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GUARD = 256

# name -> c, H, W, fv, regional box side when on, [(cur_y, cur_x)]: 23 x 45 -- the grown rectangle is taller than the frame and W % 4 != 0 (the
# element-wise form); 70 x 150 -- W % 4 = 2; 64 x 256 -- the 16-byte form; 16 x 64 -- the window as tall as the frame, one channel
SHAPES = {
    "3x23x45": (3, 23, 45, 8, 20, gref.CASES["23x45"][5]),
    "3x70x150": (3, 70, 150, 16, 24, gref.CASES["70x150"][5]),
    "3x64x256": (3, 64, 256, 32, 40, gref.CASES["64x256"][5]),
    "1x16x64": (1, 16, 64, 16, 24, [(0, 0), (0, 48), (0, 20), (0, 20), (0, 48), (0, 3)]),
}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


class Guarded:
    """`nbytes` of device memory at byte offset `lead` (>= GUARD) of a larger 0xFF-filled allocation."""

    def __init__(self, nbytes, lead=GUARD):
        self.raw = torch.full((lead + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev())
        self.lead, self.nbytes = lead, nbytes
        self.body = self.raw[lead:lead + nbytes]

    def intact(self):
        return bool((self.raw[:self.lead] == 0xFF).all()) and bool((self.raw[self.lead + self.nbytes:] == 0xFF).all())


def prep(rows, gt, n, c, H, W, dilate=10, lead=GUARD):
    """One crfp_gaze_prep_f32 call on int32 rows [n, 24] (NumPy) -> dict of the outputs; the guards are checked here."""
    from crfp_amd import _lib
    L = _lib.lib()
    d_rows = T(np.ascontiguousarray(rows, dtype=np.int32)).to(dev())
    bufs = {"mk": Guarded(n * H * W, lead), "regions": Guarded(n * 3 * H * W, lead), "fg": Guarded(n * H * W, lead)}
    if gt is not None:
        bufs["fv"] = Guarded(n * c * H * W * 4, lead)
    ptr = lambda k: bufs[k].body.data_ptr()   # noqa: E731
    with torch.cuda.device(dev()):
        rc = L.crfp_gaze_prep_f32(None if gt is None else gt.data_ptr(), d_rows.data_ptr(), ptr("fv") if gt is not None else None, ptr("mk"),
                                  ptr("regions"), ptr("fg"), n, c, H, W, dilate, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.crfp_last_error_string()
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values()), "a guard byte changed"
    out = {"mk": bufs["mk"].body.view(n, 1, H, W), "regions": bufs["regions"].body.view(n, 3, H, W), "fg": bufs["fg"].body.view(n, 1, H, W)}
    assert all(int(v.max()) <= 1 for v in out.values()), "a mask byte is neither 0 nor 1 (or was not written)"
    if gt is not None:
        out["fv"] = bufs["fv"].body.view(torch.float32).view(n, c, H, W)
    return out


def composed(H, W, fv, fv_start, rg, origins, gt):
    """RegionMasks + gt * mk on the device for every frame of the trajectory: list of dicts of uint8 / fp32 tensors."""
    from crfp_amd import gaze
    masks = gaze.RegionMasks(H, W, fv, dev(), fv_start, rg > 0, rg, rg)
    out = []
    for n, (cur_y, cur_x) in enumerate(origins):
        m = masks.frame(n, cur_y, cur_x)
        past = m["past"] if m["past"] is not None else torch.zeros_like(m["mk"])
        out.append({"mk": m["mk"].view(torch.uint8), "fg": m["fg"].view(torch.uint8),
                    "regions": torch.cat((m["fovea"], m["outskirt"], past), 1).view(torch.uint8), "fv": gt[n:n + 1] * m["mk"]})
    return out


@pytest.fixture(scope="module")
def frames():
    """Ground-truth frames per shape, strictly positive so that gt * mk has no -0 and no pixel of the fovea is 0 by chance."""
    rs = np.random.RandomState(3)
    return {k: T(rs.uniform(0.1, 1.0, (len(o), c, H, W)).astype(np.float32)).to(dev()) for k, (c, H, W, _, _, o) in SHAPES.items()}


@pytest.mark.parametrize("regional", [False, True])
@pytest.mark.parametrize("fv_start", [0, 2])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_frame_equals_region_masks_and_gt_times_mk(shape, fv_start, regional, frames):
    from crfp_amd import gaze
    c, H, W, fv, rg, origins = SHAPES[shape]
    rg = rg if regional else 0
    gt = frames[shape]
    if regional:   # the box is clipped at a vertical border for some frames and not for others (16 x 64: a box taller than the frame)
        boxes = [gaze.regional_box(y, x, fv, rg, rg, H, W) for y, x in origins]
        assert any(x1 - x0 == rg for _, _, x0, x1 in boxes) and any(x1 - x0 < rg for _, _, x0, x1 in boxes)
        assert any(y1 - y0 < rg for y0, y1, _, _ in boxes) and (rg > H or any(y1 - y0 == rg for y0, y1, _, _ in boxes))
    rows = gaze.rect_table(origins, H, W, fv, fv_start=fv_start, regional_dcn=regional, rg_h=rg, rg_w=rg)
    ref = composed(H, W, fv, fv_start, rg, origins, gt)
    for n in range(len(origins)):
        got = prep(rows[n:n + 1], gt[n:n + 1], 1, c, H, W)
        for k in ("mk", "regions", "fg", "fv"):
            assert torch.equal(got[k], ref[n][k]), (shape, n, k)
        only = prep(rows[n:n + 1], None, 1, c, H, W)   # masks alone: gt = fv = NULL
        assert set(only) == {"mk", "regions", "fg"} and all(torch.equal(only[k], got[k]) for k in only), (shape, n)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_batch_of_three_rows_equals_three_calls(shape, frames):
    from crfp_amd import gaze
    c, H, W, fv, rg, origins = SHAPES[shape]
    rows = gaze.rect_table(origins, H, W, fv, fv_start=1, regional_dcn=True, rg_h=rg, rg_w=rg)
    pick = [5, 0, 3]
    assert len({rows[i].tobytes() for i in pick}) == 3
    gt = frames[shape][pick].contiguous()
    both = prep(rows[pick], gt, 3, c, H, W)
    for j, i in enumerate(pick):
        one = prep(rows[i:i + 1], gt[j:j + 1], 1, c, H, W)
        for k in ("mk", "regions", "fg", "fv"):
            assert torch.equal(both[k][j:j + 1], one[k]), (shape, i, k)


def test_pointers_off_16_bytes_take_the_element_wise_form(frames):
    """W % 4 == 0 with every output 4 bytes past a 16-byte boundary: same bits as the aligned call, guards intact."""
    from crfp_amd import gaze
    c, H, W, fv, rg, origins = SHAPES["3x64x256"]
    rows = gaze.rect_table(origins, H, W, fv, regional_dcn=True, rg_h=rg, rg_w=rg)
    gt = frames["3x64x256"]
    for n in (0, 4, 7):
        a, b = prep(rows[n:n + 1], gt[n:n + 1], 1, c, H, W), prep(rows[n:n + 1], gt[n:n + 1], 1, c, H, W, lead=GUARD + 4)
        assert all(torch.equal(a[k], b[k]) for k in a), n


def _row(box, *entries):
    r = list(box)
    for e in entries:
        r += list(e)
    return np.array(r + [0] * (gref.ROW_INTS - len(r)), dtype=np.int32)


@pytest.mark.parametrize("H,W", [(23, 45), (32, 64)])
def test_rows_outside_the_frame_give_the_clipped_result(H, W):
    """Rows no trajectory produces -- rectangles partly or wholly outside the frame, empty ones, absent entries, extreme values -- against the
    NumPy restatement; fv is +0 (all bits clear) outside mk even where gt is negative."""
    big = 2 ** 31 - 1
    rows = np.stack([
        _row((0, H, 0, W), (-5, -3, 12, 9, 3), (H - 4, W - 6, 12, 12, 3), (-40, 5, 8, 8, 3), (7, W + 3, 8, 8, 1)),
        _row((-7, 9, W - 5, W + 30), (5, W - 4, 10, 10, 3), (3, 3, 0, 8, 3), (3, 3, 8, -2, 3), (H + 11, 2, 6, 6, 3)),
        _row((H, H + 5, 0, W), (-big, -big, big, big, 3), (2, 2, 5, 5, 0), (big, big, big, big, 3), (-big - 1, 0, big, 9, 1)),
        _row((5, 2, 0, W), (4, 6, 7, 11, 2), (4, 6, 7, 11, 1), (0, 0, 0, 0, 0), (H - 1, W - 1, 1, 1, 3)),
        _row((-big - 1, big, -big - 1, big), (0, 0, H, W, 3), (0, 0, H, W, 3), (0, 0, H, W, 1), (1, 1, 2, 2, 3)),
    ])
    n, c = rows.shape[0], 2
    gt = T(np.random.RandomState(8).uniform(-1.0, 1.0, (n, c, H, W)).astype(np.float32)).to(dev())
    for dilate in (10, 0, 3):
        got = prep(rows, gt, n, c, H, W, dilate=dilate)
        for i in range(n):
            ref = gref.rasterise(rows[i], H, W, dilate)
            for k, plane in (("mk", got["mk"][i, 0]), ("fovea", got["regions"][i, 0]), ("outskirt", got["regions"][i, 1]),
                             ("past", got["regions"][i, 2]), ("fg", got["fg"][i, 0])):
                assert np.array_equal(plane.cpu().numpy().astype(bool), ref[k]), (H, W, dilate, i, k)
            mk = T(ref["mk"]).to(dev())
            want = torch.where(mk, gt[i], torch.zeros((), device=dev())).view(torch.int32)
            assert torch.equal(got["fv"][i].view(torch.int32), want), (H, W, dilate, i, "fv bits")


def test_fused_region_masks_returns_the_rig_dict(frames):
    from crfp_amd import gaze
    c, H, W, fv, rg, origins = SHAPES["3x70x150"]
    gt = frames["3x70x150"]
    fused = gaze.FusedRegionMasks(H, W, fv, dev(), 2, True, rg, rg, origins=origins)
    ref = composed(H, W, fv, 2, rg, origins, gt)
    for n in range(len(origins)):
        m = fused.frame(n, gt[n:n + 1])
        assert set(m) == {"mk", "fovea", "outskirt", "past", "fg", "fv", "regions"}
        assert all(m[k].dtype == torch.bool and m[k].shape == (1, 1, H, W) for k in ("mk", "fovea", "outskirt", "fg"))
        assert (m["past"] is None) == (n == 0) and m["regions"].dtype == torch.uint8
        assert torch.equal(m["regions"], ref[n]["regions"]) and torch.equal(m["fv"], ref[n]["fv"])
        assert torch.equal(m["mk"].view(torch.uint8), ref[n]["mk"]) and torch.equal(m["fg"].view(torch.uint8), ref[n]["fg"])
        assert torch.equal(torch.cat((m["fovea"], m["outskirt"]), 1).view(torch.uint8), ref[n]["regions"][:, :2])
        if n:
            assert torch.equal(m["past"].view(torch.uint8), ref[n]["regions"][:, 2:3])
    only = fused.frame(3)
    assert only["fv"] is None and torch.equal(only["regions"], ref[3]["regions"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused.frame(1, gt[1:2].cpu())
    with pytest.raises(IndexError):
        fused.frame(len(origins))


@pytest.mark.parametrize("fused_metrics", [True, False])
def test_gaze_rig_with_fused_masks_equals_the_composed_rig(fused_metrics):
    """MRCF_simple_v18, synthetic weights, 6 frames at 24 x 40 -> 192 x 320, fv 32, sigma 120, seed 5, regional box 96: the same inputs reach the
    model and the metrics, so every figure is exactly equal."""
    from crfp_amd import gaze, synth
    from crfp_amd.model import CRFP
    sd = synth.make_state_dict(7)
    h, w, N, fv = 24, 40, 6, 32
    lr = T(synth.make_clip(21, 1, N, h, w, fv_size=fv)[0][0])
    gt = torch.clamp(F.interpolate(lr, scale_factor=8, mode="bilinear", align_corners=False) +
                     T(np.random.RandomState(4).normal(0, 0.02, (N, 3, 8 * h, 8 * w)).astype(np.float32)), 0, 1)
    m = CRFP.MRCF_simple_v18(device=dev(), mid_channels=32)
    m.load_state_dict({k: T(v.copy()) for k, v in sd.items()}, strict=True)
    m = m.to(dev()).eval()
    run = lambda fused: gaze.run_gaze_video(m, lr.to(dev()), gt.to(dev()), sigma=120.0, fv_size=fv, seed=5, regional_dcn=True, rg=96,   # noqa: E731
                                            fused_metrics=fused_metrics, fused_masks=fused)
    ref, got = run(False), run(True)
    H, W = 8 * h, 8 * w
    traj = ref["trajectory"]
    assert any(y in (0, H - fv) or x in (0, W - fv) for y, x in traj) and any(0 < y < H - fv and 0 < x < W - fv for y, x in traj)
    assert got["trajectory"] == traj and got["frames"] == N and set(got) == set(ref)
    for r in ("whole", "fovea", "outskirt", "past"):
        assert len(ref["per_frame"][r]) == (N - 1 if r == "past" else N)
        assert got["per_frame"][r] == ref["per_frame"][r], r
        assert got[f"psnr_{r}"] == ref[f"psnr_{r}"] and got[f"ssim_{r}"] == ref[f"ssim_{r}"], r
