"""GPU (-m gpu): crfp_frame_ingest_u8 / crfp_frame_export_u8 through ctypes against the NumPy restatement of their definitions
(tests/frameio_ref.py), bit for bit, and crfp_amd.frameio (ingest, export, HostStreamer) around MRCF_simple_v18 against the torch composition.
Every ctypes call writes into buffers carved out of larger allocations, pre-filled with 0xFF bytes (NaN as fp32), with 256 guard bytes on both
sides that must come back untouched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frameio_ref as fref

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GUARD = 256
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


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

    def numpy(self, dtype, shape):
        return self.body.cpu().numpy().view(dtype).reshape(shape)


def codes(rs, shape):
    """uint8 data of `shape` holding every code 0..255 as often as the size allows, shuffled"""
    size = int(np.prod(shape))
    return rs.permutation(np.arange(size) % 256).astype(np.uint8).reshape(shape)


def run_ingest(lr_u8, crop_u8, rects, H, W, bgr, lead=GUARD):
    """One crfp_frame_ingest_u8 call on NumPy inputs (lr_u8, or crop_u8 and rects, may be None) -> (lr, fv, mk) as NumPy; guards checked here."""
    from crfp_amd import _lib
    L = _lib.lib()
    n = (lr_u8 if lr_u8 is not None else crop_u8).shape[0]
    h, w = lr_u8.shape[1:3] if lr_u8 is not None else (1, 1)
    fh, fw = crop_u8.shape[1:3] if crop_u8 is not None else (1, 1)
    d = {k: None if v is None else T(np.ascontiguousarray(v)).to(dev()) for k, v in (("lr_u8", lr_u8), ("crop_u8", crop_u8), ("rects", rects))}
    bufs = {}
    if lr_u8 is not None:
        bufs["lr"] = Guarded(n * 3 * h * w * 4, lead)
    if crop_u8 is not None:
        bufs["fv"], bufs["mk"] = Guarded(n * 3 * H * W * 4, lead), Guarded(n * H * W, lead)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    out = lambda k: bufs[k].body.data_ptr() if k in bufs else None   # noqa: E731
    with torch.cuda.device(dev()):
        rc = L.crfp_frame_ingest_u8(ptr(d["lr_u8"]), ptr(d["crop_u8"]), ptr(d["rects"]), out("lr"), out("fv"), out("mk"), n, h, w, fh, fw, H, W,
                                    fref.BGR if bgr else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.crfp_last_error_string()
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values()), "a guard byte changed"
    return (bufs["lr"].numpy(np.float32, (n, 3, h, w)) if "lr" in bufs else None,
            bufs["fv"].numpy(np.float32, (n, 3, H, W)) if "fv" in bufs else None,
            bufs["mk"].numpy(np.uint8, (n, 1, H, W)) if "mk" in bufs else None)


def placements(H, W, fh, fw):
    """(y, x, flags) of a crop: interior at x % 4 == 0 and x % 4 != 0, over each corner, wholly outside, extreme origins, flag clear"""
    return [(H // 2 - fh // 2, 8, 1), (5, 13, 1), (-5, -7, 1), (-5, W - fw + 7, 1), (H - fh + 5, -7, 1), (H - fh + 5, W - fw + 7, 1),
            (H + 3, 4, 1), (3, -fw, 1), (-fh, -fw - 1, 1), (IMIN, IMIN, 1), (IMAX, IMAX, 1), (IMIN, 5, 1), (4, IMAX, 1), (5, 13, 0), (5, 13, 2),
            (0, 0, 3), (H - fh, W - fw, 1), (-fh + 1, -fw + 1, 1)]


def check_ingest(got, lr_u8, crop_u8, rects, H, W, bgr, tag):
    lr, fv, mk = got
    assert np.array_equal(lr.view(np.int32), fref.ingest_lr(lr_u8, bgr).view(np.int32)), (tag, "lr")
    want_fv, want_mk = fref.ingest_fovea(crop_u8, rects, H, W, bgr)
    assert np.array_equal(mk, want_mk), (tag, "mk")
    assert np.array_equal(fv.view(np.int32), want_fv.view(np.int32)), (tag, "fv bits")       # +0 outside R: the sign bit too
    assert not (fv.view(np.int32)[np.broadcast_to(want_mk == 0, fv.shape)]).any(), (tag, "fv outside R")


# h, w, H, W: 8h x 8w frames whose W is a multiple of 4 (the 4-pixel form; 7 x 9 and 17 x 65: h * w is not, the LR frame takes the element-wise
# form), and one 37 x 53 frame (the element-wise form of the fovea kernel)
INGEST_SHAPES = [(7, 9, 56, 72, 1), (7, 9, 56, 72, 3), (16, 64, 128, 512, 1), (16, 64, 128, 512, 3), (17, 65, 136, 520, 1), (17, 65, 136, 520, 3),
                 (6, 10, 37, 53, 1)]


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("h,w,H,W,n", INGEST_SHAPES)
def test_ingest_equals_the_restatement(h, w, H, W, n, bgr):
    fh, fw = 12, 20
    rs = np.random.RandomState(h * 100 + w + n)
    place = placements(H, W, fh, fw)
    seen = set()
    for i in range(0, len(place), n):
        rects = np.array([(y, x, f, 0) for y, x, f in place[i:i + n]], dtype=np.int64).astype(np.int32)
        if rects.shape[0] < n:
            rects = np.concatenate([rects, np.array([(1, 2, 1, 0)] * (n - rects.shape[0]), np.int32)])
        lr_u8, crop_u8 = codes(rs, (n, h, w, 3)), codes(rs, (n, fh, fw, 3))
        seen |= set(np.unique(lr_u8)) | set(np.unique(crop_u8))
        check_ingest(run_ingest(lr_u8, crop_u8, rects, H, W, bgr), lr_u8, crop_u8, rects, H, W, bgr, (h, w, H, W, n, bgr, i))
    assert len(seen) == 256


def test_ingest_halves_alone_and_pointers_off_their_alignment():
    """LR only, fovea only, and W % 4 == 0 with every output 4 bytes past a 16-byte boundary (the element-wise form): the same bits."""
    h, w, H, W, fh, fw, n = 16, 64, 128, 512, 12, 20, 2
    rs = np.random.RandomState(9)
    lr_u8, crop_u8 = codes(rs, (n, h, w, 3)), codes(rs, (n, fh, fw, 3))
    rects = np.array([(-5, W - fw + 7, 1, 0), (50, 13, 1, 0)], np.int32)
    for bgr in (False, True):
        both = run_ingest(lr_u8, crop_u8, rects, H, W, bgr)
        check_ingest(both, lr_u8, crop_u8, rects, H, W, bgr, "both")
        lr_only, fv_only = run_ingest(lr_u8, None, None, H, W, bgr), run_ingest(None, crop_u8, rects, H, W, bgr)
        assert lr_only[1] is None and lr_only[2] is None and fv_only[0] is None
        off = run_ingest(lr_u8, crop_u8, rects, H, W, bgr, lead=GUARD + 4)
        for a, b in ((lr_only[0], both[0]), (fv_only[1], both[1]), (fv_only[2], both[2]), (off[0], both[0]), (off[1], both[1]), (off[2], both[2])):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_export(sr, chroma, bgr, lead=GUARD, in_lead=0):
    """One crfp_frame_export_u8 call on NumPy inputs -> uint8 [n,H,W,3]; in_lead: bytes by which sr and chroma are moved off their alignment."""
    from crfp_amd import _lib
    L = _lib.lib()
    n, c, H, W = sr.shape

    def put(a):
        if a is None:
            return None
        raw = torch.empty(a.nbytes + 16, dtype=torch.uint8, device=dev())
        body = raw[in_lead:in_lead + a.nbytes]
        body.copy_(T(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev()))
        return body

    d_sr, d_ch = put(sr), put(chroma)
    buf = Guarded(n * H * W * 3, lead)
    with torch.cuda.device(dev()):
        rc = L.crfp_frame_export_u8(d_sr.data_ptr(), None if d_ch is None else d_ch.data_ptr(), buf.body.data_ptr(), n, c, H, W,
                                    fref.BGR if bgr else 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.crfp_last_error_string()
    torch.cuda.synchronize()
    assert buf.intact(), "a guard byte changed"
    return buf.numpy(np.uint8, (n, H, W, 3))


def export_values(rs, shape):
    """[-0.3, 1.3] with the 255 ties, -0.0, denormals, +-inf and NaN in front"""
    v = rs.uniform(-0.3, 1.3, shape).astype(np.float32)
    tiny = np.float32(1e-45)
    special = np.concatenate([fref.ties()[0], np.array([-0.0, 0.0, tiny, -tiny, np.float32(1e-39), np.inf, -np.inf, np.nan, 1.0, 0.5], np.float32)])
    flat = v.reshape(-1)
    flat[:special.size] = special
    flat[-special.size:] = special[::-1]
    return v


# H, W: 9 x 53 and 9 x 65 -- H * W is odd (the element-wise form); 8 x 64 -- the 4-pixel form; 8 x 65 -- the 4-pixel form with quads that cross rows
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("n,H,W", [(1, 9, 53), (2, 8, 64), (2, 9, 65), (3, 8, 65)])
def test_export_equals_the_restatement(n, H, W, c, bgr):
    rs = np.random.RandomState(H * W + c)
    sr = export_values(rs, (n, c, H, W))
    chroma = export_values(rs, (n, 3, H, W))[:, ::-1].copy() if c == 1 else None
    want = fref.export(sr, chroma, bgr)
    assert np.array_equal(run_export(sr, chroma, bgr), want), "aligned"
    assert np.array_equal(run_export(sr, chroma, bgr, lead=GUARD + 1), want), "output 1 byte off"
    assert np.array_equal(run_export(sr, chroma, bgr, in_lead=4), want), "inputs 4 bytes off"


def test_export_of_ingest_is_the_identity_on_all_codes():
    from crfp_amd import frameio
    frame = T(codes(np.random.RandomState(2), (2, 16, 64, 3))).to(dev())
    for bgr in (False, True):
        lr, _, _ = frameio.ingest(frame, None, None, 128, 512, bgr=bgr)
        assert torch.equal(frameio.export(lr, bgr=bgr), frame)
    out = torch.empty((2, 16, 64, 3), dtype=torch.uint8, device=dev())
    assert frameio.export(frameio.ingest(frame, None, None, 128, 512)[0], out=out) is out and torch.equal(out, frame)


# ---------------------------------------------------------------------------------------------------------------- end to end
H_LR, W_LR, FV, FRAMES = 24, 40, 48, 7
# (y, x) of the 48 x 48 window in the 192 x 320 frame: the top edge, the right edge, the interior
ORIGINS = [(0, 100), (10, 272), (60, 131), (144, 7), (77, 272), (0, 0), (33, 57)]


@pytest.fixture(scope="module")
def clip():
    """7 LR frames and their HR frames as 8-bit HWC host arrays"""
    from crfp_amd import synth
    lr = synth.make_clip(21, 1, FRAMES, H_LR, W_LR, fv_size=FV)[0][0]
    hr = np.clip(F.interpolate(T(lr), scale_factor=8, mode="bilinear", align_corners=False).numpy() +
                 np.random.RandomState(4).normal(0, 0.02, (FRAMES, 3, 8 * H_LR, 8 * W_LR)).astype(np.float32), 0, 1)
    to_u8 = lambda a: np.ascontiguousarray(np.rint(a * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))   # noqa: E731
    return to_u8(lr), to_u8(hr)


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("y_only", [False, True])
def test_streamed_model_through_8_bit_frames(clip, y_only, bgr):
    from crfp_amd import frameio, gaze, ops, synth
    from crfp_amd.model import CRFP
    lr_u8, hr_u8 = clip
    if bgr:
        lr_u8, hr_u8 = lr_u8[..., ::-1].copy(), hr_u8[..., ::-1].copy()
    H, W = 8 * H_LR, 8 * W_LR
    assert any(y == 0 for y, x in ORIGINS) and any(x == W - FV for y, x in ORIGINS) and any(0 < y < H - FV and 0 < x < W - FV for y, x in ORIGINS)
    crops = np.stack([hr_u8[i, y:y + FV, x:x + FV] for i, (y, x) in enumerate(ORIGINS)])
    m = CRFP.MRCF_simple_v18(device=dev(), mid_channels=32, y_only=y_only)
    m.load_state_dict({k: T(v.copy()) for k, v in synth.make_state_dict(7, y_only=y_only).items()}, strict=True)
    m = m.to(dev()).eval()
    masks = gaze.RegionMasks(H, W, FV, dev())
    rgb = (lambda t: t.flip(-1)) if bgr else (lambda t: t)
    frames = []
    m.clear_states()
    for i, (y, x) in enumerate(ORIGINS):
        if i == 4:
            m.clear_states()
        rect = torch.tensor([[y, x, fref.HAS_FOVEA, 0]], dtype=torch.int32, device=dev())
        lr, fv, mk = frameio.ingest(T(lr_u8[i:i + 1]).to(dev()), T(crops[i:i + 1]).to(dev()), rect, H, W, bgr=bgr)
        # the torch composition from u8 / 255.  The division runs on the host, where the reference does it: on the device torch divides by a
        # Python scalar as a multiplication by its reciprocal, which is another value on 126 of the 256 codes
        want_lr = (rgb(T(lr_u8[i:i + 1])).float() / 255.).permute(0, 3, 1, 2).to(dev())
        want_mk = masks.frame(i, y, x)["mk"]
        want_fv = (rgb(T(hr_u8[i:i + 1])).float() / 255.).permute(0, 3, 1, 2).to(dev()) * want_mk
        assert mk.dtype == torch.bool and torch.equal(mk, want_mk), i
        assert torch.equal(lr, want_lr) and torch.equal(fv.view(torch.int32), want_fv.contiguous().view(torch.int32)), i
        sr = m(lrs=lr.unsqueeze(0), fvs=fv.unsqueeze(0), mks=mk.unsqueeze(0), fgs=None).reshape(1, -1, H, W)
        assert sr.shape[1] == (1 if y_only else 3)
        chroma = ops.upsample_bilinear(lr, scale_factor=8) if y_only else None
        out = frameio.export(sr, chroma, bgr=bgr)
        want = fref.export(sr.cpu().numpy(), None if chroma is None else chroma.cpu().numpy(), bgr)
        assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want), i
        frames.append(want[0])
    assert len({f.tobytes() for f in frames}) == FRAMES
    # the pipelined host path: depth 2, fetches lag submits by one, every slot is reused
    s = frameio.HostStreamer(m, H_LR, W_LR, FV, depth=2, bgr=bgr)
    s.clear_states()
    got = []
    for i, origin in enumerate(ORIGINS):
        if i == 4:
            s.clear_states()
        s.submit(lr_u8[i], crops[i], origin)
        if i >= 1:
            assert s.pending() == 2
            got.append(s.fetch())
    got.append(s.fetch())
    assert s.pending() == 0 and len(got) == FRAMES
    for i in range(FRAMES):
        assert got[i].dtype == np.uint8 and got[i].shape == (H, W, 3) and np.array_equal(got[i], frames[i]), i
    with pytest.raises(RuntimeError, match="without a queued frame"):
        s.fetch()


def test_host_streamer_keeps_depth_frames_in_flight(clip):
    """Two submits before the first fetch (both slots in flight), a third is refused; has_fovea=False equals a crop that lies outside."""
    from crfp_amd import frameio, synth
    from crfp_amd.model import CRFP
    lr_u8, hr_u8 = clip
    crop = hr_u8[0, :FV, :FV]
    m = CRFP.MRCF_simple_v18(device=dev(), mid_channels=32)
    m.load_state_dict({k: T(v.copy()) for k, v in synth.make_state_dict(7).items()}, strict=True)
    m = m.to(dev()).eval()
    s = frameio.HostStreamer(m, H_LR, W_LR, FV, depth=2)
    runs = []
    for kwargs in ({"origin": (0, 0), "has_fovea": False}, {"origin": (5000, 0)}, {"origin": (0, 0)}):
        s.clear_states()
        s.submit(lr_u8[0], crop, **kwargs)
        s.submit(lr_u8[1], crop, **kwargs)
        assert s.pending() == 2
        with pytest.raises(RuntimeError, match="fetch"):
            s.submit(lr_u8[2], crop, **kwargs)
        runs.append((s.fetch(), s.fetch()))
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert not np.array_equal(runs[0][0], runs[2][0])
