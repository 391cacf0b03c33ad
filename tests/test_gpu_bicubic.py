"""GPU (-m gpu): crfp_resize_bicubic_u8 / crfp_frame_export_y_bicubic_u8 through ctypes against PIL on the host (and tests/frameio_ref.py for
the merge on PIL's frame), and crfp_amd.frameio (resize_bicubic, export_y_bicubic, HostStreamer(chroma="bicubic")).  Every comparison is
equality.  Every ctypes call writes into buffers carved out of larger allocations, pre-filled with 0xFF bytes, with 256 guard bytes on both
sides that must come back untouched; the workspace is guarded too, and the tables the device wrote into it are compared int for int with
crfp_bicubic_taps."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bicubic_ref as bref
import frameio_ref as fref
from test_gpu_frameio import GUARD, Guarded, dev, export_values

pytestmark = pytest.mark.gpu

T = torch.from_numpy
OUT_F32, TWO_PASS = 2, 4
# the CPU list without the rig's frame; 17 x 23 and 33 x 47 at x8 are 5 x 3 and 9 x 6 tiles of 32 x 64 with ragged edges on both axes
PAIRS = [p for p in bref.PAIRS if p[0] != 134] + [(33, 47, 264, 376)]


@pytest.fixture(autouse=True)
def _nograd():
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def frames(h, w, H, W):
    """three source frames [3,h,w,3] (uniform, 0 / 255, a band around 128) and PIL's resize of each [3,H,W,3]; computed once per geometry"""
    rs = np.random.RandomState(h * 1000 + W)
    c = bref.contents(rs, (h, w, 3))
    src = np.stack([c["uniform"], c["binary"], c["band"]])
    want = np.stack([bref.pil_resize(f, H, W) for f in src])
    src.setflags(write=False)
    want.setflags(write=False)
    return src, want


def put(a, lead=0):
    """`a` on the device at byte offset `lead` of an allocation"""
    raw = torch.empty(a.nbytes + 16, dtype=torch.uint8, device=dev())
    body = raw[lead:lead + a.nbytes]
    body.copy_(T(np.array(a).view(np.uint8).reshape(-1)).to(dev()))   # np.array: a writable, contiguous copy
    return body


def workspace(n, h, w, H, W):
    from crfp_amd import _lib
    need = _lib.lib().crfp_resize_bicubic_workspace_bytes(n, h, w, H, W)
    assert need > 0
    return Guarded(need)


def check_tables(ws, h, w, H, W):
    """the workspace begins with the tables of x and of y as the device computed them: the host function's, int for int"""
    from crfp_amd import _lib
    L = _lib.lib()
    got = ws.body.cpu().numpy()
    at = 0
    for i, o in ((w, W), (h, H)):
        ks = bref.ksize(i, o)
        bounds, k = np.empty((o, 2), np.int32), np.empty((o, ks), np.int32)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
        assert L.crfp_bicubic_taps(i, o, p(bounds), p(k), o * ks) == ks
        assert np.array_equal(got[at:at + 8 * o].view(np.int32).reshape(o, 2), bounds), ("bounds", i, o)
        at += 8 * o
        assert np.array_equal(got[at:at + 4 * ks * o].view(np.int32).reshape(o, ks), k), ("taps", i, o)
        at += 4 * ks * o


def run_resize(src, H, W, flags, src_lead=0, dst_lead=GUARD, tables=False):
    """One crfp_resize_bicubic_u8 call on a NumPy [n,h,w,3] -> uint8 [n,H,W,3] or float32 [n,3,H,W]; guards checked here."""
    from crfp_amd import _lib
    L = _lib.lib()
    n, h, w, _ = src.shape
    d_src, ws = put(src, src_lead), workspace(n, h, w, H, W)
    f32 = bool(flags & OUT_F32)
    buf = Guarded(n * H * W * 3 * (4 if f32 else 1), dst_lead)
    with torch.cuda.device(dev()):
        rc = L.crfp_resize_bicubic_u8(d_src.data_ptr(), buf.body.data_ptr(), n, h, w, H, W, flags, ws.body.data_ptr(), ws.nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.crfp_last_error_string()
    torch.cuda.synchronize()
    assert buf.intact() and ws.intact(), "a guard byte changed"
    if tables:
        check_tables(ws, h, w, H, W)
    return buf.numpy(np.float32, (n, 3, H, W)) if f32 else buf.numpy(np.uint8, (n, H, W, 3))


def planes(want_u8, bgr):
    """PIL's bytes [n,H,W,3] (B,G,R per pixel under bgr) -> the fp32 R,G,B planes [n,3,H,W] the reference makes: astype(float32) / 255."""
    rgb = want_u8[..., ::-1] if bgr else want_u8
    return np.ascontiguousarray((rgb.astype(np.float32) / 255.).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("h,w,H,W", PAIRS)
def test_resize_equals_pil(h, w, H, W):
    src, want = frames(h, w, H, W)
    first = True
    for sel in ([2], [0, 1]):                      # n = 1 and n = 2
        s, wu8 = src[sel], want[sel]
        for bgr in (0, 1):                         # the bytes are taken as B,G,R: the same bytes out, the planes swapped
            for lead in (0, 1):
                got = run_resize(s, H, W, bgr, src_lead=lead, dst_lead=GUARD + lead, tables=first)
                first = False
                assert np.array_equal(got, wu8), ("u8", len(sel), bgr, lead)
                got = run_resize(s, H, W, bgr | OUT_F32, src_lead=lead, dst_lead=GUARD + 4 * lead)
                assert np.array_equal(got.view(np.int32), planes(wu8, bgr).view(np.int32)), ("f32", len(sel), bgr, lead)


@pytest.mark.parametrize("h,w,H,W", [(17, 23, 136, 184), (9, 11, 10, 13)])
def test_both_paths_give_the_same_bytes(h, w, H, W):
    src, want = frames(h, w, H, W)
    for flags in (0, 1 | OUT_F32):
        fused, two = run_resize(src[:2], H, W, flags), run_resize(src[:2], H, W, flags | TWO_PASS)
        assert np.array_equal(fused.view(np.uint8), two.view(np.uint8)), flags
        assert np.array_equal(fused, planes(want[:2], 1) if flags else want[:2])


def run_merge(luma, lr_u8, H, W, bgr, luma_lead=0, dst_lead=GUARD, expect=0):
    from crfp_amd import _lib
    L = _lib.lib()
    n, h, w, _ = lr_u8.shape
    d_luma, d_lr, ws = put(luma, luma_lead), put(lr_u8), workspace(n, h, w, H, W)
    buf = Guarded(n * H * W * 3, dst_lead)
    with torch.cuda.device(dev()):
        rc = L.crfp_frame_export_y_bicubic_u8(d_luma.data_ptr(), d_lr.data_ptr(), buf.body.data_ptr(), n, h, w, H, W, fref.BGR if bgr else 0,
                                              ws.body.data_ptr(), ws.nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, L.crfp_last_error_string()
    torch.cuda.synchronize()
    assert buf.intact() and ws.intact(), "a guard byte changed"
    return buf.numpy(np.uint8, (n, H, W, 3))


@pytest.mark.parametrize("h,w,H,W", [(3, 3, 24, 24), (17, 23, 136, 184), (7, 5, 56, 40)])
def test_export_y_bicubic_equals_the_merge_on_pils_frame(h, w, H, W):
    src, want = frames(h, w, H, W)
    rs = np.random.RandomState(H + W)
    for sel in ([2], [0, 1]):
        luma = export_values(rs, (len(sel), 1, H, W))
        for bgr in (False, True):
            ref = fref.export(luma, planes(want[sel], bgr), bgr)
            assert np.array_equal(run_merge(luma, src[sel], H, W, bgr), ref), (len(sel), bgr, "aligned")
            assert np.array_equal(run_merge(luma, src[sel], H, W, bgr, dst_lead=GUARD + 1), ref), (len(sel), bgr, "output 1 byte off")
            assert np.array_equal(run_merge(luma, src[sel], H, W, bgr, luma_lead=4), ref), (len(sel), bgr, "luma 4 bytes off")


def test_export_y_bicubic_refuses_a_shrinking_geometry_and_writes_nothing():
    from crfp_amd import _lib
    rs = np.random.RandomState(1)
    for h, w, H, W in ((24, 24, 3, 3), (3, 24, 24, 23)):
        out = run_merge(rs.rand(1, 1, H, W).astype(np.float32), rs.randint(0, 256, (1, h, w, 3)).astype(np.uint8), H, W, False, expect=-3)
        assert (out == 0xFF).all()
        assert b"fused path" in _lib.lib().crfp_last_error_string()


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_resize_bicubic_in_a_graph_replays_on_new_bytes():
    """one capture, one replay with other input bytes: a single linear chain (table kernel, fused kernel)"""
    from crfp_amd import frameio
    h, w, H, W = 17, 23, 136, 184
    src, want = frames(h, w, H, W)
    x = T(src[0:1].copy()).to(dev())
    assert np.array_equal(frameio.resize_bicubic(x, H, W).cpu().numpy(), want[0:1])   # eager, and the warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = frameio.resize_bicubic(x, H, W)
    x.copy_(T(src[1:2].copy()))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[1:2])


def test_resize_bicubic_and_export_y_bicubic_wrappers():
    from crfp_amd import frameio
    h, w, H, W = 17, 23, 136, 184
    src, want = frames(h, w, H, W)
    x = T(src.copy()).to(dev())
    assert np.array_equal(frameio.resize_bicubic(x, H, W).cpu().numpy(), want)
    f32 = frameio.resize_bicubic(x, H, W, out="f32", bgr=True)
    assert f32.dtype == torch.float32 and np.array_equal(f32.cpu().numpy().view(np.int32), planes(want, True).view(np.int32))
    down = frameio.resize_bicubic(x, 5, 31)     # shrinks along y: the two-pass path
    assert np.array_equal(down.cpu().numpy(), np.stack([bref.pil_resize(f, 5, 31) for f in src]))
    luma = T(export_values(np.random.RandomState(3), (3, 1, H, W))).to(dev())
    out = torch.empty((3, H, W, 3), dtype=torch.uint8, device=dev())
    assert frameio.export_y_bicubic(luma, x, out=out) is out
    assert torch.equal(out, frameio.export(luma, frameio.resize_bicubic(x, H, W, out="f32")))
    assert np.array_equal(out.cpu().numpy(), fref.export(luma.cpu().numpy(), planes(want, False)))
    with pytest.raises(RuntimeError, match="fused path"):
        frameio.export_y_bicubic(luma[:, :, :8, :8].contiguous(), x)


H_LR, W_LR, FV, FRAMES = 16, 24, 48, 4
ORIGINS = [(0, 60), (40, 144), (80, 7), (33, 57)]


def test_host_streamer_with_bicubic_chroma():
    """a y_only MRCF_simple_v18 streamed with chroma="bicubic" delivers, frame by frame, export_y_bicubic of its luma and the staged LR frame --
    which is the merge on PIL's frame; the default keyword delivers the bilinear chroma's bytes as before"""
    from crfp_amd import frameio, ops, synth
    from crfp_amd.model import CRFP
    H, W = 8 * H_LR, 8 * W_LR
    lr = synth.make_clip(22, 1, FRAMES, H_LR, W_LR, fv_size=FV)[0][0]
    lr_u8 = np.ascontiguousarray(np.rint(lr * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))
    crops = np.random.RandomState(6).randint(0, 256, (FRAMES, FV, FV, 3)).astype(np.uint8)
    m = CRFP.MRCF_simple_v18(device=dev(), mid_channels=32, y_only=True)
    m.load_state_dict({k: T(v.copy()) for k, v in synth.make_state_dict(7, y_only=True).items()}, strict=True)
    m = m.to(dev()).eval()
    want = {"bicubic": [], "bilinear": []}
    m.clear_states()
    for i, (y, x) in enumerate(ORIGINS):
        rect = torch.tensor([[y, x, fref.HAS_FOVEA, 0]], dtype=torch.int32, device=dev())
        d_lr = T(lr_u8[i:i + 1]).to(dev())
        l, fv, mk = frameio.ingest(d_lr, T(crops[i:i + 1]).to(dev()), rect, H, W)
        sr = m(lrs=l.unsqueeze(0), fvs=fv.unsqueeze(0), mks=mk.unsqueeze(0), fgs=None).reshape(1, 1, H, W)
        out = frameio.export_y_bicubic(sr, d_lr).cpu().numpy()
        pil = bref.pil_resize(lr_u8[i], H, W)[None]
        assert np.array_equal(out, fref.export(sr.cpu().numpy(), planes(pil, False))), i
        want["bicubic"].append(out[0])
        want["bilinear"].append(frameio.export(sr, ops.upsample_bilinear(l, scale_factor=8)).cpu().numpy()[0])
    assert all(not np.array_equal(a, b) for a, b in zip(want["bicubic"], want["bilinear"]))
    for kwargs, key in (({"chroma": "bicubic"}, "bicubic"), ({}, "bilinear"), ({"chroma": "bilinear"}, "bilinear")):
        s = frameio.HostStreamer(m, H_LR, W_LR, FV, depth=2, **kwargs)
        s.clear_states()
        got = []
        for i, origin in enumerate(ORIGINS):
            s.submit(lr_u8[i], crops[i], origin)
            if i >= 1:
                got.append(s.fetch())
        got.append(s.fetch())
        for i in range(FRAMES):
            assert np.array_equal(got[i], want[key][i]), (key, i)
