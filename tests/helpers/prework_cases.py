"""The clip engines under one pre-work order, as digests: every case of tests/test_gpu_prework_batch.py in ONE process, because the library (product
or lab) and its switches (CRFP_MASK_GATE, CRFP_SIDE_STREAM) are fixed when the process loads it.  PREWORK_ORDER=per_frame in this script's
environment (lab library only) selects the one-frame-per-launch order through crfp_lab_prework_groups(0) before the first call.

    python tests/helpers/prework_cases.py OUT.json [--only PREFIX[,PREFIX...]]

OUT.json: {case id: {"frames": [[sha256 of out[b, i] ...] ...], "status": [word of clip b ...], "finite": bool}}.

Every call runs through the C entry point on a workspace this script owns, prefilled with 0xFF bytes (NaN in fp32 and in bf16): a launch that
reads a frame slot nobody wrote poisons its output.  The masks differ frame by frame -- a window that moves by (6, 5) pixels per frame across
the edges of the 64 x 16 gate tiles, every fifth frame without a single mask pixel and the one after it all mask -- so a slot that picks up
another frame's gate flags or fovea features changes bits.

Groups (engine.hip, prework_group): a clip of up to 8 frames is one group (t = 8: the cap), a longer one goes in groups of 2 with two groups' slots
in flight -- t = 9 has four full groups and a one-frame tail, from the third group on every group reuses a slot pair, t = 17 likewise; a batch goes as whole clips while n * t <= 8 (n = 2, t = 3), else one frame per launch (n = 2, t = 17: 34 frames, which
is also past the flat limit of the clip-level stages)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = {"dsv": "CRFP_DSV", "cra": "CRFP_DSV_CRA", "simple": "CRFP_simple", "dense": "CRFP"}
E_WORKSPACE = -2
OVF = 70000.0    # >= 65504: no fp16 operand holds it


def masks(n, t, H, W):
    """[n, t, 1, H, W] bool.  Frame i of clip b: a 40 x 24 window at (34 + 6 i + 3 b, 4 + 5 i + 2 b), wrapped into the frame -- it straddles x = 64
    and y = 16 in the first frames and moves on; i % 5 == 3: no mask pixel, i % 5 == 4: every pixel."""
    m = np.zeros((n, t, 1, H, W), bool)
    for b in range(n):
        for i in range(t):
            if i % 5 == 3:
                continue
            if i % 5 == 4:
                m[b, i] = True
                continue
            x0, y0 = (34 + 6 * i + 3 * b) % (W - 40), (4 + 5 * i + 2 * b) % (H - 24)
            m[b, i, 0, y0:y0 + 24, x0:x0 + 40] = True
    return m


def clip(seed, n, t, h, w):
    from crfp_amd import synth
    lrs, fvs, _ = synth.make_clip(seed, n, t, h, w, fv_size=32)
    return lrs, fvs, masks(n, t, 8 * h, 8 * w)


_engines = {}


def engine(wiring, storage, y_only):
    """One handle per (wiring, storage, y_only): seeded default init scaled up so that the fovea side matters (tests/test_gpu_cra.py)."""
    import torch
    from crfp_amd.model import CRFP
    key = (wiring, storage, y_only)
    if key not in _engines:
        dev = torch.device("cuda:0")
        torch.manual_seed(5)
        m = getattr(CRFP, MODELS[wiring])(dev, mid_channels=32, y_only=y_only).to(dev).eval()
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(1.5)
        m.storage = storage
        _engines[key] = (m, m.engine())
    return _engines[key][1]


def call(eng, lrs, fvs, mks, ws=None, short=0, single=False, stream=None):
    """crfp_<wiring>_forward_batch on [n, t, ...] arrays -> (return code, out, status words, workspace).  ws: reuse this workspace as it is;
    short: bytes to understate its size by."""
    import torch
    from crfp_amd import engine as E
    dev = eng.device
    n, t, _, h, w = lrs.shape
    T = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lrs, fvs, mk8 = T(lrs), T(fvs), T(mks).view(torch.uint8)
    nbytes = eng._call("batch_workspace_bytes")(n, t, h, w)
    if ws is None:
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    assert ws.numel() >= nbytes
    out = torch.full((n, t, 1 if eng.y_only else 3, 8 * h, 8 * w), float("nan"), dtype=torch.float32, device=dev)
    eng.single_stream = single
    fwd = eng._call("forward_batch")
    with torch.cuda.device(dev), torch.cuda.stream(stream or torch.cuda.current_stream()):
        rc = fwd(eng.packed.data_ptr(), eng._flags(), lrs.data_ptr(), fvs.data_ptr(), mk8.data_ptr(), out.data_ptr(), n, t, h, w, ws.data_ptr(),
                 nbytes - short, E._stream())
    eng.single_stream = False
    off = eng._call("batch_status_offset")(n, t, h, w)
    return rc, out, ws[off:off + 4 * n].view(torch.int32), ws, (lrs, fvs, mk8)


def digest(rc, out, words):
    import torch
    torch.cuda.synchronize()
    assert rc == 0, rc
    o = out.cpu().numpy()
    return {"frames": [[hashlib.sha256(o[b, i].tobytes()).hexdigest()[:16] for i in range(o.shape[1])] for b in range(o.shape[0])],
            "status": [int(v) for v in words.cpu().numpy()], "finite": bool(np.isfinite(o).all())}


def run(wiring, storage, y_only, n, t, h, w, seed=11, **kw):
    eng = engine(wiring, storage, y_only)
    rc, out, words, _, _ = call(eng, *clip(seed, n, t, h, w), **kw)
    return digest(rc, out, words)


def cases():
    """{case id: thunk}.  Ids: base.* (every wiring, storage and geometry at t = 3), t.* (frame counts around every rule boundary, at 8 x 16),
    and the single-purpose ones."""
    c = {}
    for wiring in MODELS:
        for storage in ("f32", "bf16"):
            for y_only in ((False, True) if wiring == "dsv" else (False,)):
                for h, w in ((20, 36), (33, 47)):
                    c[f"base.{wiring}.{storage}.y{int(y_only)}.{h}x{w}"] = lambda a=(wiring, storage, y_only, 1, 3, h, w): run(*a)
    for storage in ("f32", "bf16"):
        for n, t in ((1, 1), (1, 2), (1, 3), (1, 8), (1, 9), (1, 17), (2, 3), (2, 17)):
            c[f"t.dsv.{storage}.n{n}.t{t}"] = lambda a=("dsv", storage, False, n, t, 8, 16): run(*a)
            c[f"t1s.dsv.{storage}.n{n}.t{t}"] = lambda a=("dsv", storage, False, n, t, 8, 16): run(*a, single=True)
    for n, t in ((1, 9), (2, 3), (1, 17)):      # the fovea encoder's temporaries and level slots over a reused slot set
        c[f"t.cra.f32.n{n}.t{t}"] = lambda a=("cra", "f32", False, n, t, 8, 16): run(*a)
        c[f"t1s.cra.f32.n{n}.t{t}"] = lambda a=("cra", "f32", False, n, t, 8, 16): run(*a, single=True)
    c["swap.dsv.f32"] = swap_case
    c["reuse.dsv.f32"] = lambda: reuse_case("dsv")
    c["reuse.cra.f32"] = lambda: reuse_case("cra")
    c["ovf_lr.dsv.f32"] = lambda: overflow_case("lr")
    c["ovf_fv.dsv.f32"] = lambda: overflow_case("fv")
    c["short.dsv.f32"] = short_case
    c["flight.dsv.f32"] = flight_case
    return c


def swap_case():
    """Frames 1 and 2 trade masks (nothing else changes): what the engine computes for them must change, frame 0 must not."""
    eng = engine("dsv", "f32", False)
    lrs, fvs, mks = clip(11, 1, 3, 20, 36)
    mks = mks[:, [0, 2, 1]]
    rc, out, words, _, _ = call(eng, lrs, fvs, mks)
    return digest(rc, out, words)


def reuse_case(wiring):
    """A 9-frame clip, then a 3-frame clip on the SAME workspace (every slot now holds the longer clip's frames): the second result."""
    import torch
    eng = engine(wiring, "f32", False)
    big = torch.full((eng._call("batch_workspace_bytes")(1, 9, 8, 16),), 0xFF, dtype=torch.uint8, device=eng.device)
    assert big.numel() >= eng._call("batch_workspace_bytes")(1, 3, 8, 16)
    rc, _, _, _, _ = call(eng, *clip(12, 1, 9, 8, 16), ws=big)
    assert rc == 0
    rc, out, words, _, _ = call(eng, *clip(11, 1, 3, 8, 16), ws=big)
    d = digest(rc, out, words)
    d["fresh"] = run(wiring, "f32", False, 1, 3, 8, 16)
    return d


def overflow_case(where):
    """n = 2, t = 3: one value no fp16 operand holds in frame 1 of clip 1 -- in the LR frame (the range guard of the input conversion) or in the
    fovea frame under the mask (the guard of the launches that consume the frame stack, whose items are (clip, frame))."""
    eng = engine("dsv", "f32", False)
    lrs, fvs, mks = clip(11, 2, 3, 20, 36)
    if where == "lr":
        lrs[1, 1, 0, 5, 7] = OVF
    else:
        y, x = np.argwhere(mks[1, 1, 0])[len(np.argwhere(mks[1, 1, 0])) // 2]
        fvs[1, 1, :, y, x] = 1e30
    rc, out, words, _, _ = call(eng, lrs, fvs, mks)
    import torch
    torch.cuda.synchronize()
    assert rc == 0
    o = out.cpu().numpy()
    return {"status": [int(v) for v in words.cpu().numpy()], "clip0_finite": bool(np.isfinite(o[0]).all()),
            "frames": [[hashlib.sha256(o[b, i].tobytes()).hexdigest()[:16] for i in range(3)] for b in range(2)]}


def short_case():
    eng = engine("dsv", "f32", False)
    res = {}
    for n, t in ((1, 3), (1, 9), (2, 3), (1, 1)):
        rc, _, _, _, _ = call(eng, *clip(11, n, t, 8, 16), short=1)
        res[f"n{n}.t{t}"] = rc
    return res


def flight_case():
    """Two clip calls in flight on two streams of one host thread, each with its own workspace and output (they share the thread's side stream
    and its events): both results."""
    import torch
    eng = engine("dsv", "f32", False)
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    clips = [clip(11, 1, 9, 8, 16), clip(12, 1, 9, 8, 16)]
    torch.cuda.synchronize()
    res = []
    for _ in range(2):     # twice: the second round re-records every event of the first
        res = [call(eng, *clips[k], stream=s[k]) for k in range(2)]
    torch.cuda.synchronize()
    return {"a": digest(*res[0][:3]), "b": digest(*res[1][:3]), "a_alone": run("dsv", "f32", False, 1, 9, 8, 16, seed=11),
            "b_alone": run("dsv", "f32", False, 1, 9, 8, 16, seed=12)}


def main(argv):
    out_path = argv[1]
    only = argv[argv.index("--only") + 1].split(",") if "--only" in argv else None
    import torch
    if os.environ.get("PREWORK_ORDER") == "per_frame":
        from crfp_amd import _lib
        assert _lib.lib().crfp_lab_prework_groups(0) == 1      # AttributeError on the product library: it has no such order
    res = {}
    with torch.no_grad():
        for cid, thunk in cases().items():
            if only is None or any(cid.startswith(p) for p in only):
                res[cid] = thunk()
    with open(out_path, "w") as f:
        json.dump(res, f)
    print(f"prework_cases: {len(res)} cases -> {out_path}")


if __name__ == "__main__":
    main(sys.argv)
