"""Cases of tests/test_gpu_dcn_fused_tail.py: the 8x state warp riding in the idle last-round CUs of the fused offset head + DCN launches
(crfp_amd/csrc/dcn_fused.inc, DcnWarpPlan).

Operator level (imported by the test, product library): crfp_dcn_tail_probe on device buffers laid out here in the build's storage format.  The
fused kernel is compared with itself (the same launch without a plan), so the offset feature image and the packed weight images are random
finite fp16 / bf16 values, not a packed model: what matters is that the launch does all its work while the warp workgroups run beside it.

Engine level (run as a script, once per library):

    python tests/helpers/dcn_tail_cases.py OUT.json

OUT.json: {case id: {"frames": [...sha256...], "status": [...], "fetch": {name: sha256}}}.  WARP_TAIL_BANDS=<n> in this script's environment (lab
library only) sets the number of fused launches that carry a band of the warp through crfp_lab_warp_tail_bands(n) before the first call: 0 keeps
the stand-alone warp launch.  The product carries the warp in all three fused launches of a frame."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GUARD = 4096        # bytes behind an output that nothing may touch
GUARD_BYTE = 0xA5
FLOW_PX = 9.0       # |flow| of the ordinary vectors of the warp's flow field


class OpCase:
    """The device buffers of one probe geometry: n items of an h x w DCN map and a 4h x 4w warp, every tensor with its own batch stride."""

    def __init__(self, storage, n, h, w, seed=3):
        import torch
        self.storage, self.n, self.h, self.w = storage, n, h, w
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(seed)
        act = torch.bfloat16 if storage == "bf16" else torch.float32
        esz = 2 if storage == "bf16" else 4
        H8, W8 = 4 * h, 4 * w
        rnd = lambda *s: torch.randn(*s, generator=g)

        def p4(nq, hh, ww, extra):
            """[guard | n x (nq planes of (hh + 1) x (ww + 1) quads, zero pad row and column, + extra zero elements)] -> (buffer, offset of plane 0, stride)"""
            stride = nq * (hh + 1) * (ww + 1) * 4 + extra
            guard = (ww + 1) * 4 + 4      # one pad row + one quad, in elements
            buf = torch.zeros(guard + n * stride, dtype=act)
            for b in range(n):
                v = buf[guard + b * stride: guard + b * stride + nq * (hh + 1) * (ww + 1) * 4].view(nq, hh + 1, ww + 1, 4)
                v[:, :hh, :ww] = rnd(nq, hh, ww, 4).to(act)
            return buf.to(dev), guard * esz, stride

        # the offset feature image: 8 planes [h][w] of 8 fp16 (fp32 build) / of bf16 quads (bf16 build): 32 h w "floats" / elements per item
        self.feat_b = 32 * h * w + 64
        if storage == "bf16":
            self.feat = rnd(n * self.feat_b).to(torch.bfloat16).to(dev)
        else:
            self.feat = rnd(n * self.feat_b * 2).to(torch.float16).to(dev)      # two fp16 per float of stride
        self.flow_b = 2 * h * w + 6
        self.flow = (2.0 * rnd(n * self.flow_b)).to(dev)
        wdt = torch.bfloat16 if storage == "bf16" else torch.float16
        self.wconv = (0.05 * rnd((7 if storage == "bf16" else 14) * 1152 * 8)).to(wdt).to(dev)
        self.bconv = (0.1 * rnd(224)).to(dev)
        self.wdcn = (0.05 * rnd(36 * 64 * 8)).to(torch.float16).to(dev)
        self.bdcn = (0.1 * rnd(32)).to(dev)
        self.x, self.x_off, self.x_b = p4(8, h, w, 40)
        self.src, self.src_off, self.src_b = p4(1, H8, W8, 24)
        self.out_b = 32 * h * w + 128
        self.dst_b = 4 * H8 * W8 + 32
        self.wflow_b = 2 * H8 * W8 + 10
        f8 = FLOW_PX * (2.0 * torch.rand(n, H8, W8, 2, generator=g) - 1.0)
        far = [(-1e4, 0.0), (0.0, 1e4), (3e9, -3e9), (-float(W8 + 40), float(H8 + 40)), (float(W8), -1.5), (-1.0, float(H8) - 0.5)]
        for b in range(n):        # a few vectors far outside the image, spread over the map (first and last pixel among them)
            for k, v in enumerate(far):
                f8[b, (k * (H8 - 1)) // (len(far) - 1), (k * (W8 - 1)) // (len(far) - 1)] = torch.tensor(v)
        wf = torch.zeros(n * self.wflow_b)
        for b in range(n):
            wf[b * self.wflow_b: b * self.wflow_b + 2 * H8 * W8] = f8[b].reshape(-1)
        self.wflow = wf.to(dev)
        self.esz, self.dev = esz, dev

    def run(self, bands):
        """One probe call on fresh outputs (0xFF bytes, guard bytes behind) -> (report, out bytes, dst bytes, status words), guards included."""
        import torch
        from crfp_amd import _lib
        lib = _lib.lib()
        sfx = "_bf16" if self.storage == "bf16" else ""
        out = torch.full((self.n * self.out_b * self.esz + GUARD,), 0xFF, dtype=torch.uint8, device=self.dev)
        dst = torch.full((self.n * self.dst_b * self.esz + GUARD,), 0xFF, dtype=torch.uint8, device=self.dev)
        out[-GUARD:] = GUARD_BYTE
        dst[-GUARD:] = GUARD_BYTE
        status = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        a = _lib.DcnTailArgs()
        a.feat, a.flow, a.wconv, a.bconv = self.feat.data_ptr(), self.flow.data_ptr(), self.wconv.data_ptr(), self.bconv.data_ptr()
        a.x, a.wdcn, a.bdcn = self.x.data_ptr() + self.x_off, self.wdcn.data_ptr(), self.bdcn.data_ptr()
        a.out, a.status = out.data_ptr(), status.data_ptr()
        a.warp_src, a.warp_flow, a.warp_dst = self.src.data_ptr() + self.src_off, self.wflow.data_ptr(), dst.data_ptr()
        a.feat_b, a.flow_b, a.x_b, a.out_b = self.feat_b, self.flow_b, self.x_b, self.out_b
        a.warp_src_b, a.warp_flow_b, a.warp_dst_b = self.src_b, self.wflow_b, self.dst_b
        a.n, a.h, a.w, a.bands = self.n, self.h, self.w, bands
        r = _lib.DcnTailReport()
        torch.cuda.synchronize()
        with torch.cuda.device(self.dev):
            _lib.check(getattr(lib, "crfp_dcn_tail_probe" + sfx)(C.byref(a), C.byref(r), None), "crfp_dcn_tail_probe" + sfx)
        torch.cuda.synchronize()
        return {k: getattr(r, k) for k, _ in r._fields_}, out, dst, status

    def written(self, buf, stride, count):
        """mask [bytes] of the bytes of an output the launch owns: `count` elements at the head of every item's stride"""
        import torch
        m = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
        for b in range(self.n):
            m[b * stride * self.esz: (b * stride + count) * self.esz] = True
        return m


# ---------------------------------------------------------------- engine level
def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def engine_cases():
    import torch
    from tests.helpers import prework_cases as pc
    res = {}
    for wiring in ("dsv", "cra"):
        for storage in ("f32", "bf16"):
            eng = pc.engine(wiring, storage, False)
            for h, w in ((20, 36), (33, 47)):
                lrs, fvs, mks = pc.clip(11, 1, 3, h, w)
                T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
                out = eng.forward(T(lrs), T(fvs), T(mks))
                torch.cuda.synchronize()
                ws = eng._workspace(3, h, w)
                off = eng._call("batch_status_offset")(1, 3, h, w)
                d = {"frames": [_sha(out[0, i]) for i in range(3)], "status": [int(v) for v in ws[off:off + 4].view(torch.int32).cpu()],
                     "finite": bool(torch.isfinite(out).all()), "fetch": {}}
                for name in ("prevhrw", "aligned", "state_hr"):
                    d["fetch"][name] = _sha(eng.debug_fetch(name, 3, h, w))
                res[f"clip.{wiring}.{storage}.{h}x{w}"] = d
            # a lock-step batch of two clips
            lrs, fvs, mks = pc.clip(12, 2, 3, 20, 36)
            rc, out, words, _, _ = pc.call(eng, lrs, fvs, mks)
            res[f"batch2.{wiring}.{storage}"] = pc.digest(rc, out, words)
            # three streamed frames, one per call
            lrs, fvs, mks = pc.clip(13, 1, 3, 20, 36)
            seng = eng
            if wiring == "cra":      # the clip handle of this wiring does not stream: the same weights in the streaming handle
                from crfp_amd.model import CRFP
                sm = CRFP.MRCF_simple_v18_cra(eng.device, mid_channels=32, y_only=False)
                sm.load_state_dict(pc._engines[(wiring, storage, False)][0].state_dict(), strict=True)
                sm.storage = storage
                seng = sm.to(eng.device).eval().engine()
            seng.clear_states()
            frames = []
            for i in range(3):
                o = seng.stream_frame(torch.from_numpy(lrs[0, i]).to(eng.device), torch.from_numpy(fvs[0, i]).to(eng.device),
                                     torch.from_numpy(mks[0, i]).to(eng.device))
                torch.cuda.synchronize()
                frames.append(_sha(o))
            off = seng._call("batch_status_offset")(1, 1, 20, 36)
            res[f"stream.{wiring}.{storage}"] = {"frames": frames, "status": [int(v) for v in seng._stream_ws[off:off + 4].view(torch.int32).cpu()]}
    return res


def main(argv):
    import torch
    if os.environ.get("WARP_TAIL_BANDS"):
        from crfp_amd import _lib
        assert _lib.lib().crfp_lab_warp_tail_bands(int(os.environ["WARP_TAIL_BANDS"])) == 3      # AttributeError on the product library: no such switch
    with torch.no_grad():
        res = engine_cases()
    with open(argv[1], "w") as f:
        json.dump(res, f)
    print(f"dcn_tail_cases: {len(res)} cases -> {argv[1]}")


if __name__ == "__main__":
    main(sys.argv)
