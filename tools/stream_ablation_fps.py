"""frames/s of the one-frame-per-call schedules of the reference's four streaming models -- MRCF_simple_v13 (CRFP_simple), MRCF_simple_v15
(CRFP), MRCF_simple_v18 (CRFP_DSV) and MRCF_simple_v18_cra (CRFP_DSV_CRA), mid_channels 32 -- at BASELINE config 3's frame size (180 x 320 ->
1440 x 2560), fp32 and bf16 storage, with and without inputs_resident, in one process on one box.  The frames sit on the device before the
timed loop (a decoded video held in HBM); each pass streams `calls` frames, cycling over 10 distinct ones, after clear_states().  Behind the
CRA rows, what its stream is compared with: the wiring's clip engine as frames/s of a 7-frame clip, and the composed stream of the same model.
usage: python tools/stream_ablation_fps.py [calls] [passes]"""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from crfp_amd import synth  # noqa: E402
from crfp_amd.model import CRFP  # noqa: E402


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda:0")
    lrs, fvs, mks = (torch.from_numpy(a).to(dev) for a in synth.make_clip(3, 1, 10, 180, 320, fv_size=96))
    mks = mks.bool()
    torch.cuda.synchronize()
    frames = [(lrs[:, i:i + 1], fvs[:, i:i + 1], mks[:, i:i + 1]) for i in range(10)]

    def timed(fn, n, frames_per_call=1):   # fn(i) n times per pass, after clear(); pass 0 is the warm-up (packing, workspace, side stream)
        rates = []
        with torch.no_grad():
            for p in range(passes + 1):
                m.clear_states()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    fn(i)
                torch.cuda.synchronize()
                if p:
                    rates.append(n * frames_per_call / (time.perf_counter() - t0))
        return rates

    for cls in ("MRCF_simple_v13", "MRCF_simple_v15", "MRCF_simple_v18", "MRCF_simple_v18_cra"):
        m = getattr(CRFP, cls)(dev, mid_channels=32)
        sd = synth.make_state_dict(7) if cls.endswith("v18") else synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, 7)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        m = m.to(dev).eval()
        for storage in ("f32", "bf16"):
            for resident in (False, True):
                m.storage, m.inputs_resident = storage, resident
                rates = timed(lambda i: m(*frames[i % 10]), calls)
                assert not m.engine().overflowed(stream=True)
                print(f"{cls} storage={storage} resident={int(resident)} calls={calls} frames_per_sec median={statistics.median(rates):.1f} "
                      f"passes={[round(r, 1) for r in rates]}", flush=True)
        if not cls.endswith("cra"):
            continue
        m.inputs_resident = False
        clip = CRFP.CRFP_DSV_CRA(dev, mid_channels=32)
        clip.load_state_dict(m.state_dict(), strict=True)
        clip = clip.to(dev).eval()
        for storage in ("f32", "bf16"):
            clip.storage = storage
            rates = timed(lambda i: clip(lrs[:, :7], fvs[:, :7], mks[:, :7]), max(1, calls // 7), 7)
            print(f"CRFP_DSV_CRA clip engine storage={storage} 7-frame clips frames_per_sec median={statistics.median(rates):.1f} "
                  f"passes={[round(r, 1) for r in rates]}", flush=True)
        m.has_engine = lambda: False   # the per-operator composition with the state carried between calls (fp32 tensors)
        rates = timed(lambda i: m(*frames[i % 10]), max(1, calls // 4))
        print(f"{cls} composed stream calls={max(1, calls // 4)} frames_per_sec median={statistics.median(rates):.1f} "
              f"passes={[round(r, 1) for r in rates]}", flush=True)


if __name__ == "__main__":
    main()
