"""Child process of test_gpu_conv_pair_f32.py: CRFP_CONV_PAIR is read once per process, so each setting runs in a process of its own.

argv: h w (LR size of the 3-frame clips).  Prints one line per run: "RUN <name> <sha256 of the output> <overflowed>", for the four
wirings' clip calls (fp32 storage) and, for DSV, a lock-step batch of two clips and three streamed frames."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from crfp_amd import synth  # noqa: E402
from crfp_amd.model import CRFP  # noqa: E402

h, w = int(sys.argv[1]), int(sys.argv[2])
dev = torch.device("cuda:0")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731


def model(cls):
    m = getattr(CRFP, cls)(dev, mid_channels=32)
    sd = synth.make_state_dict_like({k: tuple(v.shape) for k, v in m.state_dict().items()}, 7)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def report(name, out, m, stream=False):
    print("RUN %s %s %d" % (name, hashlib.sha256(np.ascontiguousarray(out.cpu().numpy()).tobytes()).hexdigest(), int(bool(m.engine().overflowed(stream=stream)))), flush=True)


clip = tuple(T(a) for a in synth.make_clip(4321, 1, 3, h, w, fv_size=48))
two = tuple(T(a) for a in synth.make_clip(4322, 2, 3, h, w, fv_size=48))
with torch.no_grad():
    for name, cls in (("dsv", "CRFP_DSV"), ("cra", "CRFP_DSV_CRA"), ("simple", "CRFP_simple"), ("dense", "CRFP")):
        m = model(cls)
        report(name, m(*clip), m)
        if name == "dsv":
            report("dsv_batch2", m(*two), m)
            m.clear_states()
            report("dsv_stream", m.forward_stream(*clip), m, stream=True)
