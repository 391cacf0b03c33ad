"""Training rig for CRFP_DSV on the HIP operators: the counterpart of the reference's ``Trainer.train_basicvsr`` (trainer.py:120-149 the
optimizer and the cosine settings, :206-293 the loop, :50-83 and :596-626 the cosine rule).

    python -m crfp_amd.trainrig --iters N --h H --w W --frames T [--y_only]

trains on synthetic clips (crfp_amd.synth: the HR target is the scene ``make_clip`` downsamples) and prints the loss per iteration.
"""
import argparse
import os
from math import cos, pi

import torch

from crfp_amd import option, synth
from crfp_amd.loss import get_loss_dict

PERIODS = (600000,)      # trainer.py:123-125
MIN_LR = 1e-7
RESTART_WEIGHTS = (1,)
FLOW_FREEZE_ITERS = 5000   # trainer.py:223-229


def get_position_from_periods(iteration, cumulative_periods):
    """trainer.py:50-67: the index of the first cumulative period the iteration lies in front of."""
    for i, period in enumerate(cumulative_periods):
        if iteration < period:
            return i
    raise ValueError(f'Current iteration {iteration} exceeds cumulative_periods {cumulative_periods}')


def annealing_cos(start, end, factor, weight=1):
    """trainer.py:70-83."""
    cos_out = cos(pi * factor) + 1
    return end + 0.5 * weight * (start - end) * cos_out


def cosine_lr(base_lr, cur_iter, periods=PERIODS, min_lr=MIN_LR, restart_weights=RESTART_WEIGHTS):
    """trainer.py:612-622 (get_lr): the learning rate of iteration ``cur_iter`` for a group whose initial rate is ``base_lr``."""
    cumulative = [sum(periods[0:i + 1]) for i in range(len(periods))]
    idx = get_position_from_periods(cur_iter, cumulative)
    nearest_restart = 0 if idx == 0 else cumulative[idx - 1]
    alpha = min((cur_iter - nearest_restart) / periods[idx], 1)
    return annealing_cos(base_lr, min_lr, alpha, restart_weights[idx])


def rgb2yuv(rgb):
    """trainer.py:19-36 (y_only=False)."""
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    return torch.stack([0.299 * r + 0.587 * g + 0.114 * b, -0.147 * r - 0.289 * g + 0.436 * b, 0.615 * r - 0.515 * g - 0.100 * b], dim=1)


def yuv2rgb(yuv):
    """trainer.py:38-48."""
    y, u, v = yuv[:, 0], yuv[:, 1], yuv[:, 2]
    return torch.stack([y + 1.14 * v, y + -0.396 * u - 0.581 * v, y + 2.029 * u], 1)


class TrainRig:
    """Adam over two parameter groups (names containing ``spynet`` at ``lr_rate_flow``, the rest at ``lr_rate``), the flow net frozen
    while ``cur_iter < 5000``, cosine annealing per iteration, the masked Charbonnier loss of crfp_amd.loss."""

    def __init__(self, args, model, loss_all=None):
        if not getattr(model, "_trainable_class", False):
            raise NotImplementedError(f"crfp_amd.trainrig: {type(model).__name__} has no training path; build a CRFP_DSV")
        self.args, self.model = args, model
        self.loss_all = get_loss_dict(args, None) if loss_all is None else loss_all
        self.cur_iter = 0
        model.trainable = True
        named = list(model.named_parameters())
        self.params = [{"params": [p for n, p in named if 'spynet' not in n], "lr": args.lr_rate},
                       {"params": [p for n, p in named if 'spynet' in n], "lr": args.lr_rate_flow}]
        self.optimizer = torch.optim.Adam(self.params, lr=args.lr_rate, betas=(args.beta1, args.beta2), eps=args.eps)
        self.base_lr = [g['lr'] for g in self.optimizer.param_groups]   # before_run (trainer.py:596-603)

    def learning_rates(self, cur_iter=None):
        it = self.cur_iter if cur_iter is None else cur_iter
        return [cosine_lr(b, it) for b in self.base_lr]

    def before_train_iter(self):
        for group, lr in zip(self.optimizer.param_groups, self.learning_rates()):
            group['lr'] = lr

    def train_step(self, batch):
        """One iteration of trainer.py:215-274 on batch = {'LR', 'LR_sr', 'HR', 'Ref', 'Ref_sp'} (device tensors; 'LR_sr' is read with
        ``y_only`` alone: the x8 LR frames whose chroma the luma output is recombined with) -> the loss (a detached device scalar)."""
        lr, hr, ref, ref_sp = batch['LR'], batch['HR'], batch['Ref'], batch['Ref_sp']
        if self.cur_iter < FLOW_FREEZE_ITERS:
            for k, v in self.model.named_parameters():
                if 'spynet' in k:
                    v.requires_grad_(False)
        elif self.cur_iter == FLOW_FREEZE_ITERS:
            self.model.requires_grad_(True)
        self.before_train_iter()
        self.model.train()
        sr = self.model(lrs=lr, fvs=ref, mks=ref_sp)
        B, N, C, H, W = sr.size()
        sr = sr.view(B * N, C, H, W)
        B, N, C, H, W = hr.size()
        hr = hr.view(B * N, C, H, W)
        if self.args.y_only:
            lr_sr = batch['LR_sr']
            B, N, C, H, W = lr_sr.size()
            lr_sr = rgb2yuv(lr_sr.view(B * N, C, H, W))
            sr = yuv2rgb(torch.cat((sr[:, 0:1], lr_sr[:, 1:3]), dim=1))
        loss = self.args.rec_w * self.loss_all['cb_loss'](sr, hr)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        self.cur_iter += 1
        if self.cur_iter % self.args.save_every == 0:
            self.save(0)
        return loss.detach()

    def checkpoint_name(self, epoch=0):
        """trainer.py:279: <save_dir>/model/model_<epoch:05d>_<iter:06d>.pt"""
        return self.args.save_dir.strip('/') + '/model/model_{}_{}.pt'.format(str(epoch).zfill(5), str(self.cur_iter).zfill(6))

    def save(self, epoch=0):
        """The plain state_dict under the reference's file name pattern (trainer.py:277-280)."""
        name = self.checkpoint_name(epoch)
        os.makedirs(os.path.dirname(name), exist_ok=True)
        torch.save({k.replace('module.', ''): v for k, v in self.model.state_dict().items()}, name)
        return name


def synthetic_batch(seed, n, t, h, w, device, fv_size=64):
    """A training batch from crfp_amd.synth: the HR target is the scene the LR frames were downsampled from."""
    from crfp_amd import ops
    lrs, fvs, mks, hrs = (torch.from_numpy(a).to(device) for a in synth.make_clip_hr(seed, n, t, h, w, fv_size=fv_size))
    with torch.no_grad():
        lr_sr = ops.upsample_bilinear(lrs.reshape(n * t, 3, h, w), scale_factor=8).view(n, t, 3, 8 * h, 8 * w)
    return {'LR': lrs, 'LR_sr': lr_sr, 'HR': hrs, 'Ref': fvs, 'Ref_sp': mks}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train CRFP_DSV on synthetic clips through the HIP operators")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--h", type=int, default=32)
    ap.add_argument("--w", type=int, default=32)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--mid_channels", type=int, default=32)
    ap.add_argument("--y_only", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", action="store_true", help="write the state_dict after the last iteration")
    ns, rest = ap.parse_known_args(argv)
    args = option.parse(rest)   # the reference's flags (lr_rate, lr_rate_flow, beta1, beta2, eps, rec_w, save_dir, save_every, ...)
    args.y_only = ns.y_only
    if not torch.cuda.is_available():
        raise SystemExit("crfp_amd.trainrig: needs a HIP device (this build has no CPU path)")
    from crfp_amd.model.CRFP import CRFP_DSV
    dev = torch.device("cuda")
    model = CRFP_DSV(dev, mid_channels=ns.mid_channels, y_only=ns.y_only)
    sd = synth.make_state_dict(ns.seed, ns.mid_channels, ns.y_only)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.to(dev)
    rig = TrainRig(args, model)
    for it in range(ns.iters):
        batch = synthetic_batch(ns.seed + 1 + it, ns.batch, ns.frames, ns.h, ns.w, dev)
        loss = rig.train_step(batch)
        lrs = [g['lr'] for g in rig.optimizer.param_groups]
        print(f"iter {it + 1:6d}  loss {float(loss):.6f}  lr {lrs[0]:.3e}  lr_flow {lrs[1]:.3e}", flush=True)
    if ns.save:
        print("saved", rig.save(0))


if __name__ == "__main__":
    main()
