"""The reference's ``loss/loss.py`` interface: ``charbonnier_loss``, ``CharbonnierLoss`` and ``get_loss_dict``, same signatures and values.

On CUDA/HIP tensors ``reduction='mean'`` and ``'sum'`` come from one fused pass (``ops.charbonnier``: per-sample float64 sums, backward in
one more pass), so the three or four full-size intermediates the torch formula keeps alive for autograd are never made.
``reduction='none'`` (an elementwise result) and CPU tensors use the torch formula of the reference (loss/loss.py:7-68,115-124).
"""
import torch
import torch.nn as nn

from crfp_amd import ops

_REDUCTIONS = ('none', 'mean', 'sum')
_DIV_EPS = 1e-12   # loss/loss.py:58: "small value to prevent division by zero"


def _torch_formula(pred, target, weight, reduction, sample_wise, eps):
    """loss/loss.py:26-68 on sqrt((pred - target)^2 + eps), operation for operation."""
    loss = torch.sqrt((pred - target) ** 2 + eps)
    if weight is not None:
        assert weight.dim() == loss.dim()
        assert weight.size(1) == 1 or weight.size(1) == loss.size(1)
        loss = loss * weight
    if weight is None or reduction == 'sum':
        return loss if reduction == 'none' else (loss.mean() if reduction == 'mean' else loss.sum())
    if reduction == 'mean':
        if weight.size(1) == 1:
            weight = weight.expand_as(loss)
        if sample_wise:
            weight = weight.sum(dim=[1, 2, 3], keepdim=True)
            return (loss / (weight + _DIV_EPS)).sum() / weight.size(0)
        return loss.sum() / (weight.sum() + _DIV_EPS)
    return loss


def charbonnier_loss(pred, target, weight=None, reduction='mean', sample_wise=False, eps=1e-12):
    """Charbonnier loss sqrt((pred - target)^2 + eps) with the reference's masked reduction (the ``masked_loss`` decorator of
    loss/loss.py:70-124): 'none', 'sum', or 'mean' -- the plain mean without a weight, sum / (sum of the weight + 1e-12) with one, per
    sample and then averaged with ``sample_wise``.  The result has pred's dtype."""
    if reduction not in _REDUCTIONS:
        raise ValueError(f'Unsupported reduction mode: {reduction}. Supported ones are: {list(_REDUCTIONS)}')
    if reduction == 'none' or not pred.is_cuda:
        return _torch_formula(pred, target, weight, reduction, sample_wise, eps)
    if weight is not None:
        assert weight.dim() == pred.dim()
        assert weight.size(1) == 1 or weight.size(1) == pred.size(1)
    sums = ops.charbonnier(pred, target, weight, eps)          # [n, 2] float64: (sum loss * w, sum w) per sample
    num, den = sums[:, 0], sums[:, 1].detach()
    if reduction == 'sum':
        out = num.sum()
    elif weight is None:
        out = num.sum() / den.sum()                            # the element count
    elif sample_wise:
        out = (num / (den + _DIV_EPS)).sum() / sums.shape[0]
    else:
        out = num.sum() / (den.sum() + _DIV_EPS)
    return out.to(pred.dtype)


class CharbonnierLoss(nn.Module):
    """loss/loss.py:126-173: ``loss_weight * charbonnier_loss(pred, target, weight, ...)``."""

    def __init__(self, loss_weight=1.0, reduction='mean', sample_wise=False, eps=1e-12):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise ValueError(f'Unsupported reduction mode: {reduction}. Supported ones are: {list(_REDUCTIONS)}')
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.sample_wise = sample_wise
        self.eps = eps

    def forward(self, pred, target, weight=None, **kwargs):
        return self.loss_weight * charbonnier_loss(pred, target, weight, eps=self.eps, reduction=self.reduction,
                                                   sample_wise=self.sample_wise)


def get_loss_dict(args, logger):
    """loss/loss.py:177-184."""
    if abs(args.rec_w - 0) <= 1e-8:
        raise SystemExit('NotImplementError: ReconstructionLoss must exist!')
    return {'cb_loss': CharbonnierLoss()}
