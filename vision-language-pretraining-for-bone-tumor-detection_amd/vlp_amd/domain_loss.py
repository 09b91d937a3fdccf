"""The baselines' weighted BCE + CORAL loss as one device op (csrc/domain_loss_ops.hip;
reference FusionModule.py:341-390 and coral_loss/coral.py:5-37).

domain_codes maps the batch's dataset names to the op's per-row codes; DomainLossFn is
the autograd function FusionModule / OnlyImagingModule call with `loss_on_device=True`.
The op forms the two domains' second-moment difference, its squared Frobenius norm, the
BCE and both gradients in fp64 in a fixed summation order; where a domain has fewer than
two rows, or lambda is 0, the CORAL term and its gradient are exactly 0 -- decided on the
device from the codes, so the host neither counts nor indexes anything.
"""
from __future__ import annotations

from typing import Sequence

import torch

INTERNAL, BTXRD, OTHER = 0, 1, 2


def domain_codes(dataset: Sequence[str]) -> torch.Tensor:
    """uint8 [N] on the host (pinned where a GPU is present, for the non-blocking upload):
    "INTERNAL" -> 0, "BTXRD" -> 1, anything else -> 2."""
    codes = torch.tensor([INTERNAL if d == "INTERNAL" else (BTXRD if d == "BTXRD" else OTHER) for d in dataset],
                         dtype=torch.uint8)
    return codes.pin_memory() if torch.cuda.is_available() and codes.numel() else codes


class DomainLossFn(torch.autograd.Function):
    """total, cls, coral = f(features [N, D] fp32, logits [N] fp32, labels [N], codes [N] uint8,
    w0, w1, coral_lambda): 0-dim fp32 tensors on the features' device.  The forward is one
    vlp_domain_loss call that also forms d coral / d features and d cls / d logits when an input
    needs a gradient; the backward scales them by the gradient of `total`.  cls and coral are
    for logging (non-differentiable).  Nothing is read back and no branch looks at device data."""

    @staticmethod
    def forward(ctx, features, logits, labels, codes, w0, w1, coral_lambda):
        from . import ops
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        out, g_feat, g_logits = ops.domain_loss(features, logits, labels, codes, w0, w1, coral_lambda, grad=need)
        ctx.grads = (g_feat, g_logits)
        losses = out.float()
        total, cls, coral = losses[0], losses[1], losses[2]
        ctx.mark_non_differentiable(cls, coral)
        return total, cls, coral

    @staticmethod
    def backward(ctx, d_total, d_cls, d_coral):
        g_feat, g_logits = ctx.grads
        ctx.grads = None
        gf = g_feat * d_total if ctx.needs_input_grad[0] else None
        gl = g_logits * d_total if ctx.needs_input_grad[1] else None
        return gf, gl, None, None, None, None, None


def domain_loss(features, logits, labels, dataset, label_weights, coral_lambda):
    """FusionModule._compute_loss on the device: (total, cls, coral).  features [N, D] or
    [N, D, h, w] (pooled by the spatial mean, the identity on the towers' 1 x 1 maps); dataset the
    rows' names or a ready uint8 code tensor; label_weights two host floats."""
    pooled = features.mean((2, 3)) if features.dim() == 4 else features
    if pooled.dtype != torch.float32:
        pooled = pooled.float()
    if pooled.stride(1) != 1 or (pooled.shape[0] > 1 and pooled.stride(0) < pooled.shape[1]):
        pooled = pooled.contiguous()
    z = logits.reshape(-1)
    if z.dtype != torch.float32:
        z = z.float()
    dev = pooled.device
    y = labels.to(dev, non_blocking=True).reshape(-1)
    if y.dtype not in (torch.int64, torch.int32, torch.uint8, torch.bool):
        y = y.long()
    codes = dataset if torch.is_tensor(dataset) else domain_codes(dataset)
    codes = codes.to(dev, non_blocking=True)
    return DomainLossFn.apply(pooled, z.contiguous(), y.contiguous(), codes, float(label_weights[0]),
                              float(label_weights[1]), float(coral_lambda))
