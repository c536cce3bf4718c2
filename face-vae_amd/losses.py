"""Loss modules with the reference call signatures (losses.py of Luh1124/face-vae)."""
from __future__ import annotations

import math

import torch
from torch import nn

from . import ops


class KLDivergenceLoss(nn.Module):
    """losses.py:385-393: mean(-0.5 - logstd + 0.5 mu^2 + 0.5 exp(2 logstd)); called as
    KLDivergenceLoss()((mu, logstd))."""

    def forward(self, kl):
        return ops.kl_loss(kl[0], kl[1])


class ReconLoss(nn.Module):
    """losses.py:396-403: nn.MSELoss()(Rec[0], Rec[1]); called as ReconLoss()((target, pred))."""

    def forward(self, Rec):
        return ops.mse_loss(Rec[0], Rec[1])


class L1Loss(nn.Module):
    """nn.L1Loss (mean |a - b|): the pixel term of PerceptualLoss (losses.py:128,135)."""

    def forward(self, input, target):
        return ops.l1_loss(input, target)


class GANLoss(nn.Module):
    """Hinge GAN loss (losses.py:154-179) on the discriminator's [N, 1, h, w] fp32 logits (a few
    KB: plain torch ops).  GANLoss()(dis_output, t_real, dis_update):
      discriminator update, real:  -mean(min(x - 1, 0))
      discriminator update, fake:  -mean(min(-x - 1, 0))
      generator update:            -mean(x)"""

    def forward(self, dis_output, t_real, dis_update=True):
        x = dis_output.float()
        if not dis_update:
            return -torch.mean(x)
        v = x - 1 if t_real else -x - 1
        return -torch.mean(torch.clamp(v, max=0))


class FeatureMatchingLoss(nn.Module):
    """losses.py:182-195, called as FeatureMatchingLoss()(fake_features, real_features) with the
    discriminator's feature lists.  The reference loops `fake_features[i][j]` over the SAMPLES j of
    layer i and adds mean|.| of each sample's slice with weight 1 / n_layers; the per-sample
    means of equal-sized slices sum to B times the layer's mean, so the value is
    (B / n_layers) * sum_i mean|fake_i - real_i.detach()|, not the plain mean.  It is computed
    in that closed form: one L1 kernel pass (ops.l1_loss) per layer."""

    def forward(self, fake_features, real_features):
        num_d = len(fake_features)
        loss = None
        for f, r in zip(fake_features, real_features):
            if not f.is_cuda:
                raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
            t = ops.l1_loss(f, r.detach()) * (f.shape[0] / num_d)
            loss = t if loss is None else loss + t
        return loss


class HeadPoseLoss(nn.Module):
    """losses.py:224-231: the mean of the three L1 distances between the estimated and the
    (detached) teacher angles, in degrees.  [N] tensors: plain torch ops on any device."""

    def forward(self, yaw, pitch, roll, real_yaw, real_pitch, real_roll):
        loss = ((yaw - real_yaw.detach()).abs().mean() + (pitch - real_pitch.detach()).abs().mean()
                + (roll - real_roll.detach()).abs().mean()) / 3
        return loss / math.pi * 180


from .perceptual import PerceptualLoss  # noqa: E402,F401  (losses.py:123-151)
