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


class EquivarianceLoss(nn.Module):
    """losses.py:198-205: mean |kp_d[..., :2] - reverse_kp|, the detected keypoints of a warped
    image against the warp applied to the original's.  [N, K, 3] and [N, K, 2] tensors: plain torch
    ops on any device."""

    def forward(self, kp_d, reverse_kp):
        return (kp_d[:, :, :2] - reverse_kp).abs().mean()


class KeypointPriorLoss(nn.Module):
    """losses.py:208-221: keypoints closer than sqrt(Dt) repel (a hinge on the squared pairwise
    distances, the K diagonal terms of Dt each subtracted again) and the mean depth is pulled to
    zt.  The distances are torch.cdist(...).square(), not a squared difference: the gradient at the
    zero diagonal is then what torch gives the reference.  Plain torch ops on any device."""

    def __init__(self, Dt=0.1, zt=0.33):
        super().__init__()
        self.Dt, self.zt = Dt, zt

    def forward(self, kp_d):
        dist = torch.cdist(kp_d, kp_d).square()
        hinge = torch.max(0 * dist, self.Dt - dist).sum((1, 2)).mean()
        depth = (kp_d[:, :, 2].mean(1) - self.zt).abs().mean()
        return hinge + depth - kp_d.shape[1] * self.Dt


class DeformationPriorLoss(nn.Module):
    """losses.py:234-240: mean |delta_d| of the expression deformations.  Plain torch ops."""

    def forward(self, delta_d):
        return delta_d.abs().mean()


from .perceptual import PerceptualLoss  # noqa: E402,F401  (losses.py:123-151)
