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


class ContrastiveLoss_linear(nn.Module):
    """losses.py:243-278, called as ContrastiveLoss_linear(mode=...)(f1, f2) on the two 4 x 4 codes
    EFE_conv5 returns (x_c, x_a_c; trainer.py:261 uses mode="non-direction").  mode "direction": one
    minus the mean cosine similarity of the flattened features.  Any other mode: a three-layer
    `projection` (Linear without bias, BatchNorm1d, ReLU, twice; then Linear with a frozen bias and
    a BatchNorm1d without affine) and a two-layer `predictor` (Linear without bias, BatchNorm1d, ReLU,
    Linear), each applied to both inputs, and one minus the mean of the two cosine similarities
    between a prediction and the other input's detached projection.  Reference signature, state-dict
    keys (25 by default) and init draws; projection[6].bias.requires_grad is False.

    Plain torch ops on GPU tensors, like KeypointPriorLoss: N x 512 GEMMs on a batch of codes are
    not a hot path, so there is no HIP kernel here.  The features are flattened in NCHW order
    whatever their memory layout and computed in fp32.  nn.BatchNorm1d in a single process only:
    there is no SyncBN for the projector."""

    def __init__(self, in_dim=512, hid_1_dim=512, out_1_dim=512, hid_2_dim=512, out_2_dim=512, mode="direction"):
        super().__init__()
        self.criterion = nn.CosineSimilarity(dim=1)
        self.mode = mode
        if mode == "direction":
            return
        # construction order = the reference's RNG draw order
        self.projection = nn.Sequential(
            nn.Linear(in_dim, hid_1_dim, bias=False), nn.BatchNorm1d(hid_1_dim), nn.ReLU(inplace=True),
            nn.Linear(hid_1_dim, hid_1_dim, bias=False), nn.BatchNorm1d(hid_1_dim), nn.ReLU(inplace=True),
            nn.Linear(hid_1_dim, out_1_dim, bias=True), nn.BatchNorm1d(out_1_dim, affine=False))
        self.projection[6].bias.requires_grad = False        # a bias in front of a BN: kept, never trained
        self.predictor = nn.Sequential(
            nn.Linear(out_1_dim, hid_2_dim, bias=False), nn.BatchNorm1d(hid_2_dim), nn.ReLU(inplace=True),
            nn.Linear(hid_2_dim, out_2_dim))

    def forward(self, f1, f2):
        f1 = f1.float().reshape(f1.shape[0], -1)
        f2 = f2.float().reshape(f2.shape[0], -1)
        if self.mode == "direction":
            return 1 - self.criterion(f1, f2).mean()
        z1, z2 = self.projection(f1), self.projection(f2)
        p1, p2 = self.predictor(z1), self.predictor(z2)
        return 1 - 0.5 * (self.criterion(p1, z2.detach()).mean() + self.criterion(p2, z1.detach()).mean())


from .perceptual import PerceptualLoss  # noqa: E402,F401  (losses.py:123-151)
