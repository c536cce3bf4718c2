"""The frozen Hopenet teacher (trainer.py:16-88 of Luh1124/face-vae): the ResNet-50 whose yaw, pitch
and roll are the targets of HeadPoseLoss (`real_yaw, real_pitch, real_roll`, trainer.py:278-280).

`Hopenet(block, layers, num_bins)` keeps the reference's positional signature and the state-dict
keys of the reference class over torchvision's Bottleneck (conv1, bn1, layerL.i.conv{1,2,3},
layerL.i.bn{1,2,3}, layerL.i.downsample.{0,1}, fc_yaw / fc_pitch / fc_roll and the vestigial
fc_finetune; `idx_tensor` is not a buffer), so `hopenet_robust_alpha1.pkl` loads with
load_state_dict.  Construction makes the reference's RNG draws in the reference's order, so a seeded
construction holds the reference's parameters bit for bit.

The net is frozen by construction: it runs in eval mode only, under no_grad, on the folded-BN
inference path of ops_hopenet (three or four launches per bottleneck).  The parameter holders are
plain torch.nn modules; none of them is ever called.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import ops
from . import ops_hopenet as OH
from .modules import _Block


class Bottleneck(nn.Module):
    """Parameter holder in the layout of torchvision.models.resnet.Bottleneck (stride on the 3x3)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


class Hopenet(_Block):
    """forward(x) -> (yaw [N], pitch [N], roll [N]) in radians, fp32, without grad; x is the
    preprocessed NCHW fp32 image batch on the GPU (`preprocess`), sized so that a 7 x 7 plane enters
    the pool (224 x 224).  `teacher_angles(frames)` is forward(preprocess(frames)).  fp8 mode runs
    in bf16."""

    def __init__(self, block=None, layers=(3, 4, 6, 3), num_bins=66):
        if block is not None and getattr(block, "expansion", None) != 4:
            raise NotImplementedError("facevae_amd Hopenet: bottleneck blocks (expansion 4) only; the module brings "
                                      "its own in torchvision's layout")
        layers = list(layers)
        if len(layers) != 4 or min(layers) < 1:
            raise ValueError(f"facevae_amd Hopenet: layers must be four positive block counts (got {layers})")
        super().__init__()
        block = Bottleneck
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AvgPool2d(7)
        self.fc_yaw = nn.Linear(512 * block.expansion, num_bins)
        self.fc_pitch = nn.Linear(512 * block.expansion, num_bins)
        self.fc_roll = nn.Linear(512 * block.expansion, num_bins)
        self.fc_finetune = nn.Linear(512 * block.expansion + 3, 3)      # vestigial in the reference too
        self.n_bins = num_bins
        for m in self.modules():                                         # trainer.py:39-45
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        object.__setattr__(self, "_plan", None)          # (signature, ops_hopenet.FrozenPlan)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    # ------------------------------------------------------------------ the frozen path
    def _signature(self, dtype, device):
        sig = [dtype, device]
        for t in list(self.parameters()) + list(self.buffers()):
            sig.append((t.data_ptr(), t._version, t.device, t.dtype))
        return sig

    def _frozen_plan(self, device):
        """The folded weight images and shifts, rebuilt when a parameter's or buffer's version or
        storage changes (load_state_dict, .to(), an in-place edit) or the compute dtype does."""
        dtype = ops.storage(self.compute_dtype())
        sig = self._signature(dtype, device)
        if self._plan is None or self._plan[0] != sig:
            for t in list(self.parameters()) + list(self.buffers()):
                if t.device != device:
                    raise RuntimeError(f"facevae_amd Hopenet: parameters on {t.device}, input on {device}; move the "
                                       "module to the input's device")
                if t.is_floating_point() and t.dtype != torch.float32:
                    raise RuntimeError("facevae_amd Hopenet: parameters and statistics must be fp32")
            with torch.no_grad():
                object.__setattr__(self, "_plan", (sig, OH.FrozenPlan(self, dtype, device)))
        return self._plan[1]

    def _check(self, x):
        if self.training:
            raise RuntimeError("facevae_amd Hopenet is a frozen teacher: call .eval() (batch statistics are not "
                               "built; the reference calls .eval() before every use)")
        OH._gpu(x, "Hopenet")
        H, W = x.shape[2], x.shape[3]
        if H % 32 or W % 32 or (H // 32, W // 32) != (7, 7):
            raise ValueError(f"facevae_amd Hopenet: the plane entering AvgPool2d(7) must be 7 x 7, i.e. a 224 x 224 "
                             f"input (got {H} x {W}, which leaves {H / 32:g} x {W / 32:g})")

    def preprocess(self, x, size=(224, 224)):
        """F.interpolate(apply_imagenet_normalization(x), size=size) (trainer.py:280), one launch."""
        return OH.preprocess(x, size)

    @torch.no_grad()
    def _features(self, x, taps=None):
        """The pooled [N, 2048] fp32 vector (the input of the three heads)."""
        self._check(x)
        plan = self._frozen_plan(x.device)
        return plan.features(plan.trunk(x.detach().contiguous(), taps))

    @torch.no_grad()
    def forward(self, x):
        feat = self._features(x)
        return self._plan[1].angles(feat, self.n_bins)

    def teacher_angles(self, frames, size=(224, 224)):
        return self.forward(self.preprocess(frames, size))
