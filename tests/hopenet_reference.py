"""The frozen Hopenet teacher (trainer.py:16-88 of Luh1124/face-vae) and its preprocessing
(trainer.py:280, utils.py:182-186) restated in torch CPU ops, plus the recipe the fixture
tests/golden/hopenet.pt is regenerated from.  Imports nothing of the reference and nothing of the
product: tests/golden/make_golden_hopenet.py checks it against the reference itself, and
tests/test_hopenet_cpu.py checks it against the fixture.

The fixture stores no weights (34 MB even for layers [1, 1, 1, 1]): it stores the construction seed,
and `overwrite` below re-draws the batch-norm statistics and scales the angle heads, because with
default statistics (0, 1) the fold is nearly trivial and with nn.Linear's default init the softmaxes
are within 0.03 of uniform, so the angles would hardly depend on the trunk.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
SEED = 1601                # construction
STAT_SEED = 1602           # the overwrite recipe
INPUT_SEED = 1603
# name: (layers, num_bins, gain of the angle heads' weights).  With 6 bins the angles span 15 degrees only:
# at gain 10 two of the images' angles are closer than the fixture's 1e-2 rad, at 20 a softmax exceeds 0.9
NETS = {"l1111": ((1, 1, 1, 1), 66, 10.0), "l3463": ((3, 4, 6, 3), 66, 10.0), "bins6": ((1, 1, 1, 1), 6, 15.0)}
RESIZES = [((256, 256), (224, 224)), ((40, 56), (224, 224)), ((17, 23), (9, 31)), ((23, 17), (31, 9)), ((3, 3), (7, 7)),
           ((5, 5), (2, 2)), ((224, 224), (224, 224)), ((250, 250), (224, 224)), ((300, 300), (224, 224))]


class Bottleneck(nn.Module):
    """torchvision.models.resnet.Bottleneck's layout and forward (stride on the 3x3 conv)."""
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

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class RefHopenet(nn.Module):
    """The reference class restated (same constructor draws, same state-dict keys, same forward)."""

    def __init__(self, block=Bottleneck, layers=(3, 4, 6, 3), num_bins=66):
        self.inplanes = 64
        super().__init__()
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
        self.fc_finetune = nn.Linear(512 * block.expansion + 3, 3)
        self.idx_tensor = torch.arange(num_bins, dtype=torch.float32).unsqueeze(0)
        self.n_bins = num_bins
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

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

    def forward(self, x):
        return angles_of(self, features_of(self, x)[0])


def features_of(net, x):
    """-> (pooled [N, 2048], [the maps after the pool and after each layerL]); works on the reference
    class and on RefHopenet alike (submodules only)."""
    taps = []
    with torch.no_grad():
        x = net.maxpool(net.relu(net.bn1(net.conv1(x))))
        taps.append(x)
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            x = layer(x)
            taps.append(x)
        x = net.avgpool(x)
        return x.view(x.size(0), -1), taps


def angles_of(net, feat):
    """trainer.py:75-88 on the pooled features -> [3, N] (yaw, pitch, roll)."""
    out = []
    with torch.no_grad():
        idx = torch.arange(net.n_bins, dtype=torch.float32).unsqueeze(0)
        for fc in (net.fc_yaw, net.fc_pitch, net.fc_roll):
            p = torch.softmax(fc(feat), dim=1)
            out.append(((p * idx).sum(dim=1) - net.n_bins // 2) * 3 * math.pi / 180)
    return torch.stack(out)


def max_probs(net, feat):
    with torch.no_grad():
        return torch.stack([torch.softmax(fc(feat), dim=1).max(dim=1).values
                            for fc in (net.fc_yaw, net.fc_pitch, net.fc_roll)])


def overwrite(net, seed=STAT_SEED, head_gain=10.0):
    """The fixture's recipe: every batch norm's running_mean ~ 0.2 N(0, 1), running_var ~ U(0.5, 2),
    weight ~ U(0.5, 1.5) (U(0.1, 0.3) for every bn3, which keeps the residual sums bounded), bias ~
    0.1 N(0, 1), drawn in named_modules() order from one generator; then the three angle heads'
    weights times head_gain (10)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in net.named_modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(0.2 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
                lo, hi = (0.1, 0.3) if name.endswith("bn3") else (0.5, 1.5)
                m.weight.copy_(lo + (hi - lo) * torch.rand(c, generator=g))
                m.bias.copy_(0.1 * torch.randn(c, generator=g))
        for fc in (net.fc_yaw, net.fc_pitch, net.fc_roll):
            fc.weight.mul_(head_gain)
    return net


def build(cls, layers, num_bins, head_gain=10.0, seed=SEED, stat_seed=STAT_SEED, block=Bottleneck):
    """cls(block, layers, num_bins) after torch.manual_seed(seed), with the recipe applied, in eval
    mode.  cls is the reference class, RefHopenet or the product's Hopenet (same keys)."""
    torch.manual_seed(seed)
    net = cls(block, list(layers), num_bins)
    return overwrite(net, stat_seed, head_gain).eval()


def make_inputs(seed=INPUT_SEED):
    """Three 40 x 56 frames in [0, 1]: uniform noise, a smooth ramp, an 8-pixel checkerboard."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(3, 40, 56, generator=g)
    i = torch.arange(40, dtype=torch.float32).view(1, 40, 1) / 39
    j = torch.arange(56, dtype=torch.float32).view(1, 1, 56) / 55
    ramp = torch.cat([i * j, 0.5 * (i + j), (1 - i).expand(1, 40, 56)], 0)
    cb = (((torch.arange(40).view(40, 1) // 8) + (torch.arange(56).view(1, 56) // 8)) % 2).float()
    check = torch.stack([cb, 1 - cb, 0.25 + 0.5 * cb])
    return torch.stack([noise, ramp, check]).contiguous()


def nearest_index(n_in, n_out):
    """ATen's legacy nearest source index: min((int)floorf(dst * scale), in - 1), scale in fp32."""
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    dst = torch.arange(n_out, dtype=torch.float32)
    return torch.clamp(torch.floor(dst * scale).long(), max=n_in - 1)


def preprocess(x, size=(224, 224)):
    """(x - mean) / std at the nearest source pixel, fp32."""
    mean = x.new_tensor(MEAN).view(1, 3, 1, 1)
    std = x.new_tensor(STD).view(1, 3, 1, 1)
    src = x[:, :, nearest_index(x.shape[2], size[0])][:, :, :, nearest_index(x.shape[3], size[1])]
    return ((src - mean) / std).contiguous()


def preprocess_torch(x, size=(224, 224)):
    """What the reference computes: F.interpolate(apply_imagenet_normalization(x), size=size)."""
    mean = x.new_tensor(MEAN).view(1, 3, 1, 1)
    std = x.new_tensor(STD).view(1, 3, 1, 1)
    return F.interpolate((x - mean) / std, size=size)


def checksum(t):
    """Two exact, order-free int64 sums over the tensor's bits."""
    t = t.detach().contiguous()
    v = (t.view(torch.int32) if t.dtype == torch.float32 else t.to(torch.int32)).flatten().to(torch.int64)
    k = torch.arange(v.numel(), dtype=torch.int64) % 127 + 1
    return torch.stack([v.sum(), (v * k).sum()])


def state_checksums(net):
    return torch.stack([checksum(v) for v in net.state_dict().values()])


def sample(t, count=2000):
    """Strided samples of a map in NCHW order (an odd stride, so every channel and position class is hit)."""
    f = t.detach().float().contiguous().flatten()
    return f[::max(1, f.numel() // count) | 1].clone()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


# ------------------------------------------------------------------ bf16 emulation of the frozen path
def _bf(t):
    return t.bfloat16().float()


def _fold(bn):
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.double() - bn.running_mean.double() * scale
    return scale.float(), shift.float()


def _conv_bf16(x, conv, bn, res=None, relu_out=True):
    """One folded conv with bf16 operands and a bf16 stored output: the weights w * scale are formed
    in fp32 and rounded once; accumulator, shift and residual are added in fp32."""
    scale, shift = _fold(bn)
    w = _bf(conv.weight * scale.view(-1, 1, 1, 1))
    y = F.conv2d(_bf(x), w, None, conv.stride, conv.padding) + shift.view(1, -1, 1, 1)
    if res is not None:
        y = y + res
    return _bf(torch.relu(y) if relu_out else y)


def emulate_bf16(net, x):
    """The teacher with every conv's folded weights, input and stored output rounded to bf16 (the
    stem's batch norm is applied to the stored bf16 conv output in fp32 and the result stored in bf16,
    as a pool prologue does) -> (pooled features fp32, angles [3, N])."""
    with torch.no_grad():
        y = _bf(F.conv2d(_bf(x), _bf(net.conv1.weight), None, 2, 3))
        s, h = _fold(net.bn1)
        y = _bf(torch.relu(y * s.view(1, -1, 1, 1) + h.view(1, -1, 1, 1)))
        y = F.max_pool2d(y, 3, 2, 1)
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for b in layer:
                z = _conv_bf16(y, b.conv1, b.bn1)
                z = _conv_bf16(z, b.conv2, b.bn2, relu_out=False)        # stored before the ReLU conv3 reads through
                idn = y if b.downsample is None else _conv_bf16(y, b.downsample[0], b.downsample[1], relu_out=False)
                y = _conv_bf16(torch.relu(z), b.conv3, b.bn3, res=idn)
        feat = y.mean(dim=(2, 3))
        return feat, angles_of(net, feat)
