"""The frozen Hopenet teacher's inference path (trainer.py:16-88 of Luh1124/face-vae, called on
3 B images per generator step at trainer.py:278-280) over fv_hopenet_prep_fwd / fv_pw_infer_*
(csrc/hopenet.hip) and the stem, pool, 3x3 conv and pose-head entries the head pose estimator
already uses.  Inference only: nothing here is an autograd Function, nothing is saved.  As
everywhere, no CPU fallback, activations NHWC in the storage dtype, parameters fp32.

The batch norms are constants, so each one is folded: scale = gamma / sqrt(running_var + eps) goes
into the conv's weights, shift = beta - running_mean * scale is the conv's bias.  Per bottleneck

    conv1  1x1            pointwise GEMM, scale1 / shift1, ReLU at the store
    conv2  3x3 (stride)   fv_conv2d_fwd / fv_conv2d_s2_fwd on w * scale2 with shift2 as the bias
    conv3  1x1            pointwise GEMM reading max(., 0), scale3 / shift3, + residual, ReLU
    projection 1x1        pointwise GEMM at the block's stride, scale_d / shift_d

that is three or four launches, with no BN-apply, subsample or join pass.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from . import ops as O
from ._lib import call, ptr, query, stream

CL = torch.channels_last
F32 = torch.float32
IMAGENET_MEAN = (0.485, 0.456, 0.406)        # utils.py:183-184
IMAGENET_STD = (0.229, 0.224, 0.225)


def _gpu(x, what):
    if not x.is_cuda:
        raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
    if x.dtype != F32 or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"facevae_amd {what}: an NCHW fp32 image batch [N, 3, H, W] is expected (got {x.dtype}, "
                         f"{list(x.shape)})")


def preprocess(x, size=(224, 224), mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """F.interpolate(apply_imagenet_normalization(x), size=size) (nearest) in one launch, bit-equal
    to torch on the CPU.  x NCHW fp32 [N, 3, H, W] on the GPU -> NCHW fp32 [N, 3, *size]."""
    _gpu(x, "Hopenet.preprocess")
    x = x.detach().contiguous()
    N, _, H, W = x.shape
    ho, wo = int(size[0]), int(size[1])
    y = torch.empty((N, 3, max(ho, 0), max(wo, 0)), dtype=F32, device=x.device)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    call("fv_hopenet_prep_fwd", ptr(x), N, H, W, ho, wo, m3, s3, ptr(y), stream())
    return y


def pw_desc(dtype, n, h, w, stride, cin, cout, in_relu=False, out_relu=False):
    return L.PwDesc(L.dtype_code(dtype), n, h, w, stride, cin, cout, int(in_relu), int(out_relu))


def pw_weight_prep(dtype, w, scale):
    """w [cout, cin(, 1, 1)] fp32, scale [cout] fp32 or None -> the weight image of `dtype`."""
    cout, cin = w.shape[0], w.shape[1]
    d = pw_desc(dtype, 1, 2, 2, 1, cin, cout)
    n = query("fv_pw_infer_wk_elems", ctypes.byref(d))
    if n == 0:
        raise L.FaceVAELibError("fv_pw_infer_wk_elems: " + L.load().fv_last_error().decode(errors="replace"))
    wk = O._empty(n, dtype, w.device)
    call("fv_pw_infer_weight_prep", ctypes.byref(d), ptr(w), ptr(scale), ptr(wk), stream())
    return wk


def pw_forward(x, wk, cout, stride=1, shift=None, res=None, in_relu=False, out_relu=False):
    """x NHWC [N, cin, H, W] of the storage dtype -> NHWC [N, cout, H / stride, W / stride]."""
    N, cin, H, W = x.shape
    d = pw_desc(x.dtype, N, H, W, stride, cin, cout, in_relu, out_relu)
    y = torch.empty((N, cout, H // stride, W // stride), dtype=x.dtype, device=x.device, memory_format=CL)
    call("fv_pw_infer_fwd", ctypes.byref(d), ptr(x), ptr(wk), ptr(shift), ptr(res), ptr(y), stream())
    return y


def fold_bn(bn):
    """(scale, shift) fp32 of an eval-mode batch norm, computed in fp64."""
    var = bn.running_var.double()
    scale = bn.weight.detach().double() / torch.sqrt(var + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.double() * scale
    return scale.float().contiguous(), shift.float().contiguous()


class _FrozenBlock:
    """Folded images of one bottleneck: the pointwise weight images and every shift.  The 3x3 conv's
    image depends on the launch geometry (the halo kernels read their own layout), so it is
    prepared per descriptor from the folded fp32 weights and kept."""

    def __init__(self, blk, dtype):
        self.dtype = dtype
        self.stride = blk.stride
        self.mid, self.cout = blk.conv1.out_channels, blk.conv3.out_channels
        s1, self.h1 = fold_bn(blk.bn1)
        s2, self.h2 = fold_bn(blk.bn2)
        s3, self.h3 = fold_bn(blk.bn3)
        self.wk1 = pw_weight_prep(dtype, blk.conv1.weight.detach(), s1)
        self.wk3 = pw_weight_prep(dtype, blk.conv3.weight.detach(), s3)
        self.w2 = (blk.conv2.weight.detach() * s2.view(-1, 1, 1, 1)).contiguous()       # fp32 fold
        self.wk2 = {}
        self.wkd = self.hd = None
        if blk.downsample is not None:
            sd, self.hd = fold_bn(blk.downsample[1])
            self.wkd = pw_weight_prep(dtype, blk.downsample[0].weight.detach(), sd)

    def conv2(self, x):
        N, mid, H, W = x.shape
        s = self.stride
        Ho, Wo = H // s, W // s
        d = O.desc(self.dtype, N, Ho, Wo, mid, mid, mid, mid, 3)
        key = bytes(d)
        wk = self.wk2.get(key)
        names = ("fv_conv2d_s2_wk_elems", "fv_conv2d_s2_weight_prep") if s == 2 else ("fv_conv_wk_elems", "fv_conv_weight_prep")
        if wk is None:
            wk = O._empty(query(names[0], ctypes.byref(d)), self.dtype, x.device)
            call(names[1], ctypes.byref(d), ptr(self.w2), None, ptr(wk), None, stream())
            self.wk2 = {key: wk}                    # the latest geometry only
        y = torch.empty((N, mid, Ho, Wo), dtype=self.dtype, device=x.device, memory_format=CL)
        if s == 2:
            call("fv_conv2d_s2_fwd", ctypes.byref(d), H, W, ptr(x), ptr(wk), ptr(self.h2), ptr(y), stream())
        else:
            call("fv_conv2d_fwd", ctypes.byref(d), ptr(x), ptr(wk), ptr(self.h2), None, None, None, ptr(y), None, stream())
        return y

    def forward(self, x):
        z = pw_forward(x, self.wk1, self.mid, 1, self.h1, None, False, True)
        z = self.conv2(z)
        res = x if self.wkd is None else pw_forward(x, self.wkd, self.cout, self.stride, self.hd)
        return pw_forward(z, self.wk3, self.cout, 1, self.h3, res, True, True)


class FrozenPlan:
    """Everything Hopenet.forward launches with, built once per (parameters, storage dtype)."""

    def __init__(self, net, dtype, device):
        self.dtype = dtype
        dc = L.dtype_code(dtype)
        w = net.conv1.weight.detach()
        cout = w.shape[0]
        self.stem_cout = cout
        self.stem_wk = O._empty(query("fv_stem7s2_wk_elems", cout), dtype, device)
        call("fv_stem7s2_weight_prep", dc, ptr(w.contiguous()), cout, ptr(self.stem_wk), stream())
        self.stem_bias = torch.zeros(cout, dtype=F32, device=device)
        self.s1, self.h1 = fold_bn(net.bn1)
        self.blocks = []
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for b in layer:
                self.blocks.append(_FrozenBlock(b, dtype))
                self.blocks[-1].last = False
            self.blocks[-1].last = True             # the layer's output: a tap of trunk()
        c = net.fc_yaw.in_features
        self.zt_w, self.zt_b = torch.zeros((3, c), dtype=F32, device=device), torch.zeros(3, dtype=F32, device=device)
        heads = (net.fc_yaw, net.fc_pitch, net.fc_roll)
        self.head_w = [h.weight.detach().contiguous() for h in heads] + [self.zt_w, self.zt_w[:1]]
        self.head_b = [h.bias.detach().contiguous() for h in heads] + [self.zt_b, self.zt_b[:1]]

    def trunk(self, x, taps=None):
        """x NCHW fp32 [N, 3, H, W] -> NHWC [N, 2048, H / 32, W / 32].  taps: a list that receives the
        maps after the pool and after each layer (the tests' localisation samples)."""
        N, _, H, W = x.shape
        dc = L.dtype_code(self.dtype)
        y = torch.empty((N, self.stem_cout, H // 2, W // 2), dtype=self.dtype, device=x.device, memory_format=CL)
        call("fv_stem7s2_fwd", dc, ptr(x), N, H, W, self.stem_cout, ptr(self.stem_wk), ptr(self.stem_bias), ptr(y), None,
             stream())
        h = torch.empty((N, self.stem_cout, H // 4, W // 4), dtype=self.dtype, device=x.device, memory_format=CL)
        am = O._empty(h.numel(), torch.uint8, x.device)
        call("fv_maxpool3s2_fwd", dc, ptr(y), N, H // 2, W // 2, self.stem_cout, ptr(self.s1), ptr(self.h1), 0.0, ptr(h),
             ptr(am), stream())
        if taps is not None:
            taps.append(h)
        for b in self.blocks:
            h = b.forward(h)
            if taps is not None and b.last:
                taps.append(h)
        return h

    def features(self, h):
        N, C, H, W = h.shape
        feat = torch.empty((N, C), dtype=F32, device=h.device)
        call("fv_pose_pool_fwd", L.dtype_code(self.dtype), ptr(h), N, H * W, C, ptr(feat), stream())
        return feat

    def angles(self, feat, n_bins):
        N, C = feat.shape
        out = torch.empty((N, 7), dtype=F32, device=feat.device)
        prob = torch.empty((N, 3, n_bins), dtype=F32, device=feat.device)
        w5 = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in self.head_w])
        b5 = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in self.head_b])
        call("fv_pose_head_fwd", ptr(feat), N, C, n_bins, w5, b5, ptr(out), ptr(prob), stream())
        ang = out[:, :3].t().contiguous()
        return ang[0], ang[1], ang[2]
