"""Encoder (AFE 2-D trunk), decoder (Generator 2-D trunk) and the FaceVAE composition
 with the reference constructor signatures and state-dict keys
(models.py:922-945 AFE, 1085-1111 Generator of Luh1124/face-vae)."""
from __future__ import annotations

import torch
from torch import nn

from . import config as _config
from . import ops
from . import ops3d, warp
from .modules import (Conv2d, Conv3d, ConvBlock2D, DownBlock2D, DownBlock3D, MaxPool2d, ResBlock2D, ResBlock3D,
                      ResBottleneck, UpBlock2D, UpBlock3D, _Block)


def _batched_weight_prep(model, device):
    """The per-step weight work of every conv under `model` in a few launches: one batched
    power iteration for the spectral-normed convs (ops.SNBatch, 4 launches for all of them) and
    one re-layout launch for the generic weight layouts (ops.WPrepBatch).  Run by the top-level
    forward of AFE / Generator / FaceVAE (sub-module calls go through forward_2d)."""
    from .modules import _Conv
    sb = model.__dict__.get("_snb")
    if sb is None:
        sb = ops.SNBatch([c for c in model.modules() if isinstance(c, _Conv) and c.sn])
        object.__setattr__(model, "_snb", sb)
    wb = model.__dict__.get("_wpb")
    if wb is None:
        wb = ops.WPrepBatch([c for c in model.modules() if isinstance(c, _Conv)])
        object.__setattr__(model, "_wpb", wb)
    sb.run(model.training)
    wb.run(device)


class AFE(_Block):
    """Appearance-feature extractor (models.py:922-945): in_conv 7x7 CNA, DownBlock2D chain,
    1x1 mid_conv (the 2-D trunk = the FaceVAE encoder), then x.view(N, C, D, H, W) and n_res
    ResBlock3D(C) (the 3-D trunk).  forward(x) -> [N, C, D, H/4, W/4] in the compute dtype,
    NDHWC memory (torch.channels_last_3d)."""

    def __init__(self, use_weight_norm=False, down_seq=(64, 128, 256), n_res=6, C=32, D=16):
        super().__init__()
        down_seq = list(down_seq)
        self.in_conv = ConvBlock2D("CNA", 3, down_seq[0], 7, 1, 3, use_weight_norm)
        self.down = nn.Sequential(*[DownBlock2D(down_seq[i], down_seq[i + 1], use_weight_norm)
                                    for i in range(len(down_seq) - 1)])
        self.mid_conv = Conv2d(down_seq[-1], C * D, 1, 1, 0)
        self.res = nn.Sequential(*[ResBlock3D(C, use_weight_norm) for _ in range(n_res)])
        self.C, self.D = C, D

    def forward_2d(self, x):
        return self.mid_conv(self.down(self.in_conv(x)))

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        _batched_weight_prep(self, x.device)
        h = self.forward_2d(x)
        fs = ops3d.depth_split(h, self.C, self.D, self.compute_dtype())
        if len(self.res):
            wb = self.__dict__.get("_w3b")
            if wb is None:
                wb = ops3d.W3PrepBatch([c for blk in self.res for c in (blk.conv1, blk.conv2)])
                object.__setattr__(self, "_w3b", wb)
            N, C, D, H, W = fs.shape
            wb.prep(ops3d.desc3(ops.storage(self.compute_dtype()), N, D, H, W, C, C), x.device)
        return self.res(fs)


class MFE(_Block):
    """Motion field estimator (models.py:1040-1082): 1x1x1 `compress` of the appearance volume,
    the keypoint heatmaps and the K+1 sparse motions with the compressed volume sampled at each
    (warp.py), a 3-D hourglass (DownBlock3D / UpBlock3D chains), then the 7x7x7 `mask_conv` whose
    softmax blends the sparse motions into the dense deformation, and the 7x7 `occlusion_conv`
    over the depth-merged features.  forward(fs, kp_s, kp_d, Rs, Rd) -> (deformation
    [N, D, H, W, 3], occlusion [N, 1, H, W], mask [N, K+1, D, H, W, 1]), all fp32.

    Every conv runs on the HIP kernels (3-D: ops3d.CNA3DFn / Conv3dFn on conv3d_gemm.hip; the
    occlusion conv on the 2-D path with its fused sigmoid).  The two concatenations
    (models.py:1071, 1074) are torch copies of NDHWC tensors."""

    def __init__(self, use_weight_norm=False, down_seq=(80, 64, 128, 256, 512, 1024),
                 up_seq=(1024, 512, 256, 128, 64, 32), K=15, D=16, C1=32, C2=4):
        super().__init__()
        if use_weight_norm:
            raise NotImplementedError("facevae_amd MFE: use_weight_norm=False only (no spectral norm on 3-D convs)")
        down_seq, up_seq = list(down_seq), list(up_seq)
        self.compress = Conv3d(C1, C2, 1, 1, 0)
        self.down = nn.Sequential(*[DownBlock3D(down_seq[i], down_seq[i + 1], use_weight_norm)
                                    for i in range(len(down_seq) - 1)])
        self.up = nn.Sequential(*[UpBlock3D(up_seq[i], up_seq[i + 1], use_weight_norm)
                                  for i in range(len(up_seq) - 1)])
        self.mask_conv = Conv3d(down_seq[0] + up_seq[-1], K + 1, 7, 1, 3)
        self.occlusion_conv = Conv2d((down_seq[0] + up_seq[-1]) * D, 1, 7, 1, 3)
        self.C, self.D = down_seq[0] + up_seq[-1], D

    def forward(self, fs, kp_s, kp_d, Rs, Rd):
        if not fs.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        mode = self.compute_dtype()
        dtype = ops.storage(mode)
        _batched_weight_prep(self, fs.device)
        N, _, D, H, W = fs.shape
        fc = self.compress(fs)                                               # [N, C2, D, H, W]
        heat = warp.create_heatmap_representations(fc, kp_s, kp_d)           # [N, K+1, 1, D, H, W]
        sparse_motion = warp.create_sparse_motions(fc, kp_s, kp_d, Rs, Rd)   # [N, K+1, D, H, W, 3]
        deformed = warp.create_deformed_source_image(fc, sparse_motion, dtype)   # [N, K+1, C2, D, H, W]
        # cat(dim=2).view(N, -1, D, H, W) (models.py:1071): channel = k * (C2 + 1) + c, built
        # directly in NDHWC order [N, D, H, W, K+1, C2+1]
        inp = torch.cat([heat.to(dtype).permute(0, 3, 4, 5, 1, 2), deformed.permute(0, 3, 4, 5, 1, 2)], dim=5)
        inp = inp.reshape(N, D, H, W, -1).permute(0, 4, 1, 2, 3)
        out = self.up(self.down(inp))
        x = torch.cat([inp, out], dim=1).contiguous(memory_format=ops3d.CL3)   # models.py:1074
        mask_logits = self.mask_conv(x)
        deformation, mask = warp.deformation_from_mask(mask_logits, sparse_motion)
        occlusion = self.occlusion_conv(ops3d.depth_merge(x, mode), sigmoid=True)   # models.py:1080-1081
        return deformation, occlusion, mask

    def infer(self, fs, kp_s, kp_d, Rs, Rd, fc=None, J=None):
        """Inference-only forward up to the mask logits: the hourglass input comes from one fused
        launch (warp.mfe_input), so no sparse-motion, heat-map or per-motion sample tensor is written.
        -> (x [N, C, D, H, W] the hourglass features that mask_conv and the occlusion conv read,
        mask_logits [N, K+1, D, H, W], fc = compress(fs)).  Pass the returned fc back in to skip the
        compress of an unchanged source (fs may then be None).  The source side (fs / fc, kp_s, Rs) is
        a batch of 1 or of kp_d's N.  The blend of the logits is Generator.infer's (warp.motion_warp).
        J = warp.motion_jacobian(Rs, Rd) may be passed when the caller has formed it.  Eval mode only; runs under torch.no_grad() and raises on an input that requires grad."""
        if self.training:
            raise RuntimeError("facevae_amd MFE.infer is inference-only: call .eval() first (batch statistics are "
                               "not collected on this path)")
        ts = (fs, kp_s, kp_d, Rs, Rd, fc, J)
        if fs is None and fc is None:
            raise ValueError("facevae_amd MFE.infer: the appearance volume fs or its compressed form fc is required")
        if any(t is not None and not t.is_cuda for t in ts):
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        warp._no_grad_inputs("MFE.infer", *ts)
        dtype = ops.storage(self.compute_dtype())
        with torch.no_grad():
            _batched_weight_prep(self, kp_d.device)
            if fc is None:
                fc = self.compress(fs)
            inp = warp.mfe_input(fc, kp_s, kp_d, Rs, Rd, dtype, J=J)
            out = self.up(self.down(inp))
            x = torch.cat([inp, out], dim=1).contiguous(memory_format=ops3d.CL3)   # models.py:1074
            return x, self.mask_conv(x), fc


class HPE_EDE(_Block):
    """Head pose estimator (models.py:990-1037): a ResNet-50-shaped trunk -- `pre_layers` (7x7
    stride-2 stem CNA, MaxPool2d(3, 2, 1)), `res_layers` (ResBottleneck chains, the first of every
    chain but the first at stride 2) -- then the mean over the plane and five Linear heads; the
    angles are the softmax expectation over n_bins 3-degree bins.  forward(x) -> (yaw [N],
    pitch [N], roll [N], t [N, 3], scale [N, 1, 1, 1]), all fp32; x is the NCHW fp32 image on the
    GPU and gets no gradient.  Reference constructor signature, state-dict keys and init draws
    (`K` is unused there too; `idx_tensor` is not a buffer).  H and W must be even at every
    strided stage (a multiple of 32 for the default depth)."""

    def __init__(self, use_weight_norm=False, n_filters=[64, 256, 512, 1024, 2048], n_blocks=[3, 3, 5, 2], n_bins=66,
                 K=15):
        super().__init__()
        if use_weight_norm:
            raise NotImplementedError("facevae_amd HPE_EDE: use_weight_norm=False only (no spectral norm on the "
                                      "stem, stride-2 and 'CN' blocks)")
        n_filters, n_blocks = list(n_filters), list(n_blocks)
        self.pre_layers = nn.Sequential(ConvBlock2D("CNA", 3, n_filters[0], 7, 2, 3, use_weight_norm), MaxPool2d(3, 2, 1))
        res_layers = []
        for i in range(len(n_filters) - 1):
            res_layers.extend(self._make_layer(i, n_filters[i], n_filters[i + 1], n_blocks[i], use_weight_norm))
        self.res_layers = nn.Sequential(*res_layers)
        self.fc_yaw = nn.Linear(n_filters[-1], n_bins)
        self.fc_pitch = nn.Linear(n_filters[-1], n_bins)
        self.fc_roll = nn.Linear(n_filters[-1], n_bins)
        self.fc_t = nn.Linear(n_filters[-1], 3)
        self.fc_scale = nn.Linear(n_filters[-1], 1)
        self.n_bins = n_bins

    @staticmethod
    def _make_layer(i, in_channels, out_channels, n_block, use_weight_norm):
        stride = 1 if i == 0 else 2
        return [ResBottleneck(in_channels, out_channels, stride, use_weight_norm)] + [
            ResBottleneck(out_channels, out_channels, 1, use_weight_norm) for _ in range(n_block)]

    def _check_sizes(self, H, W):
        stages = [("pre_layers.0 (7x7 stride-2 stem)", 2), ("pre_layers.1 (MaxPool2d(3, 2, 1))", 2)]
        stages += [(f"res_layers.{i} (stride-2 ResBottleneck)", b.stride) for i, b in enumerate(self.res_layers)]
        h, w = H, W
        for name, stride in stages:
            if stride != 2:
                continue
            if h % 2 or w % 2:
                raise ValueError(f"facevae_amd HPE_EDE: {name} needs an even input size, got {h} x {w} "
                                 f"(image {H} x {W})")
            h, w = h // 2, w // 2

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        from . import ops_pose
        self._check_sizes(x.shape[2], x.shape[3])
        _batched_weight_prep(self, x.device)
        stem = self.pre_layers[0]
        h = ops_pose.StemFn.apply(x, stem.conv.weight, stem.conv.bias, stem.bn.weight, stem.bn.bias, stem, True)
        h = self.res_layers(h)
        fcs = (self.fc_yaw, self.fc_pitch, self.fc_roll, self.fc_t, self.fc_scale)
        wb = [p for fc in fcs for p in (fc.weight, fc.bias)]
        out = ops_pose.PoseHeadFn.apply(h, self.n_bins, ops.storage(self.compute_dtype()), *wb)
        return out[:, 0], out[:, 1], out[:, 2], out[:, 3:6], out[:, 6].view(-1, 1, 1, 1)


class CKD(_Block):
    """Canonical keypoint detector (models.py:948-987): the image resized by `scale_factor`
    (bilinear), a DownBlock2D chain, the 1x1 `mid_conv` to C * D channels, x.view(N, C, D, H, W), an
    UpBlock3D chain, the 3x3x3 `out_conv` to K logit volumes, and the softmax expectation of the
    coordinate grid at temperature 0.1 (utils.py:106-118).  forward(x) -> kp [N, K, 3] fp32 in
    [-1, 1], (x, y, z) = (along W, along H, along D); x is the NCHW fp32 image on the GPU and gets
    no gradient.  Reference constructor signature, state-dict keys and init draws.

    The resize writes the first conv's input directly (ops_ckd.ResizeFn) and the soft-argmax never
    materialises the heatmap (ops_ckd.SoftArgmaxFn, csrc/ckd.hip); everything between runs on the
    2-D conv / BN kernels, fv_depth_split and the general 3-D conv kernels of the MFE's up stack.
    The resized image must stay even through every DownBlock2D (a multiple of 32 for the default
    depth, i.e. an image that is a multiple of 128 at scale 0.25).  fp8 mode runs in bf16."""

    def __init__(self, use_weight_norm=False, down_seq=[3, 64, 128, 256, 512, 1024],
                 up_seq=[1024, 512, 256, 128, 64, 32], D=16, K=15, scale_factor=0.25):
        super().__init__()
        if use_weight_norm:
            raise NotImplementedError("facevae_amd CKD: use_weight_norm=False only (no spectral norm on 3-D convs)")
        down_seq, up_seq = list(down_seq), list(up_seq)
        if down_seq[0] != 3:
            raise NotImplementedError(f"facevae_amd CKD: down_seq[0] must be 3, the image (got {down_seq[0]})")
        for c in down_seq[1:]:
            if not (ops.is_pow2_8(c) and c <= 2048):
                raise NotImplementedError("facevae_amd CKD: the batch-norm kernels take 8 * a power of two channels, at "
                                          f"most 2048 (down_seq has {c})")
        if not ops.is_pow2_8(up_seq[0] * D):
            raise NotImplementedError("facevae_amd CKD: the depth split reads a dense NHWC tensor, so up_seq[0] * D must "
                                      f"be 8 * a power of two (got {up_seq[0]} * {D})")
        for c in up_seq:
            if c % 8 or ops.pad_pow2(c) > 2048:
                raise NotImplementedError("facevae_amd CKD: the 3-D conv kernels take input channels in multiples of 8 "
                                          f"and the batch norm at most 2048 (up_seq has {c})")
        if D < 2:
            raise NotImplementedError(f"facevae_amd CKD: D must be at least 2, the depth coordinate divides by D - 1 (got {D})")
        if not 1 <= K <= 256:
            raise NotImplementedError(f"facevae_amd CKD: the soft-argmax kernel takes 1 <= K <= 256 (got {K})")
        self.down = nn.Sequential(*[DownBlock2D(down_seq[i], down_seq[i + 1], use_weight_norm)
                                    for i in range(len(down_seq) - 1)])
        self.mid_conv = Conv2d(down_seq[-1], up_seq[0] * D, 1, 1, 0)
        self.up = nn.Sequential(*[UpBlock3D(up_seq[i], up_seq[i + 1], use_weight_norm)
                                  for i in range(len(up_seq) - 1)])
        self.out_conv = Conv3d(up_seq[-1], K, 3, 1, 1)
        self.C, self.D = up_seq[0], D
        self.scale_factor = scale_factor
        self.temperature = 0.1                      # out2heatmap's default, utils.py:106

    def _check_sizes(self, H, W):
        from . import ops_ckd
        h, w = ops_ckd.resized(H, self.scale_factor), ops_ckd.resized(W, self.scale_factor)
        if h < 1 or w < 1:
            raise ValueError(f"facevae_amd CKD: image {H} x {W} at scale {self.scale_factor} leaves no pixel")
        for i in range(len(self.down)):
            if h % 2 or w % 2:
                raise ValueError(f"facevae_amd CKD: down.{i} (DownBlock2D, AvgPool2d(2)) needs an even input size, got "
                                 f"{h} x {w} (image {H} x {W} resized by {self.scale_factor})")
            h, w = h // 2, w // 2
        if (h << len(self.up)) < 2 or (w << len(self.up)) < 2:
            raise ValueError(f"facevae_amd CKD: the heatmap of image {H} x {W} is below 2 x 2 (the coordinate grid "
                             "divides by size - 1)")

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        from . import ops_ckd
        self._check_sizes(x.shape[2], x.shape[3])
        mode = self.compute_dtype()
        if mode == ops.FP8:
            # no fp8 path through the 3-D convs: the whole module runs in bf16 for this forward
            # (the backward reads what the forward stored, not the modules' mode)
            saved = [(m, m._dtype) for m in self.modules() if hasattr(m, "_dtype")]
            self.set_compute_dtype(torch.bfloat16)
            try:
                return self._forward(x, torch.bfloat16, ops_ckd)
            finally:
                for m, d in saved:
                    m._dtype = d
        return self._forward(x, mode, ops_ckd)

    def _forward(self, x, mode, ops_ckd):
        _batched_weight_prep(self, x.device)
        h = ops_ckd.ResizeFn.apply(x, self.scale_factor, ops.storage(mode))
        h = self.mid_conv(self.down(h))
        v = ops3d.depth_split(h, self.C, self.D, mode)            # x.view(N, C, D, H, W), models.py:982
        z = self.out_conv(self.up(v))
        return ops_ckd.SoftArgmaxFn.apply(z, self.temperature)


class EFE_conv5(_Block):
    """Expression feature extractor (models.py:724-799; `EFE` in trainer.py:8): the image resized by
    `scale_factor`, `down` (SameBlock2D then a DownBlock2D chain) to the 32-channel 4 x 4 code that
    flatten_vae_nl (models.py:525-570) splits into mu | logstd and reparameterises, the 1x1
    `mid_conv` of the 16-channel sample to C * D channels, x.view(N, C, D, H, W), `up` (UpBlock3D with
    a SameBlock3D second to last), the 3x3x3 `out_conv` to K logit volumes, the Gaussians of the
    posed keypoints `kpc` appended (models.py:790-791), `mix` (ResBlock3D(2K)), `mix_out`
    (SameBlock3D(2K, K)) and the softmax expectation of the coordinate grid at temperature 0.1.

    forward(x, x_a=None, kpc=None, train_vae=None, eps=None) -> kp [N, K, 3] fp32, x_c, x_a_c,
    (x_mu, x_logstd), (x_vae, x_hat) as the reference: x_c = down(x) and x_a_c = down(x_a) when x_a is
    given (the same modules run twice: batch-norm statistics of each pass, num_batches_tracked + 2),
    else None; x_mu / x_logstd [N, 256] fp32 in NCHW flatten order when train_vae, else None;
    x_vae = down(x) and x_hat [N, 16, 4, 4] the sample.  `eps` [N, 16, 4, 4] is the noise the
    reference draws inside flatten_vae_nl (models.py:561), here an input (torch.randn on the device
    when None).  A following KLDivergenceLoss()((x_mu, x_logstd)) reuses the value the
    reparameterisation pass reduced.  With train_vae falsy the sample is mu and the logstd channels
    get a zero gradient.  x and x_a are NCHW fp32 images on the GPU and get no gradient; kpc does.

    The resize and the soft-argmax are CKD's kernels, the concatenation is fv_efe_kpcat_fwd (one
    launch that also creates the zero pad of the 2K channels to 8 * 2^k), `mix` runs at that padded
    channel count end to end on the 3x3x3 kernels of the AFE trunk and `mix_out`'s weight gets zero
    columns for the pad.  Reference constructor signature, state-dict keys and init draws;
    use_weight_norm=True and use_vae=False raise (the reference's mid_conv takes down_seq[-1] // 2
    channels, so it cannot run without the VAE either).  fp8 mode runs in bf16."""

    def __init__(self, use_weight_norm=False, down_seq=[3, 32, 64, 128, 256, 32],
                 up_seq=[256, 256, 128, 64, 32, 32], D=16, K=15, n_res=3, scale_factor=0.25, use_vae=True):
        super().__init__()
        from .modules import SameBlock2D, SameBlock3D
        if use_weight_norm:
            raise NotImplementedError("facevae_amd EFE_conv5: use_weight_norm=False only (no spectral norm on 3-D "
                                      "convs)")
        if not use_vae:
            raise NotImplementedError("facevae_amd EFE_conv5: use_vae=True only (mid_conv takes down_seq[-1] // 2 "
                                      "channels, the VAE's sample: the reference cannot run without it either)")
        down_seq, up_seq = list(down_seq), list(up_seq)
        if down_seq[0] != 3:
            raise NotImplementedError(f"facevae_amd EFE_conv5: down_seq[0] must be 3, the image (got {down_seq[0]})")
        if down_seq[-1] != 32:
            raise NotImplementedError("facevae_amd EFE_conv5: down_seq[-1] must be 32, the 16 mu and 16 logstd channels "
                                      f"flatten_vae_nl splits (got {down_seq[-1]})")
        for c in down_seq[1:]:
            if not (ops.is_pow2_8(c) and c <= 2048):
                raise NotImplementedError("facevae_amd EFE_conv5: the batch-norm kernels take 8 * a power of two "
                                          f"channels, at most 2048 (down_seq has {c})")
        if not ops.is_pow2_8(up_seq[0] * D):
            raise NotImplementedError("facevae_amd EFE_conv5: the depth split reads a dense NHWC tensor, so up_seq[0] * D "
                                      f"must be 8 * a power of two (got {up_seq[0]} * {D})")
        for c in up_seq:
            if c % 8 or ops.pad_pow2(c) > 2048:
                raise NotImplementedError("facevae_amd EFE_conv5: the 3-D conv kernels take input channels in multiples "
                                          f"of 8 and the batch norm at most 2048 (up_seq has {c})")
        if D < 2:
            raise NotImplementedError("facevae_amd EFE_conv5: D must be at least 2, the depth coordinate divides by "
                                      f"D - 1 (got {D})")
        if not 1 <= K <= 256:
            raise NotImplementedError(f"facevae_amd EFE_conv5: the soft-argmax kernel takes 1 <= K <= 256 (got {K})")
        if ops.pad_pow2(2 * K) > 64:
            raise NotImplementedError("facevae_amd EFE_conv5: mix runs ResBlock3D at the 2K channels padded to 8 * a "
                                      f"power of two, at most 64 (got K = {K})")
        self.down = nn.Sequential(*[SameBlock2D(down_seq[i], down_seq[i + 1], use_weight_norm) if i == 0 else
                                    DownBlock2D(down_seq[i], down_seq[i + 1], use_weight_norm)
                                    for i in range(len(down_seq) - 1)])
        self.mid_conv = Conv2d(down_seq[-1] // 2, up_seq[0] * D, 1, 1, 0)
        self.up = nn.Sequential(*[SameBlock3D(up_seq[i], up_seq[i + 1], use_weight_norm) if i == len(up_seq) - 2 else
                                  UpBlock3D(up_seq[i], up_seq[i + 1], use_weight_norm)
                                  for i in range(len(up_seq) - 1)])
        self.out_conv = Conv3d(up_seq[-1], K, 3, 1, 1)
        self.mix = nn.Sequential(*[ResBlock3D(2 * K, use_weight_norm) for _ in range(n_res)])
        self.mix_out = SameBlock3D(2 * K, K, use_weight_norm)
        self.C, self.D, self.K = up_seq[0], D, K
        self.scale_factor = scale_factor
        self.temperature = 0.1                      # out2heatmap's default, utils.py:106
        self.kp_variance = 0.01                     # kp2gaussian_3d's default, utils.py:130

    def _check_sizes(self, H, W):
        from . import ops_ckd
        h, w = ops_ckd.resized(H, self.scale_factor), ops_ckd.resized(W, self.scale_factor)
        if h < 1 or w < 1:
            raise ValueError(f"facevae_amd EFE_conv5: image {H} x {W} at scale {self.scale_factor} leaves no pixel")
        for i in range(1, len(self.down)):
            if h % 2 or w % 2:
                raise ValueError(f"facevae_amd EFE_conv5: down.{i} (DownBlock2D, AvgPool2d(2)) needs an even input "
                                 f"size, got {h} x {w} (image {H} x {W} resized by {self.scale_factor})")
            h, w = h // 2, w // 2
        last = len(self.down) - 1
        if (h, w) != (4, 4):
            raise ValueError(f"facevae_amd EFE_conv5: down.{last} leaves {h} x {w}, but the VAE's view(b, 16, 4, 4) "
                             f"(models.py:564) needs 4 x 4 there: the resized image must be {4 << last} x {4 << last} "
                             f"(image {H} x {W} resized by {self.scale_factor})")

    def forward(self, x, x_a=None, kpc=None, train_vae=None, eps=None):
        if not x.is_cuda or (x_a is not None and not x_a.is_cuda) or (kpc is not None and not kpc.is_cuda):
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        if kpc is None:
            raise ValueError("facevae_amd EFE_conv5: the posed keypoints kpc [N, K, 3] are required "
                             "(kp2gaussian_3d(kpc), models.py:790)")
        if tuple(kpc.shape) != (x.shape[0], self.K, 3):
            raise ValueError(f"facevae_amd EFE_conv5: kpc must be [{x.shape[0]}, {self.K}, 3], got {list(kpc.shape)}")
        self._check_sizes(x.shape[2], x.shape[3])
        if x_a is not None:
            self._check_sizes(x_a.shape[2], x_a.shape[3])
        mode = self.compute_dtype()
        if mode == ops.FP8:
            # no fp8 path through the 3-D convs: the whole module runs in bf16 for this forward
            saved = [(m, m._dtype) for m in self.modules() if hasattr(m, "_dtype")]
            self.set_compute_dtype(torch.bfloat16)
            try:
                return self._forward(x, x_a, kpc, train_vae, eps, torch.bfloat16)
            finally:
                for m, d in saved:
                    m._dtype = d
        return self._forward(x, x_a, kpc, train_vae, eps, mode)

    def _forward(self, x, x_a, kpc, train_vae, eps, mode):
        from . import ops_ckd, ops_efe
        dtype = ops.storage(mode)
        N = x.shape[0]
        _batched_weight_prep(self, x.device)
        h = self.down(ops_ckd.ResizeFn.apply(x, self.scale_factor, dtype))          # [N, 32, 4, 4]
        x_c = x_a_c = None
        if x_a is not None:
            x_c = h
            x_a_c = self.down(ops_ckd.ResizeFn.apply(x_a, self.scale_factor, dtype))
        if train_vae:
            if eps is None:
                eps = torch.randn(N, 16, 4, 4, device=x.device)
            mu, ls, z = ops.reparameterise(h, eps, mode)
            # mu.flatten(start_dim=1) of the NCHW tensor (models.py:559-560); the pair carries the KL
            # value of the reparameterisation pass like (mu, ls) itself (ops.KLFn)
            x_mu, x_ls = mu.float().reshape(N, -1), ls.float().reshape(N, -1)
            x_mu._fv_kl = (x_ls, mu._fv_kl[1], x_mu._version, x_ls._version, mu._fv_kl[4])
        else:
            x_mu = x_ls = None
            z = h[:, :16]               # z = mu; logstd * 0 (models.py:560-561): a zero gradient
        v = ops3d.depth_split(self.mid_conv(z), self.C, self.D, mode)             # x.view(N, C, D, H, W)
        logits = self.out_conv(self.up(v))
        m = ops_efe.KpCatFn.apply(logits, kpc, self.kp_variance)                  # [N, pad_pow2(2K), D, H, W]
        heat = self.mix_out(self.mix(m))
        kp = ops_ckd.SoftArgmaxFn.apply(heat, self.temperature)
        return kp, x_c, x_a_c, (x_mu, x_ls), (h, z)


class Generator(_Block):
    """Decoder (models.py:1085-1111): grid_sample of the 3-D appearance volume by the motion
    field (1103, warp.grid_sample_3d), view to [N, C*D, H, W], in_conv (SN, LeakyReLU .2),
    mid_conv, occlusion multiply (1106, warp.occlusion_multiply), 6 ResBlock2D, 2 UpBlock2D,
    out_conv 7x7 + sigmoid.  forward(fs, deformation=None, occlusion=None): None skips the warp
    / the occlusion (identity), which is the FaceVAE composition's 2-D input."""

    def __init__(self, use_weight_norm=True, n_res=6, up_seq=(256, 128, 64), D=16, C=32):
        super().__init__()
        up_seq = list(up_seq)
        self.in_conv = ConvBlock2D("CNA", C * D, up_seq[0], 3, 1, 1, use_weight_norm, nonlinearity_type="leakyrelu")
        self.mid_conv = Conv2d(up_seq[0], up_seq[0], 1, 1, 0)
        self.res = nn.Sequential(*[ResBlock2D(up_seq[0], use_weight_norm) for _ in range(n_res)])
        self.up = nn.Sequential(*[UpBlock2D(up_seq[i], up_seq[i + 1], use_weight_norm)
                                  for i in range(len(up_seq) - 1)])
        self.out_conv = Conv2d(up_seq[-1], 3, 7, 1, 3)

    def forward_2d(self, fs, occlusion=None):
        fs = self.in_conv(fs)
        fs = self.mid_conv(fs)
        if occlusion is not None:
            fs = warp.occlusion_multiply(fs, occlusion, self.compute_dtype())
        fs = self.res(fs)
        fs = self.up(fs)
        return self.out_conv(fs, sigmoid=True)       # conv + bias + sigmoid, NCHW fp32 out

    def forward(self, fs, deformation=None, occlusion=None):
        mode = self.compute_dtype()
        if fs.is_cuda:
            _batched_weight_prep(self, fs.device)
        if fs.dim() == 5:
            if deformation is not None:
                fs = warp.grid_sample_3d(fs, deformation, ops.storage(mode))
            fs = ops3d.depth_merge(fs, mode)          # .view(N, -1, H, W), models.py:1103
        elif deformation is not None:
            raise ValueError("Generator: a deformation needs the 5-D feature volume fs [N, C, D, H, W]")
        return self.forward_2d(fs, occlusion)

    def infer(self, fs, mask_logits, kp_s, kp_d, Rs, Rd, occlusion, J=None):
        """Inference-only forward from the MFE's mask logits: the softmax, the blend of the K+1
        motions and the warp of fs [1 or N, C, D, H, W] are one fused launch (warp.motion_warp; no
        sparse-motion tensor, no separate grid sample), then the depth merge and forward_2d as in
        forward.  -> (image [N, 3, H, W] fp32, deformation [N, D, H, W, 3] fp32).  J as in MFE.infer.
        Eval mode only (no
        power iteration); runs under torch.no_grad() and raises on an input that requires grad."""
        if self.training:
            raise RuntimeError("facevae_amd Generator.infer is inference-only: call .eval() first")
        ts = (fs, mask_logits, kp_s, kp_d, Rs, Rd, occlusion, J)
        if any(t is not None and not t.is_cuda for t in ts):
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        warp._no_grad_inputs("Generator.infer", *ts)
        mode = self.compute_dtype()
        with torch.no_grad():
            _batched_weight_prep(self, fs.device)
            warped, deformation, _ = warp.motion_warp(mask_logits, fs, kp_s, kp_d, Rs, Rd, ops.storage(mode), J=J)
            return self.forward_2d(ops3d.depth_merge(warped, mode), occlusion), deformation


class Discriminator(_Block):
    """Patch discriminator (models.py:1114-1139): ConvBlock2D "CNA" with instance norm and
    LeakyReLU(0.2), stride 2 for all but the last of them, then a "CN" 3x3 conv to one channel.
    forward(x, kp) -> (output [N, 1, h, w] NCHW fp32, features = the outputs of the instance-norm
    blocks).  The input is the image with K keypoint heatmaps (kp detached, kp[..., :2] used)
    appended; kp may be None when K == 0.  Each top-level forward runs one power iteration per
    spectral-normed conv in training mode, as torch's spectral_norm does."""

    def __init__(self, use_weight_norm=True, down_seq=(64, 128, 256, 512), K=15):
        super().__init__()
        down_seq = list(down_seq)
        if 3 + K > 32:
            raise NotImplementedError("facevae_amd Discriminator: 3 + K <= 32")
        layers = [ConvBlock2D("CNA", 3 + K, down_seq[0], 3, 2, 1, use_weight_norm, "instance", "leakyrelu")]
        layers.extend(ConvBlock2D("CNA", down_seq[i], down_seq[i + 1], 3, 2 if i < len(down_seq) - 2 else 1, 1,
                                  use_weight_norm, "instance", "leakyrelu") for i in range(len(down_seq) - 1))
        layers.append(ConvBlock2D("CN", down_seq[-1], 1, 3, 1, 1, use_weight_norm, activation_type="none"))
        self.layers = nn.ModuleList(layers)
        self.K = K
        for blk in self.layers:
            # real and fake forwards meet in one backward pass: their spectral-norm terms are
            # applied per forward, not batched at the end of backward (ops._sn_defer_ok)
            blk.conv._fv_sn_nodefer = True

    def forward(self, x, kp=None):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        if self.K > 0 and kp is None:
            raise ValueError("Discriminator: keypoints are required when K > 0")
        if kp is not None and kp.shape[1] != self.K:
            raise ValueError(f"Discriminator: expected {self.K} keypoints, got {kp.shape[1]}")
        _batched_weight_prep(self, x.device)
        h = ops.DiscInputFn.apply(x, kp, self.K, ops.storage(self.compute_dtype()))
        res = []
        for layer in self.layers:
            h = layer(h)
            res.append(h)
        return res[-1], res[:-1]


class FaceVAE(_Block):
    """AFE 2-D trunk -> [mu | logstd] split + reparameterisation -> Generator 2-D trunk.

    forward(x, eps) -> (y, mu, logstd).  x: [B,3,H,H] fp32 in [0,1]; eps: [B,L,H/4,H/4]
    standard-normal noise (the reference draws it with torch.randn inside
    flatten_vae_nl, models.py:561; here it is an input so runs are reproducible)."""

    def __init__(self, cfg: _config.FaceVAEConfig = None):
        super().__init__()
        cfg = cfg or _config.FaceVAEConfig()
        self.cfg = cfg
        self.afe = AFE(False, list(cfg.down_seq), 0, C=2 * cfg.latent, D=1)
        self.generator = Generator(True, cfg.n_res, list(cfg.up_seq), D=1, C=cfg.latent)

    def forward(self, x, eps):
        if x.is_cuda:
            # all 15 power iterations in 4 launches, the generic weight layouts in one
            _batched_weight_prep(self, x.device)
        h = self.afe.forward_2d(x)
        mu, logstd, z = ops.reparameterise(h, eps, self.compute_dtype())
        y = self.generator.forward_2d(z)
        return y, mu, logstd
