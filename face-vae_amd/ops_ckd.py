"""torch.autograd.Functions of the canonical keypoint detector (CKD, models.py:948-987 of
Luh1124/face-vae) over the fv_ckd_* entries of libfacevae (csrc/ckd.hip).  As in ops.py, no CPU
fallback; activations in the storage dtype, results the module returns fp32.

  ResizeFn       F.interpolate(x, mode="bilinear", scale_factor=s, align_corners=False,
                 recompute_scale_factor=True) of the NCHW fp32 image, written as the first conv's
                 input (NHWC, storage dtype, channels 3 -> 8): one launch for the interpolate, the
                 cast and the re-layout
  SoftArgmaxFn   heatmap2kp(out2heatmap(z)) (utils.py:106-118) of the NDHWC logits without the
                 heatmap: kp [N, K, 3] fp32
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from . import ops as O
from . import ops3d
from ._lib import call, ptr, query, stream

F32 = torch.float32


def resized(size: int, scale_factor: float) -> int:
    """Output size of F.interpolate(..., recompute_scale_factor=True): floor(size * scale)."""
    return int(math.floor(float(size) * scale_factor))


class ResizeFn(torch.autograd.Function):
    """x [N, 3, H, W] (any float dtype, NCHW) -> [N, 8, Ho, Wo] dense NHWC in `dtype`, channels
    3-7 zero: ops.to_nhwc passes it through, and the conv that follows runs with cin_valid = 3.
    The image is data (trainer.py:272-273): it gets no gradient."""

    @staticmethod
    def forward(ctx, x, scale_factor, dtype):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        N, C, H, W = x.shape
        if C != 3:
            raise ValueError("facevae_amd resize: a 3-channel image is expected")
        Ho, Wo = resized(H, scale_factor), resized(W, scale_factor)
        if Ho < 1 or Wo < 1:
            raise ValueError(f"facevae_amd resize: {H} x {W} at scale {scale_factor} leaves no pixel")
        x32 = x.detach().float().contiguous()
        y = torch.empty((N, 8, Ho, Wo), dtype=dtype, device=x.device, memory_format=O.CL)
        call("fv_ckd_resize_fwd", L.dtype_code(dtype), ptr(x32), N, H, W, Ho, Wo, ptr(y), stream())
        ctx.mark_non_differentiable(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return None, None, None


def softargmax_forward(zb, temperature):
    """zb NDHWC [N, K, D, H, W] fp32 / bf16 -> (kp [N, K, 3] fp32, stat [N, K, 8] fp32: the maximum, the sum
    and kp as fp32 pairs for the backward)."""
    N, K, D, H, W = zb.shape
    dev = zb.device
    kp = torch.empty((N, K, 3), dtype=F32, device=dev)
    stat = torch.empty((N, K, 8), dtype=F32, device=dev)
    ws = O._empty(max(query("fv_ckd_softargmax_ws_bytes", N, K, D, H, W), 8) // 8, torch.float64, dev)
    call("fv_ckd_softargmax_fwd", L.dtype_code(zb.dtype), ptr(zb), N, K, D, H, W, float(temperature), ptr(kp),
         ptr(stat), ptr(ws), stream())
    return kp, stat


def softargmax_backward(zb, g, stat, temperature):
    """-> dz like zb (NDHWC, the layout ops3d.conv3dg_backward takes as dy)."""
    N, K, D, H, W = zb.shape
    dz = torch.empty_like(zb)
    call("fv_ckd_softargmax_bwd", L.dtype_code(zb.dtype), ptr(zb), ptr(g), ptr(stat), N, K, D, H, W,
         float(temperature), ptr(dz), stream())
    return dz


class SoftArgmaxFn(torch.autograd.Function):
    """z [N, K, D, H, W] (fp32 or bf16; NDHWC as Conv3dFn leaves it, anything else is copied) ->
    kp [N, K, 3] fp32 = sum_v softmax_v(z / T) * grid(v), grid = (x along W, y along H, z along D) in
    [-1, 1] (make_coordinate_grid_3d, utils.py:91-103)."""

    @staticmethod
    def forward(ctx, z, temperature=0.1):
        if z.dim() != 5:
            raise ValueError("facevae_amd soft-argmax: logits [N, K, D, H, W] are expected")
        dtype = z.dtype if z.dtype in (F32, torch.bfloat16) else F32
        zb = ops3d.to_ndhwc(z, dtype)
        kp, stat = softargmax_forward(zb, temperature)
        ctx.temperature, ctx.zdtype = temperature, z.dtype
        ctx.save_for_backward(zb, stat)
        return kp

    @staticmethod
    def backward(ctx, g):
        zb, stat = ctx.saved_tensors
        dz = softargmax_backward(zb, g.float().contiguous(), stat, ctx.temperature)
        if dz.dtype != ctx.zdtype:
            dz = dz.to(ctx.zdtype)
        return dz, None
