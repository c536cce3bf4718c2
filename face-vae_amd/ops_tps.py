"""The equivariance transform's operators (Transform, trainer.py:91-129 of Luh1124/face-vae) over the
fv_tps_* entries of libfacevae (csrc/tps.hip).  As in ops.py, no CPU fallback.

  warp_frame     Transform.transform_frame (trainer.py:106-110): the grid, the affine + thin-plate-
                 spline map of it and F.grid_sample(align_corners=True, padding_mode="reflection")
                 in one launch; NCHW fp32 in and out, no gradient (the frame is data)
  WarpCoordsFn   Transform.warp_coordinates (trainer.py:112-129) of [N, M, 2] points, differentiable
                 in the points

theta [N, 2, 3] and control_params [N, 1, points_tps^2] (or [N, points_tps^2]) are device tensors the
kernels read when they run.
"""
from __future__ import annotations

import torch

from . import ops as O
from ._lib import call, ptr, stream

F32 = torch.float32


def _cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")


def _params(theta, control_params, n, points_tps):
    if tuple(theta.shape) != (n, 2, 3):
        raise ValueError(f"facevae_amd tps: theta {tuple(theta.shape)} is not [{n}, 2, 3]")
    if control_params.numel() != n * points_tps ** 2:
        raise ValueError(f"facevae_amd tps: control_params {tuple(control_params.shape)} does not hold "
                         f"{n} x {points_tps ** 2} values")
    return theta.detach().to(F32).contiguous(), control_params.detach().to(F32).contiguous()


def warp_frame(frame, theta, control_params, points_tps):
    """frame [N, C, H, W] (any float dtype) -> the warped frame, NCHW fp32."""
    _cuda(frame, theta, control_params)
    if frame.dim() != 4:
        raise ValueError("facevae_amd tps: a frame [N, C, H, W] is expected")
    N, C, H, W = frame.shape
    th, cp = _params(theta, control_params, N, points_tps)
    x = frame.detach().to(F32).contiguous()
    y = O._empty(x.numel(), F32, frame.device).view(N, C, H, W)
    call("fv_tps_warp_frame_fwd", ptr(x), ptr(th), ptr(cp), N, C, H, W, int(points_tps), ptr(y), stream())
    return y


def warp_coords_forward(coords, theta, cparams, points_tps):
    """coords [N, M, 2] fp32 contiguous -> T(coords)."""
    N, M, _ = coords.shape
    out = O._empty(coords.numel(), F32, coords.device).view(N, M, 2)
    call("fv_tps_warp_coords_fwd", ptr(coords), ptr(theta), ptr(cparams), N, M, int(points_tps), ptr(out), stream())
    return out


def warp_coords_backward(coords, g, theta, cparams, points_tps):
    N, M, _ = coords.shape
    out = O._empty(coords.numel(), F32, coords.device).view(N, M, 2)
    call("fv_tps_warp_coords_bwd", ptr(coords), ptr(g), ptr(theta), ptr(cparams), N, M, int(points_tps), ptr(out),
         stream())
    return out


class WarpCoordsFn(torch.autograd.Function):
    """coords [N, M, 2] -> theta[:, :, :2] p + theta[:, :, 2] + r(p), r the thin-plate-spline term over
    the points_tps x points_tps lattice; fp32.  theta and control_params get no gradient: they are
    the transform's random constants."""

    @staticmethod
    def forward(ctx, coords, theta, control_params, points_tps):
        _cuda(coords, theta, control_params)
        if coords.dim() != 3 or coords.shape[2] != 2:
            raise ValueError("facevae_amd tps: coordinates [N, M, 2] are expected")
        th, cp = _params(theta, control_params, coords.shape[0], points_tps)
        c32 = coords.detach().to(F32).contiguous()
        ctx.points_tps, ctx.cdtype = points_tps, coords.dtype
        ctx.save_for_backward(c32, th, cp)
        return warp_coords_forward(c32, th, cp, points_tps)

    @staticmethod
    def backward(ctx, g):
        c32, th, cp = ctx.saved_tensors
        d = warp_coords_backward(c32, g.to(F32).contiguous(), th, cp, ctx.points_tps)
        if d.dtype != ctx.cdtype:
            d = d.to(ctx.cdtype)
        return d, None, None, None
