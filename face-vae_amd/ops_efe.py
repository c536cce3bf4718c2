"""torch.autograd.Functions of the expression feature extractor (EFE_conv5, models.py:724-799 of
Luh1124/face-vae) over the fv_efe_* entries of libfacevae (csrc/efe.hip).  As in ops.py, no CPU
fallback; activations in the storage dtype.

  KpCatFn   torch.cat((z, kp2gaussian_3d(kpc, z.shape[2:])), 1) (models.py:790-791, utils.py:130-136)
            of the NDHWC logits z [N, K, D, H, W] and the posed keypoints kpc [N, K, 3], written in one
            launch with the 2K channels zero-padded to 8 * 2^k: the input of the padded-channel
            ResBlock3D chain `mix`.  Gradients to z (the channel slice) and to kpc.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops as O
from . import ops3d
from ._lib import call, ptr, query, stream

F32 = torch.float32
KP_VARIANCE = 0.01          # kp2gaussian_3d's default, utils.py:130


def kpcat_forward(zb, kpc, kp_variance=KP_VARIANCE):
    """zb NDHWC [N, K, D, H, W] fp32 / bf16, kpc [N, K, 3] fp32 -> NDHWC [N, pad_pow2(2K), D, H, W]."""
    N, K, D, H, W = zb.shape
    cp = O.pad_pow2(2 * K)
    out = torch.empty((N, cp, D, H, W), dtype=zb.dtype, device=zb.device, memory_format=ops3d.CL3)
    call("fv_efe_kpcat_fwd", L.dtype_code(zb.dtype), ptr(zb), ptr(kpc), N, K, cp, D, H, W, float(kp_variance),
         ptr(out), stream())
    return out


def kpcat_backward(g, kpc, K, kp_variance=KP_VARIANCE):
    """g NDHWC [N, Cp, D, H, W] -> (dz NDHWC [N, K, D, H, W] like g, dkpc [N, K, 3] fp32)."""
    N, cp, D, H, W = g.shape
    dz = torch.empty((N, K, D, H, W), dtype=g.dtype, device=g.device, memory_format=ops3d.CL3)
    dkpc = torch.empty((N, K, 3), dtype=F32, device=g.device)
    ws = O._empty(max(query("fv_efe_kpcat_ws_bytes", N, K, cp, D, H, W), 8) // 8, torch.float64, g.device)
    call("fv_efe_kpcat_bwd", L.dtype_code(g.dtype), ptr(g), ptr(kpc), N, K, cp, D, H, W, float(kp_variance), ptr(dz),
         ptr(dkpc), ptr(ws), stream())
    return dz, dkpc


class KpCatFn(torch.autograd.Function):
    """z [N, K, D, H, W] (fp32 or bf16; NDHWC as Conv3dFn leaves it, anything else is copied), kpc
    [N, K, 3] -> [N, Cp, D, H, W] NDHWC in z's storage dtype: channels [0, K) z, [K, 2K) the Gaussians
    of kpc on the grid of make_coordinate_grid_3d, [2K, Cp) zero."""

    @staticmethod
    def forward(ctx, z, kpc, kp_variance=KP_VARIANCE):
        if z.dim() != 5 or kpc.dim() != 3 or tuple(kpc.shape) != (z.shape[0], z.shape[1], 3):
            raise ValueError("facevae_amd kpcat: logits [N, K, D, H, W] and keypoints [N, K, 3] are expected")
        dtype = z.dtype if z.dtype in (F32, torch.bfloat16) else F32
        zb = ops3d.to_ndhwc(z, dtype)
        if not kpc.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        k32 = kpc.detach().float().contiguous()
        out = kpcat_forward(zb, k32, kp_variance)
        ctx.K, ctx.var, ctx.zdtype, ctx.kdtype = z.shape[1], kp_variance, z.dtype, kpc.dtype
        ctx.save_for_backward(k32)
        return out

    @staticmethod
    def backward(ctx, g):
        k32, = ctx.saved_tensors
        dz, dkpc = kpcat_backward(ops3d.to_ndhwc(g, g.dtype if g.dtype in (F32, torch.bfloat16) else F32), k32,
                                  ctx.K, ctx.var)
        if dz.dtype != ctx.zdtype:
            dz = dz.to(ctx.zdtype)
        if dkpc.dtype != ctx.kdtype:
            dkpc = dkpc.to(ctx.kdtype)
        return dz, dkpc, None
