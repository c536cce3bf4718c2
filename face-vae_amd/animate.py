"""Reenactment inference: a source face and driving frames in, the re-enacted frames out -- the job
of the reference's evaluate.py, on the data flow of GeneratorFull.forward (trainer.py:267-297),
which is the current one (evaluate.py itself is stale against the networks: HPE_EDE returns a
scale, not a per-keypoint delta, and the MFE returns three values).

Everything about the source is computed once (`set_source`); a `drive` call batches T driving
frames against it without repeating the appearance volume, builds the MFE's hourglass input and
the blended warp with the fused kernels of csrc/animate.hip (warp.mfe_input / warp.motion_warp) and
can hand back uint8 side-by-side frames (warp.frames_u8).  No gradient is taken anywhere.
"""
from __future__ import annotations

import torch

from . import ops3d, warp
from .pose import transform_kp, transform_kp_with_new_pose


class Animator:
    """Animator(afe, ckd, hpe_ede, mfe, generator, efe=None): puts every network in eval mode;
    every call runs under torch.no_grad().  The networks keep their device and compute dtype.

    set_source(s): s [1 or N, 3, H, W] fp32 in [0, 1] on the GPU.  Keeps fs = afe(s), kp_c = ckd(s),
    the source pose (yaw, pitch, roll, t, scale) = hpe_ede(s), (kp_s, Rs) = transform_kp(...) -- kp_s
    refined by efe(s, None, kp_s)[0] when an EFE is given -- and fc = mfe.compress(fs).

    drive(d, new_pose=None, as_uint8=False): d [T, 3, H, W]; T is free with a single source, else
    the source batch.  hpe_ede(d) -> transform_kp -> (efe(d, None, kp_d_old)[0]) -> mfe.infer with
    the cached fc -> the occlusion conv -> generator.infer.  Returns the generated frames
    [T, 3, H, W] fp32, or with as_uint8 the [T, H, 2W, 3] uint8 frames, driving left, generated
    right.  `aux` holds the last call's kp_d, Rd, pose, deformation and occlusion.

    new_pose=(yaw, pitch, roll) (floats or [T] tensors, radians as hpe_ede's) re-poses every frame:
    (kp_d, Rd) = transform_kp_with_new_pose(scale_d * kp_c, yaw_d, pitch_d, roll_d, t_d, delta,
    *new_pose), with delta = kp_d - kp_d_old the EFE's expression offset of that frame (zeros
    without an EFE).  transform_kp_with_new_pose shifts z by 0.33 - mean(z) over the whole call's
    keypoints, so a frame's result depends on the frames it is batched with.  new_pose=(0, 0, 0) on the
    frame given to set_source is the reference's frontalisation mode (evaluate.py:46-66); that mode
    cannot run as the reference wrote it, because it passes HPE_EDE's fifth output as a
    per-keypoint delta and HPE_EDE now returns the scale there.
    """

    def __init__(self, afe, ckd, hpe_ede, mfe, generator, efe=None):
        self.afe, self.ckd, self.hpe_ede, self.mfe, self.generator, self.efe = afe, ckd, hpe_ede, mfe, generator, efe
        for m in (afe, ckd, hpe_ede, mfe, generator, efe):
            if m is not None:
                m.eval()
        self.fs = self.fc = self.kp_c = self.kp_s = self.Rs = self.pose_s = None
        self.aux = {}

    @staticmethod
    def _gpu(x, what):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"Animator: {what} must be [N, 3, H, W], got {list(x.shape)}")

    @torch.no_grad()
    def set_source(self, s):
        self._gpu(s, "the source")
        self.fs = self.afe(s)
        self.kp_c = self.ckd(s)
        self.pose_s = self.hpe_ede(s)
        self.kp_s, self.Rs = transform_kp(self.kp_c, *self.pose_s)
        if self.efe is not None:
            self.kp_s = self.efe(s, None, self.kp_s)[0]
        self.fc = self.mfe.compress(self.fs)
        return self

    @torch.no_grad()
    def drive(self, d, new_pose=None, as_uint8=False):
        self._gpu(d, "the driving frames")
        if self.fc is None:
            raise RuntimeError("Animator.drive: call set_source first")
        T, Ns = d.shape[0], self.fs.shape[0]
        if Ns not in (1, T):
            raise ValueError(f"Animator.drive: {T} driving frames against a source batch of {Ns} (1 or {T})")
        yaw, pitch, roll, t, scale = self.hpe_ede(d)
        kp_d_old, Rd = transform_kp(self.kp_c, yaw, pitch, roll, t, scale)
        kp_d = self.efe(d, None, kp_d_old)[0] if self.efe is not None else kp_d_old
        if new_pose is not None:
            new = [torch.as_tensor(a, dtype=yaw.dtype, device=yaw.device).expand(T) for a in new_pose]
            kp_d, Rd = transform_kp_with_new_pose(scale.view(T, 1, 1) * self.kp_c, yaw, pitch, roll, t,
                                                  kp_d - kp_d_old, *new)
        J = warp.motion_jacobian(self.Rs, Rd)                      # one inverse for both fused launches
        x, mask_logits, _ = self.mfe.infer(None, self.kp_s, kp_d, self.Rs, Rd, fc=self.fc, J=J)
        occlusion = self.mfe.occlusion_conv(ops3d.depth_merge(x, self.mfe.compute_dtype()), sigmoid=True)
        generated, deformation = self.generator.infer(self.fs, mask_logits, self.kp_s, kp_d, self.Rs, Rd, occlusion,
                                                      J=J)
        self.aux = dict(kp_d=kp_d, kp_d_old=kp_d_old, Rd=Rd, pose=(yaw, pitch, roll, t, scale),
                        deformation=deformation, occlusion=occlusion)
        return warp.frames_u8(d, generated) if as_uint8 else generated
