"""Reenactment inference: a source face and driving frames in, the re-enacted frames out -- the job
of the reference's evaluate.py, on the data flow of GeneratorFull.forward (trainer.py:267-297),
which is the current one (evaluate.py itself is stale against the networks: HPE_EDE returns a
scale, not a per-keypoint delta, and the MFE returns three values).

Everything about the source is computed once (`set_source`); a `drive` call batches T driving
frames against it without repeating the appearance volume, builds the MFE's hourglass input and
the blended warp with the fused kernels of csrc/animate.hip (warp.mfe_input / warp.motion_warp) and
can hand back uint8 side-by-side frames (warp.frames_u8).  No gradient is taken anywhere.

For one frame at a time (T = 1: a webcam, a stream) the eager call costs the host ~490 library
entries per frame.  `drive(fused_pose=True)` runs the pose step as one launch (pose.pose_kp /
pose_kp_new) without the solver call of torch.inverse, which leaves nothing in the call that
synchronises with the host, and `Animator.capture` records that call once into a HIP graph
(graph.StepGraph): a `CapturedDrive` replays it on static input tensors with one graph launch per
call (the frame itself stays bound by its kernels).
"""
from __future__ import annotations

import torch

from . import ops3d, pose, warp
from .graph import StepGraph
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

    drive(..., fused_pose=True): the same data flow with transform_kp + warp.motion_jacobian (and, with
    new_pose, transform_kp_with_new_pose + the second Jacobian) replaced by pose.pose_kp /
    pose.pose_kp_new: one launch each, the inverse in closed form, no host synchronisation anywhere
    in the call.  The default runs the torch composition.

    capture(T, new_pose=False, as_uint8=False, u8_in=False, warmup=1) -> CapturedDrive: the
    drive(fused_pose=True) call for T frames as one HIP graph on static inputs.  Needs set_source
    first and every network in eval mode.  After a capture, set_source writes the new source's tensors
    into the captured ones in place (the graph then drives the new source); a source of another
    shape raises ValueError: capture again on a new Animator.
    """

    def __init__(self, afe, ckd, hpe_ede, mfe, generator, efe=None):
        self.afe, self.ckd, self.hpe_ede, self.mfe, self.generator, self.efe = afe, ckd, hpe_ede, mfe, generator, efe
        for m in (afe, ckd, hpe_ede, mfe, generator, efe):
            if m is not None:
                m.eval()
        self.fs = self.fc = self.kp_c = self.kp_s = self.Rs = self.pose_s = None
        self.aux = {}
        self._hw = None
        self._captured = False         # a CapturedDrive reads the source tensors by address

    @staticmethod
    def _gpu(x, what):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"Animator: {what} must be [N, 3, H, W], got {list(x.shape)}")

    @torch.no_grad()
    def set_source(self, s):
        self._gpu(s, "the source")
        if self._captured and tuple(s.shape) != (self.fs.shape[0], 3, *self._hw):
            raise ValueError(f"Animator.set_source: a graph was captured on a source of "
                             f"{[self.fs.shape[0], 3, *self._hw]}, got {list(s.shape)}: capture again on a new "
                             "Animator")
        fs = self.afe(s)
        kp_c = self.ckd(s)
        pose_s = self.hpe_ede(s)
        kp_s, Rs = transform_kp(kp_c, *pose_s)
        if self.efe is not None:
            kp_s = self.efe(s, None, kp_s)[0]
        fc = self.mfe.compress(fs)
        new = (fs, fc, kp_c, kp_s, Rs, *pose_s)
        if self._captured:
            old = (self.fs, self.fc, self.kp_c, self.kp_s, self.Rs, *self.pose_s)
            if any(o.shape != n.shape or o.dtype != n.dtype for o, n in zip(old, new)):
                raise ValueError("Animator.set_source: the new source's tensors differ in shape or dtype from the "
                                 "captured ones: capture again on a new Animator")
            for o, n in zip(old, new):
                o.copy_(n)
        else:
            self.fs, self.fc, self.kp_c, self.kp_s, self.Rs, self.pose_s = fs, fc, kp_c, kp_s, Rs, pose_s
            self._hw = tuple(s.shape[2:])
        return self

    def _check_drive(self, d, what):
        self._gpu(d, "the driving frames")
        if self.fc is None:
            raise RuntimeError(f"Animator.{what}: call set_source first")
        T, Ns = d.shape[0], self.fs.shape[0]
        if Ns not in (1, T):
            raise ValueError(f"Animator.{what}: {T} driving frames against a source batch of {Ns} (1 or {T})")
        return T

    @torch.no_grad()
    def _drive_fused(self, d, new_pose, as_uint8):
        T = self._check_drive(d, "drive")
        yaw, pitch, roll, t, scale = self.hpe_ede(d)
        kp_d_old, Rd, J = pose.pose_kp(self.kp_c, yaw, pitch, roll, t, scale, self.Rs)
        kp_d = self.efe(d, None, kp_d_old)[0] if self.efe is not None else kp_d_old
        if new_pose is not None:
            # a float becomes a device fill, not a host-to-device copy
            new = [a.to(device=yaw.device, dtype=yaw.dtype).expand(T) if isinstance(a, torch.Tensor) else
                   torch.full((T,), float(a), dtype=yaw.dtype, device=yaw.device) for a in new_pose]
            kp_d, Rd, J = pose.pose_kp_new(scale.view(T, 1, 1) * self.kp_c, yaw, pitch, roll, t, kp_d - kp_d_old,
                                           *new, Rs=self.Rs)
        x, mask_logits, _ = self.mfe.infer(None, self.kp_s, kp_d, self.Rs, Rd, fc=self.fc, J=J)
        occlusion = self.mfe.occlusion_conv(ops3d.depth_merge(x, self.mfe.compute_dtype()), sigmoid=True)
        generated, deformation = self.generator.infer(self.fs, mask_logits, self.kp_s, kp_d, self.Rs, Rd, occlusion,
                                                      J=J)
        self.aux = dict(kp_d=kp_d, kp_d_old=kp_d_old, Rd=Rd, pose=(yaw, pitch, roll, t, scale),
                        deformation=deformation, occlusion=occlusion)
        return warp.frames_u8(d, generated) if as_uint8 else generated

    def capture(self, T, new_pose=False, as_uint8=False, u8_in=False, warmup=1):
        return CapturedDrive(self, T, new_pose, as_uint8, u8_in, warmup)

    @torch.no_grad()
    def drive(self, d, new_pose=None, as_uint8=False, fused_pose=False):
        if fused_pose:
            return self._drive_fused(d, new_pose, as_uint8)
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


class CapturedDrive:
    """One `Animator.drive(fused_pose=True)` call for T frames, captured as a HIP graph
    (Animator.capture).  The graph is a single chain on one stream; the eval-mode descriptor tables
    of the batched weight preparation go through graph.StepGraph's staging protocol.

    __call__(d, new_pose=None): copies d ([T, 3, H, W] fp32, or [T, H, W, 3] uint8 with u8_in) -- and,
    for a capture with new_pose, the three angles (floats or [T] tensors) -- into the static inputs,
    replays, and returns the static output: the generated frames [T, 3, H, W] fp32, or with as_uint8
    the [T, H, 2W, 3] uint8 side-by-side frames.  `aux` is a dict of static tensors (kp_d, kp_d_old,
    Rd, pose, deformation, occlusion).  THE OUTPUT AND EVERY aux TENSOR ARE OVERWRITTEN BY THE NEXT
    REPLAY: clone what must outlive it.  A d of another shape or dtype raises ValueError; there is
    no eager fall-back.

    stream(chunks): a generator over host uint8 [T, H, W, 3] arrays that yields the host uint8
    [T, H, 2W, 3] frames of every chunk in order (u8_in and as_uint8 captures only).  The upload
    of chunk i + 1 and the download of chunk i - 1 run on one copy stream while chunk i replays.
    """

    def __init__(self, animator, T, new_pose=False, as_uint8=False, u8_in=False, warmup=1):
        a = animator
        if a.fc is None:
            raise RuntimeError("Animator.capture: call set_source first")
        nets = (a.afe, a.ckd, a.hpe_ede, a.mfe, a.generator, a.efe)
        if any(m is not None and m.training for m in nets):
            raise RuntimeError("Animator.capture is inference-only: call .eval() on every network first")
        T, Ns = int(T), a.fs.shape[0]
        if T < 1 or Ns not in (1, T):
            raise ValueError(f"Animator.capture: {T} driving frames against a source batch of {Ns} (1 or {T})")
        dev, (H, W) = a.fs.device, a._hw
        self.animator, self.T, self.new_pose, self.as_uint8, self.u8_in = a, T, bool(new_pose), bool(as_uint8), bool(u8_in)
        self.d = (torch.zeros((T, H, W, 3), dtype=torch.uint8, device=dev) if u8_in
                  else torch.zeros((T, 3, H, W), dtype=torch.float32, device=dev))
        self.angles = tuple(torch.zeros(T, dtype=torch.float32, device=dev) for _ in range(3)) if new_pose else None

        def step():
            d = warp.frames_from_u8(self.d) if self.u8_in else self.d
            out = a.drive(d, new_pose=self.angles, as_uint8=self.as_uint8, fused_pose=True)
            return out, dict(a.aux)
        self._graph = StepGraph(step, warmup=warmup).capture()
        self.out, self.aux = self._graph.out
        a._captured = True
        self._pipe = None

    def _set_inputs(self, d, new_pose):
        if not isinstance(d, torch.Tensor) or d.shape != self.d.shape or d.dtype != self.d.dtype:
            raise ValueError(f"CapturedDrive: captured for {list(self.d.shape)} {self.d.dtype}, got "
                             f"{list(getattr(d, 'shape', ()))} {getattr(d, 'dtype', type(d))}: capture again for "
                             "another shape")
        if (new_pose is not None) != self.new_pose:
            raise ValueError("CapturedDrive: new_pose is part of the capture (Animator.capture(new_pose=...)): "
                             + ("three angles are required" if self.new_pose else "this graph takes none"))
        self.d.copy_(d, non_blocking=True)
        if self.new_pose:
            for dst, src in zip(self.angles, new_pose):
                if isinstance(src, torch.Tensor):
                    dst.copy_(src.expand(self.T), non_blocking=True)
                else:
                    dst.fill_(float(src))

    def __call__(self, d, new_pose=None):
        self._set_inputs(d, new_pose)
        self._graph.replay()
        return self.out

    def stream(self, chunks):
        if not (self.u8_in and self.as_uint8):
            raise RuntimeError("CapturedDrive.stream: needs a capture with u8_in=True and as_uint8=True")
        if self.new_pose:
            raise RuntimeError("CapturedDrive.stream: a new_pose capture takes its angles per call")
        import numpy as np
        if self._pipe is None:
            # two pinned buffers per direction for the host side, two device buffers per direction so
            # that a copy never touches the graph's own input / output while it replays
            self._pipe = dict(
                cs=torch.cuda.Stream(device=self.d.device),
                pin_in=[torch.empty(self.d.shape, dtype=torch.uint8).pin_memory() for _ in range(2)],
                pin_out=[torch.empty(self.out.shape, dtype=torch.uint8).pin_memory() for _ in range(2)],
                dev_in=[torch.empty_like(self.d) for _ in range(2)],
                dev_out=[torch.empty_like(self.out) for _ in range(2)],
                up=[torch.cuda.Event() for _ in range(2)], in_free=[torch.cuda.Event() for _ in range(2)],
                ready=[torch.cuda.Event() for _ in range(2)], down=[torch.cuda.Event() for _ in range(2)])
        p = self._pipe
        cs, cur = p["cs"], torch.cuda.current_stream()

        def upload(j, a):
            a = np.asarray(a)
            if a.shape != tuple(self.d.shape) or a.dtype != np.uint8:
                raise ValueError(f"CapturedDrive.stream: captured for uint8 {list(self.d.shape)}, got {a.dtype} "
                                 f"{list(a.shape)}")
            p["up"][j].synchronize()                    # the upload two chunks ago has left this pinned buffer
            p["pin_in"][j].copy_(torch.from_numpy(np.ascontiguousarray(a)))
            cs.wait_event(p["in_free"][j])              # ... and the replay has taken its device buffer
            with torch.cuda.stream(cs):
                p["dev_in"][j].copy_(p["pin_in"][j], non_blocking=True)
                p["up"][j].record(cs)

        def fetch(j):
            p["down"][j].synchronize()
            return p["pin_out"][j].numpy().copy()

        it = iter(chunks)
        nxt = next(it, None)
        if nxt is not None:
            upload(0, nxt)
        i, pending = 0, None
        while nxt is not None:
            j = i & 1
            cur.wait_event(p["up"][j])
            self.d.copy_(p["dev_in"][j], non_blocking=True)
            p["in_free"][j].record(cur)
            nxt = next(it, None)
            if nxt is not None:
                upload(j ^ 1, nxt)                      # runs while chunk i replays
            cur.wait_event(p["down"][j])                # the download two chunks ago has read dev_out[j]
            self._graph.replay()
            p["dev_out"][j].copy_(self.out, non_blocking=True)
            p["ready"][j].record(cur)
            cs.wait_event(p["ready"][j])
            with torch.cuda.stream(cs):
                p["pin_out"][j].copy_(p["dev_out"][j], non_blocking=True)
                p["down"][j].record(cs)
            if pending is not None:
                yield fetch(pending)                    # chunk i - 1, downloaded while chunk i was issued
            pending = j
            i += 1
        if pending is not None:
            yield fetch(pending)
