"""Head pose -> keypoints (utils.py:5-59 of Luh1124/face-vae): the three axis rotations and
`transform_kp`, which turns canonical keypoints and the HPE_EDE outputs into the posed keypoints
and the rotation matrix the MFE takes (kp_s / kp_d, Rs / Rd).  A handful of [N, 3, 3] and
[N, K, 3] tensors: plain torch ops, on whatever device the inputs live.  `pose_kp` / `pose_kp_new` are
the inference-only one-launch forms of the two transforms (GPU only), which also return the motion
Jacobian Rs inv(R)."""
from __future__ import annotations

import torch

from . import warp
from ._lib import call, ptr, stream


def _rot(theta, rows):
    theta = theta.reshape(-1, 1, 1)
    e = {"z": torch.zeros_like(theta), "o": torch.ones_like(theta), "c": torch.cos(theta), "s": torch.sin(theta)}
    e["-s"] = -e["s"]
    return torch.cat([torch.cat([e[k] for k in row], 2) for row in rows], 1)


def rotation_matrix_x(theta):
    """utils.py:5-18 (the reference's naming: [[c, 0, s], [0, 1, 0], [-s, 0, c]])."""
    return _rot(theta, (("c", "z", "s"), ("z", "o", "z"), ("-s", "z", "c")))


def rotation_matrix_y(theta):
    """utils.py:21-34: [[1, 0, 0], [0, c, -s], [0, s, c]]."""
    return _rot(theta, (("o", "z", "z"), ("z", "c", "-s"), ("z", "s", "c")))


def rotation_matrix_z(theta):
    """utils.py:37-50: [[c, -s, 0], [s, c, 0], [0, 0, 1]]."""
    return _rot(theta, (("c", "-s", "z"), ("s", "c", "z"), ("z", "z", "o")))


def transform_kp(canonical_kp, yaw, pitch, roll, t, scale):
    """utils.py:53-59: R = Ry(pitch) @ Rx(yaw) @ Rz(roll); kp = R (scale * canonical_kp) + t.
    canonical_kp [N, K, 3]; yaw / pitch / roll [N]; t [N, 3]; scale broadcastable against
    [N, K, 3, 1] (HPE_EDE returns [N, 1, 1, 1]).  -> (kp [N, K, 3], R [N, 3, 3])."""
    rot_mat = rotation_matrix_y(pitch) @ rotation_matrix_x(yaw) @ rotation_matrix_z(roll)
    kp = torch.matmul(rot_mat.unsqueeze(1), scale * canonical_kp.unsqueeze(-1)).squeeze(-1) + t.unsqueeze(1)
    return kp, rot_mat


def transform_kp_with_new_pose(canonical_kp, yaw, pitch, roll, t, delta, new_yaw, new_pitch, new_roll):
    """utils.py:62-76: the keypoints under another head pose.  R_new = Ry(new_pitch) @ Rx(new_yaw) @
    Rz(new_roll); kp = R_new canonical_kp + t + (R_new inv(R_old)) delta, with delta [N, K, 3] the
    expression offset estimated under the old pose (yaw, pitch, roll); then ONE z-shift for the
    whole batch, 0.33 - mean(kp[..., 2]) over every sample and keypoint.  canonical_kp takes no scale
    here (the caller multiplies it in).  -> (kp [N, K, 3], R_new [N, 3, 3])."""
    old_rot_mat = rotation_matrix_y(pitch) @ rotation_matrix_x(yaw) @ rotation_matrix_z(roll)
    rot_mat = rotation_matrix_y(new_pitch) @ rotation_matrix_x(new_yaw) @ rotation_matrix_z(new_roll)
    R = torch.matmul(rot_mat, torch.inverse(old_rot_mat))
    kp = (torch.matmul(rot_mat.unsqueeze(1), canonical_kp.unsqueeze(-1)).squeeze(-1) + t.unsqueeze(1)
          + torch.matmul(R.unsqueeze(1), delta.unsqueeze(-1)).squeeze(-1))
    zt = 0.33 - kp[:, :, 2].mean()
    shift = torch.zeros(3, dtype=kp.dtype, device=kp.device)
    shift[2] = zt
    return kp + shift, rot_mat


# ----------------------------------------------------------------------------------------
# inference-only fused forms (csrc/animate.hip): one launch each, no solver call, no host
# synchronisation, so they can sit inside a HIP-graph capture (animate.CapturedDrive)
# ----------------------------------------------------------------------------------------

def _fused_args(name, N, Rs, *ts):
    warp._cuda(*ts, Rs)
    warp._no_grad_inputs(name, *ts, Rs)
    if Rs is not None and (Rs.dim() != 3 or Rs.shape[0] not in (1, N) or tuple(Rs.shape[1:]) != (3, 3)):
        raise ValueError(f"{name}: Rs must be [1 or {N}, 3, 3], got {list(Rs.shape)}")
    return [warp._f32(x) for x in ts], warp._f32(Rs)


def _angles(name, N, **angles):
    for k, a in angles.items():
        if a.numel() != N:
            raise ValueError(f"{name}: {k} must hold {N} angles, got {list(a.shape)}")


def pose_kp(kp_c, yaw, pitch, roll, t, scale, Rs=None):
    """transform_kp and the motion Jacobian in one launch (fv_pose_kp_fwd).  kp_c [1 or N, K, 3];
    yaw / pitch / roll [N]; t [N, 3]; scale [N] in any shape (HPE_EDE's [N, 1, 1, 1]); Rs [1 or N, 3, 3]
    or None.  -> (kp [N, K, 3], R [N, 3, 3], J = Rs inv(R) [N, 3, 3] or None), fp32.  GPU and inference
    only."""
    N = yaw.numel()
    (c, y, p, r, tt, s), rs = _fused_args("pose_kp", N, Rs, kp_c, yaw, pitch, roll, t, scale)
    _angles("pose_kp", N, pitch=p, roll=r, scale=s)
    if c.dim() != 3 or c.shape[0] not in (1, N) or c.shape[2] != 3 or tuple(tt.shape) != (N, 3):
        raise ValueError(f"pose_kp: kp_c [1 or {N}, K, 3] and t [{N}, 3], got {list(c.shape)} and {list(tt.shape)}")
    K = c.shape[1]
    kp = torch.empty((N, K, 3), dtype=torch.float32, device=c.device)
    R = torch.empty((N, 3, 3), dtype=torch.float32, device=c.device)
    J = torch.empty_like(R) if rs is not None else None
    call("fv_pose_kp_fwd", ptr(c), ptr(y), ptr(p), ptr(r), ptr(tt), ptr(s), ptr(rs), N, c.shape[0],
         rs.shape[0] if rs is not None else 0, K, ptr(kp), ptr(R), ptr(J), stream())
    return kp, R, J


def pose_kp_new(kp_in, yaw, pitch, roll, t, delta, new_yaw, new_pitch, new_roll, Rs=None):
    """transform_kp_with_new_pose and the motion Jacobian in one launch (fv_pose_kp_new_fwd).  kp_in
    (the caller's scale * kp_c) and delta [N, K, 3]; the six angle tensors [N]; t [N, 3].  -> (kp
    [N, K, 3] after the z-shift 0.33 - mean(z) over all N K keypoints of the call, R_new [N, 3, 3],
    J = Rs inv(R_new) or None), fp32.  The mean is one block's fixed-order sum, so N K <= 65536.  GPU
    and inference only."""
    N = yaw.numel()
    (c, y, p, r, tt, d, ny, np_, nr), rs = _fused_args("pose_kp_new", N, Rs, kp_in, yaw, pitch, roll, t, delta,
                                                        new_yaw, new_pitch, new_roll)
    _angles("pose_kp_new", N, pitch=p, roll=r, new_yaw=ny, new_pitch=np_, new_roll=nr)
    if c.dim() != 3 or c.shape[0] != N or c.shape[2] != 3 or d.shape != c.shape or tuple(tt.shape) != (N, 3):
        raise ValueError(f"pose_kp_new: kp_in and delta [{N}, K, 3] and t [{N}, 3], got {list(c.shape)}, "
                         f"{list(d.shape)} and {list(tt.shape)}")
    K = c.shape[1]
    kp = torch.empty((N, K, 3), dtype=torch.float32, device=c.device)
    R = torch.empty((N, 3, 3), dtype=torch.float32, device=c.device)
    J = torch.empty_like(R) if rs is not None else None
    call("fv_pose_kp_new_fwd", ptr(c), ptr(y), ptr(p), ptr(r), ptr(tt), ptr(d), ptr(ny), ptr(np_), ptr(nr), ptr(rs),
         N, rs.shape[0] if rs is not None else 0, K, ptr(kp), ptr(R), ptr(J), stream())
    return kp, R, J
