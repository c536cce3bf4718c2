"""Head pose -> keypoints (utils.py:5-59 of Luh1124/face-vae): the three axis rotations and
`transform_kp`, which turns canonical keypoints and the HPE_EDE outputs into the posed keypoints
and the rotation matrix the MFE takes (kp_s / kp_d, Rs / Rd).  A handful of [N, 3, 3] and
[N, K, 3] tensors: plain torch ops, on whatever device the inputs live."""
from __future__ import annotations

import torch


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
