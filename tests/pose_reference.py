"""Yardsticks shared by test_pose_fused_cpu.py and test_animate_graph_gpu.py: fp64 CPU restatements of
utils.transform_kp (utils.py:53-59) and utils.transform_kp_with_new_pose (utils.py:62-76) with the
motion Jacobian Rs inv(R) of create_sparse_motions (utils.py:146), and of data.u8_to_float, plus the
seeded inputs of the pose-kernel cases (computed once per case and left unchanged).

The oracle (oracle/facevae_cpu.py) starts from given rotation matrices and has no pose function, so the
three axis rotations are written out here as in animate_reference.rotations; test_pose_fused_cpu.py
checks the restatement against the two reference fixtures before anything is asked of a kernel.  The
inverse is the closed form (adjugate over determinant) the kernels use; the same CPU test holds it to
torch.inverse in fp64."""
import numpy as np
import torch

F64 = torch.float64

# case -> (N, Nc, Ns, K)
CASES = {
    "a": (1, 1, 1, 1),        # smallest
    "b": (2, 2, 2, 3),        # the fixtures' shape
    "c": (3, 1, 1, 15),       # broadcast canonical keypoints and source rotation
    "d": (5, 5, 1, 15),       # 75 keypoints: the z-sum crosses a wave
    "e": (40, 1, 1, 15),      # 600 keypoints: the z-sum loops over the block
}


def _rot(t, rows):
    c, s, z, o = torch.cos(t), torch.sin(t), torch.zeros_like(t), torch.ones_like(t)
    e = {"c": c, "s": s, "-s": -s, "z": z, "o": o}
    return torch.stack([torch.stack([e[k] for k in r], -1) for r in rows], -2)


def rotation(yaw, pitch, roll):
    """Ry(pitch) @ Rx(yaw) @ Rz(roll) in the reference's naming of the axes (utils.py:5-57), fp64."""
    yaw, pitch, roll = (a.double().reshape(-1) for a in (yaw, pitch, roll))
    Rx = _rot(yaw, (("c", "z", "s"), ("z", "o", "z"), ("-s", "z", "c")))
    Ry = _rot(pitch, (("o", "z", "z"), ("z", "c", "-s"), ("z", "s", "c")))
    Rz = _rot(roll, (("c", "-s", "z"), ("s", "c", "z"), ("z", "z", "o")))
    return Ry @ Rx @ Rz


def inverse_adjugate(m):
    """[N, 3, 3] fp64 inverses as adjugate / determinant."""
    m = m.double()
    c = torch.linalg.cross(m[:, [1, 2, 0]], m[:, [2, 0, 1]], dim=2)      # row i: the cofactors of row i
    det = (m[:, 0] * c[:, 0]).sum(1)
    return c.transpose(1, 2) / det.view(-1, 1, 1)


def jacobian(Rs, R):
    """J = Rs inv(R) [N, 3, 3] fp64 (Rs [1 or N, 3, 3])."""
    return Rs.double() @ inverse_adjugate(R)


def transform_kp_fp64(kp_c, yaw, pitch, roll, t, scale, Rs=None):
    """-> (kp [N, K, 3], R [N, 3, 3], J or None) fp64; kp_c [1 or N, K, 3], scale of N elements."""
    R = rotation(yaw, pitch, roll)
    x = scale.double().reshape(-1, 1, 1) * kp_c.double()
    kp = torch.einsum("nij,nkj->nki", R, x.expand(R.shape[0], -1, -1)) + t.double().unsqueeze(1)
    return kp, R, None if Rs is None else jacobian(Rs, R)


def transform_kp_new_fp64(kp_in, yaw, pitch, roll, t, delta, new_yaw, new_pitch, new_roll, Rs=None):
    """-> (kp [N, K, 3] after the one z-shift 0.33 - mean(z), R_new [N, 3, 3], J or None) fp64."""
    R_old, R = rotation(yaw, pitch, roll), rotation(new_yaw, new_pitch, new_roll)
    rel_rot = R @ inverse_adjugate(R_old)
    kp = (torch.einsum("nij,nkj->nki", R, kp_in.double()) + t.double().unsqueeze(1)
          + torch.einsum("nij,nkj->nki", rel_rot, delta.double()))
    kp = kp.clone()
    kp[:, :, 2] += 0.33 - kp[:, :, 2].mean()
    return kp, R, None if Rs is None else jacobian(Rs, R)


def u8_to_float_exact(a):
    """x * fp32(1 / 255) rounded once to fp32: the product of an 8-bit integer and a 24-bit
    significand is exact in fp64, so rounding it to fp32 is the single fp32 multiply."""
    return (np.asarray(a).astype(np.float64) * np.float64(np.float32(1.0 / 255.0))).astype(np.float32)


_INPUTS = {}


def pose_inputs(name):
    """fp32 CPU inputs of a case: canonical keypoints in [-0.8, 0.8], angles N(0, 0.3) (the fixtures'
    draw; the first sample of a case with N > 1 gets larger ones, about 1 rad), translations N(0, 0.1),
    scales in [0.75, 1.25], expression offsets N(0, 0.05), a source rotation per Ns."""
    if name not in _INPUTS:
        N, Nc, Ns, K = CASES[name]
        gen = torch.Generator().manual_seed(7100 + sorted(CASES).index(name))
        r = lambda *s: torch.randn(*s, generator=gen)                # noqa: E731
        ins = dict(kp_c=(torch.rand(Nc, K, 3, generator=gen) - 0.5) * 1.6,
                   yaw=r(N) * 0.3, pitch=r(N) * 0.3, roll=r(N) * 0.3, t=r(N, 3) * 0.1,
                   scale=(torch.rand(N, generator=gen) * 0.5 + 0.75).view(N, 1, 1, 1),
                   delta=r(N, K, 3) * 0.05, new_yaw=r(N) * 0.3, new_pitch=r(N) * 0.3, new_roll=r(N) * 0.3)
        if N > 1:
            for k, v in (("yaw", 1.1), ("pitch", -0.9), ("roll", 1.3), ("new_yaw", -1.2)):
                ins[k][0] = v
        src = r(Ns, 3) * 0.3
        ins["Rs"] = rotation(src[:, 0], src[:, 1], src[:, 2]).float()
        _INPUTS[name] = ins
    return _INPUTS[name]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
