"""Yardsticks shared by test_animate_cpu.py and test_animate_gpu.py: the numpy restatement of
evaluate.py's frame conversion, the fp64 restatements of the two fused motion kernels built from
the oracle's functions, the running-statistics perturbation of tests/golden/make_golden_animate.py,
and the test inputs of the kernel tests (computed once per case and left unchanged)."""
import numpy as np
import torch

from oracle import facevae_cpu as O

F32, BF16 = torch.float32, torch.bfloat16

SEEDS = dict(afe=301, ckd=302, hpe_ede=303, mfe=304, generator=305)       # make_golden_animate.py

# (N, Ns, K, C2, D, H, W)
SHAPES = {
    "fixture": (2, 2, 3, 3, 4, 8, 8),          # the fixture's MFE: 16 channels
    "odd_bcast": (3, 1, 15, 4, 2, 5, 7),       # 80 channels, D - 1 = 1, odd sizes, 210 voxels, broadcast source
    "tiny": (1, 1, 1, 4, 3, 4, 4),             # fewer voxels than one block
    "centres": (1, 1, 2, 3, 2, 3, 5),          # every size - 1 a power of two: identity_is_integral
}


def frames_u8_numpy(driving, generated):
    """evaluate.py:39-44 per frame: cat along the width, HWC, clip(0, 1), (255 * a).astype(uint8),
    for [N, 3, H, W] fp32 tensors -> [N, H, 2W, 3] uint8.  The multiply is numpy's fp32 one."""
    a = torch.cat((driving, generated), dim=3).cpu().numpy()
    a = np.transpose(a, [0, 2, 3, 1]).clip(0, 1)
    assert a.dtype == np.float32
    return torch.from_numpy((255 * a).astype(np.uint8))


def perturb_stats(mod, seed):
    """make_golden_animate.perturb_stats: running_mean ~ N(0, 0.2), running_var in [0.5, 1.5], in
    state-dict key order."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in mod.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=gen) * 0.2)
            elif k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=gen) + 0.5)


def identity_is_integral(size):
    """Whether the identity motion samples voxel centres with weight exactly 1 along an axis of
    `size` voxels: src_index(ident(i)) = ((g + 1) / 2) * (size - 1) with g = 2 * (i / (size - 1)) - 1 in
    fp32, and the fraction ix - floor(ix).  hipcc contracts that subtraction into
    fma(h, size - 1, -floor(fl(h * (size - 1)))), which sees the unrounded product, so the fraction is 0
    only where h * (size - 1) is an integer exactly, not merely after rounding (size = 4: h = fl(1 / 3),
    3 h = 1 + 2^-25, fraction 3e-8).  That holds when size - 1 is a power of two (2, 3, 5, 9, 17, ...)."""
    i = torch.arange(size)
    g = 2 * (i / (size - 1)) - 1
    h = (g + 1) * 0.5
    return bool(((h.double() * (size - 1)) == i.double()).all())


def rotations(gen, n):
    a = (torch.rand(n, 3, generator=gen) - 0.5) * 0.8

    def rot(t, rows):
        c, s, z, o = torch.cos(t), torch.sin(t), torch.zeros_like(t), torch.ones_like(t)
        e = {"c": c, "s": s, "-s": -s, "z": z, "o": o}
        return torch.stack([torch.stack([e[k] for k in r], -1) for r in rows], -2)
    Rx = rot(a[:, 0], (("c", "z", "s"), ("z", "o", "z"), ("-s", "z", "c")))
    Ry = rot(a[:, 1], (("o", "z", "z"), ("z", "c", "-s"), ("z", "s", "c")))
    Rz = rot(a[:, 2], (("c", "-s", "z"), ("s", "c", "z"), ("z", "z", "o")))
    return Ry @ Rx @ Rz


_INPUTS = {}


def motion_inputs(name):
    """Keypoints and rotations of a kernel-test case (fp32, CPU): every sample its own keypoints and
    non-identity rotations; one coordinate at exactly +1.0, one at -1.0 (a corner index equal to
    size - 1 with its neighbour outside), and a keypoint pair (kp_s 1.7, kp_d -1.0 on x) whose whole
    motion samples outside the volume."""
    if name not in _INPUTS:
        N, Ns, K, C2, D, H, W = SHAPES[name]
        gen = torch.Generator().manual_seed(4000 + sorted(SHAPES).index(name))
        kp_s = (torch.rand(Ns, K, 3, generator=gen) - 0.5) * 1.6
        kp_d = (torch.rand(N, K, 3, generator=gen) - 0.5) * 1.6
        kp_s[0, 0, 1] = 1.0
        kp_d[0, 0, 2] = -1.0
        kp_s[-1, -1, 0] = 1.7
        kp_d[-1, -1, 0] = -1.0
        _INPUTS[name] = dict(kp_s=kp_s, kp_d=kp_d, Rs=rotations(gen, Ns), Rd=rotations(gen, N),
                             fc=torch.randn(Ns, C2, D, H, W, generator=gen))
    return _INPUTS[name]


def volume(name, C, salt):
    N, Ns, K, C2, D, H, W = SHAPES[name]
    return torch.randn(Ns, C, D, H, W, generator=torch.Generator().manual_seed(5000 + salt))


def logits(name, salt):
    """Random mask logits [N, K+1, D, H, W]; voxel 1 of sample 0 has logit K 60 above the rest
    (softmax saturation)."""
    N, Ns, K, C2, D, H, W = SHAPES[name]
    lg = torch.randn(N, K + 1, D, H, W, generator=torch.Generator().manual_seed(6000 + salt)) * 2
    lg[0, :, 0, 0, 1] = lg[0, :, 0, 0, 1].clamp(-1, 1)
    lg[0, K, 0, 0, 1] = 61.0
    return lg


def _rep(t, n):
    return t if t.shape[0] == n else t.repeat(n, *([1] * (t.dim() - 1)))


def _sparse(vol64, m, N):
    return O.sparse_motions(_rep(vol64, N), _rep(m["kp_s"], N).double(), m["kp_d"].double(), _rep(m["Rs"], N).double(),
                            m["Rd"].double())


def mfe_input_fp64(name, dtype):
    """[N, (K+1)(C2+1), D, H, W] fp64: heatmap_representations, sparse_motions, deformed_source and
    the cat of MFE.forward (models.py:1066-1071) on fc rounded to `dtype`."""
    N, Ns, K, C2, D, H, W = SHAPES[name]
    m = motion_inputs(name)
    fc = _rep(m["fc"].to(dtype).double(), N)
    heat = O.heatmap_representations(fc, _rep(m["kp_s"], N).double(), m["kp_d"].double()).double()
    deformed = O.deformed_source(fc, _sparse(fc, m, N))
    return torch.cat([heat, deformed], dim=2).view(N, -1, D, H, W)


def motion_warp_fp64(name, fs, lg, dtype):
    """(warped, deformation, mask) fp64: motion_mask on the sparse motions, then deformed_source with
    that one motion, on fs and the logits rounded to `dtype`."""
    N = SHAPES[name][0]
    m = motion_inputs(name)
    fs64 = _rep(fs.to(dtype).double(), N)
    deform, mask = O.motion_mask(lg.to(dtype).double(), _sparse(fs64, m, N))
    warped = O.deformed_source(fs64, deform.unsqueeze(1))[:, 0]
    return warped, deform, mask


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()

