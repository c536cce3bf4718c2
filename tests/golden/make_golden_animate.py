"""Generate the golden fixture of the reenactment inference path FROM THE REFERENCE ITSELF.

Run in the build container only (it needs the reference checkout, absent on the GPU box):

    python tests/golden/make_golden_animate.py

Imports the reference `models.py` / `utils.py` read-only (see make_golden.py); torch.Tensor.cuda is
the identity for the duration of the script, as in make_golden_mfe.py (CPU fp32 arithmetic).  Writes
tests/golden/animate.pt (plain tensors, loaded with weights_only=True):

  new_pose  utils.transform_kp_with_new_pose (utils.py:62-76) for N = 2, K = 3: seeded canonical
            keypoints, old pose, translation, delta [2, 3, 3] and a non-zero new pose; the inputs and
            both outputs (kp, rot).
  e2e       one eval-mode pass of the reference's own networks at the toy sizes of the other
            fixtures -- AFE(False, [16, 32], n_res=1, C=8, D=4), CKD(False, down_seq=[3, 8, 16, 32],
            up_seq=[32, 16, 8], D=4, K=3), HPE_EDE(False, n_filters=[16, 32, 64], n_blocks=[1, 1],
            n_bins=6, K=3), MFE(False, down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3),
            Generator(True, 1, [32, 16], D=4, C=8) -- on one 64 x 64 source frame and two driving
            frames, without an EFE, in GeneratorFull.forward's data flow (trainer.py:267-297; the
            source side repeated for the two frames, as the reference's MFE needs).  Each network is
            built after torch.manual_seed(SEEDS[name]) and its BatchNorm running statistics are then
            re-drawn by perturb_stats(net, SEEDS[name] + 10), so that eval mode differs from identity
            statistics.  No weights are stored: the product modules draw the same RNG sequence, the
            test repeats seed + perturb_stats and checks `init_sum`.  Stored: s, d, kp_c, kp_s, kp_d,
            Rs, Rd, deformation, occlusion, mask, generated.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, save_golden  # noqa: E402

SEEDS = dict(afe=301, ckd=302, hpe_ede=303, mfe=304, generator=305)
CONFIGS = dict(
    afe=((False, [16, 32]), dict(n_res=1, C=8, D=4)),
    ckd=((False,), dict(down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3)),
    hpe_ede=((False,), dict(n_filters=[16, 32, 64], n_blocks=[1, 1], n_bins=6, K=3)),
    mfe=((False,), dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)),
    generator=((True, 1, [32, 16]), dict(D=4, C=8)),
)
CLASSES = dict(afe="AFE", ckd="CKD", hpe_ede="HPE_EDE", mfe="MFE", generator="Generator")


def perturb_stats(mod, seed):
    """Re-draw every BatchNorm's running_mean from N(0, 0.2) and running_var in [0.5, 1.5], in
    state-dict key order (the reference and the product modules share their key lists)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in mod.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=gen) * 0.2)
            elif k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=gen) + 0.5)


def init_sums(mod):
    return {k: v.detach().double().sum() for k, v in mod.state_dict().items() if v.is_floating_point()}


def build(namespace, name):
    """A seeded network with perturbed statistics, in eval mode, and its initial checksums."""
    torch.manual_seed(SEEDS[name])
    args, kw = CONFIGS[name]
    net = getattr(namespace, CLASSES[name])(*args, **kw)
    isum = init_sums(net)
    perturb_stats(net, SEEDS[name] + 10)
    return net.eval(), isum


def new_pose_case(utils):
    gen = torch.Generator().manual_seed(311)
    N, K = 2, 3
    ins = dict(kp_c=(torch.rand(N, K, 3, generator=gen) - 0.5) * 1.6,
               yaw=torch.randn(N, generator=gen) * 0.3, pitch=torch.randn(N, generator=gen) * 0.3,
               roll=torch.randn(N, generator=gen) * 0.3, t=torch.randn(N, 3, generator=gen) * 0.1,
               delta=torch.randn(N, K, 3, generator=gen) * 0.05,
               new_yaw=torch.randn(N, generator=gen) * 0.3, new_pitch=torch.randn(N, generator=gen) * 0.3,
               new_roll=torch.randn(N, generator=gen) * 0.3)
    kp, rot = utils.transform_kp_with_new_pose(ins["kp_c"], ins["yaw"], ins["pitch"], ins["roll"], ins["t"], ins["delta"],
                                               ins["new_yaw"], ins["new_pitch"], ins["new_roll"])
    return dict(ins, kp=kp, rot=rot)


@torch.no_grad()
def e2e_case(models, utils):
    nets, isum = {}, {}
    for name in SEEDS:
        nets[name], isum[name] = build(models, name)
    gen = torch.Generator().manual_seed(312)
    s = torch.rand(1, 3, 64, 64, generator=gen)
    d = torch.rand(2, 3, 64, 64, generator=gen)
    T = d.shape[0]
    fs = nets["afe"](s)
    kp_c = nets["ckd"](s)
    kp_s, Rs = utils.transform_kp(kp_c, *nets["hpe_ede"](s))
    kp_d, Rd = utils.transform_kp(kp_c, *nets["hpe_ede"](d))
    rep = lambda t: t.repeat(T, *([1] * (t.dim() - 1)))      # noqa: E731
    deformation, occlusion, mask = nets["mfe"](rep(fs), rep(kp_s), kp_d, rep(Rs), Rd)
    generated = nets["generator"](rep(fs), deformation, occlusion)
    return dict(s=s, d=d, kp_c=kp_c, kp_s=kp_s, kp_d=kp_d, Rs=Rs, Rd=Rd, deformation=deformation, occlusion=occlusion,
                mask=mask, generated=generated, init_sum=isum)


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # reference grids call .cuda()
    _, models, _ = import_reference()
    import utils  # noqa: E402  (reference)
    torch.set_num_threads(8)
    out = dict(new_pose=new_pose_case(utils), e2e=e2e_case(models, utils))
    e = out["e2e"]
    print("kp_s", e["kp_s"].flatten().tolist())
    print("kp_d", e["kp_d"].flatten().tolist())
    print("generated mean/std", e["generated"].mean().item(), e["generated"].std().item(),
          "occlusion mean/std", e["occlusion"].mean().item(), e["occlusion"].std().item(),
          "mask max", e["mask"].max().item(), "deformation std", e["deformation"].std().item())
    for path in save_golden(out, "animate.pt"):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
