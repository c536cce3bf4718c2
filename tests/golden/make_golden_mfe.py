"""Generate the golden fixtures of the motion field estimator FROM THE REFERENCE ITSELF.

Run in the build container only (it needs /root/reference, absent on the GPU box):

    python tests/golden/make_golden_mfe.py

Imports the reference `modules.py` / `models.py` read-only (see make_golden.py).  The reference's
coordinate grids hard-code `.cuda()` (utils.py:81-82, 93-95, 134); this container has no GPU, so
for the duration of this script torch.Tensor.cuda is the identity (the arithmetic is unchanged:
CPU fp32).  Stores plain tensors in tests/golden/mfe.pt (in parts below 1 MiB, loaded with
weights_only=True) and the state-dict key lists in tests/golden/mfe_keys.json:

  down3d  DownBlock3D(16, 24, False) (modules.py:73-75) on x [2, 16, 3, 4, 6]
  up3d    UpBlock3D(24, 8, False) (modules.py:92-94) on x [2, 24, 3, 2, 3]
  mfe     MFE(False, [16, 16, 24], [24, 16, 8], K=3, D=4, C1=8, C2=3) (models.py:1040-1082) on
          fs [2, 8, 4, 8, 8], keypoints in [-1, 1], near-identity head rotations; the loss is
          sum(deformation * g_def) + sum(occlusion * g_occ) + sum(mask * g_mask)
All in training mode, seeded.  Per case: inputs, outputs, input gradients, parameter gradients,
the BN buffers after the step, the eval-mode output with those statistics, and `init_sum`
checksums of the initial parameters (the product modules draw the same RNG sequence as the
reference constructors, so torch.manual_seed(seed) + construction reproduces them).
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, save_golden  # noqa: E402

TOY = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)


def grads(mod):
    return {k: p.grad.detach().clone() for k, p in mod.named_parameters()}


def init_sums(mod):
    return {k: v.detach().double().sum() for k, v in mod.state_dict().items() if v.is_floating_point()}


def buffers(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items() if "running" in k or "num_batches" in k}


def block_case(ctor, seed, shape):
    torch.manual_seed(seed)
    blk = ctor().train()
    isum = init_sums(blk)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1))
    xr = x.clone().requires_grad_(True)
    y = blk(xr)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 2))
    (y * g).sum().backward()
    bufs = buffers(blk)
    blk.eval()
    with torch.no_grad():
        y_eval = blk(x)
    return dict(seed=torch.tensor(seed), x=x, g=g, out=y.detach(), dx=xr.grad.detach(), grads=grads(blk),
                buffers=bufs, out_eval=y_eval, init_sum=isum)


def near_identity(gen, n, utils):
    a = (torch.rand(n, 3, generator=gen) - 0.5) * 0.4
    return utils.rotation_matrix_y(a[:, 1]) @ utils.rotation_matrix_x(a[:, 0]) @ utils.rotation_matrix_z(a[:, 2])


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # reference grids call .cuda()
    modules, models, _ = import_reference()
    import utils  # noqa: E402  (reference)
    torch.set_num_threads(8)
    out = {}
    out["down3d"] = block_case(lambda: modules.DownBlock3D(16, 24, False), 51, (2, 16, 3, 4, 6))
    out["up3d"] = block_case(lambda: modules.UpBlock3D(24, 8, False), 61, (2, 24, 3, 2, 3))

    torch.manual_seed(71)
    mfe = models.MFE(False, **TOY).train()
    isum = init_sums(mfe)
    toy_keys = list(mfe.state_dict().keys())
    gen = torch.Generator().manual_seed(72)
    N, K, D = 2, TOY["K"], TOY["D"]
    fs = torch.randn(N, TOY["C1"], D, 8, 8, generator=gen)
    kp_s = (torch.rand(N, K, 3, generator=gen) - 0.5) * 2
    kp_d = (torch.rand(N, K, 3, generator=gen) - 0.5) * 2
    Rs, Rd = near_identity(gen, N, utils), near_identity(gen, N, utils)
    ins = [t.clone().requires_grad_(True) for t in (fs, kp_s, kp_d)]
    deformation, occlusion, mask = mfe(ins[0], ins[1], ins[2], Rs, Rd)
    g_def = torch.randn(deformation.shape, generator=gen)
    g_occ = torch.randn(occlusion.shape, generator=gen)
    g_mask = torch.randn(mask.shape, generator=gen)
    ((deformation * g_def).sum() + (occlusion * g_occ).sum() + (mask * g_mask).sum()).backward()
    bufs = buffers(mfe)
    mfe.eval()
    with torch.no_grad():
        e_def, e_occ, e_mask = mfe(fs, kp_s, kp_d, Rs, Rd)
    out["mfe"] = dict(seed=torch.tensor(71), fs=fs, kp_s=kp_s, kp_d=kp_d, Rs=Rs, Rd=Rd,
                      g_def=g_def, g_occ=g_occ, g_mask=g_mask,
                      deformation=deformation.detach(), occlusion=occlusion.detach(), mask=mask.detach(),
                      d_fs=ins[0].grad.clone(), d_kp_s=ins[1].grad.clone(), d_kp_d=ins[2].grad.clone(),
                      grads=grads(mfe), buffers=bufs,
                      eval_deformation=e_def, eval_occlusion=e_occ, eval_mask=e_mask, init_sum=isum)
    print("toy MFE parameters:", sum(p.numel() for p in mfe.parameters()))

    for path in save_golden(out, "mfe.pt"):      # in parts below 1 MiB (tests/golden_io.py)
        print("wrote", path, os.path.getsize(path), "bytes")

    torch.manual_seed(0)
    full = models.MFE()
    keys = dict(toy=toy_keys, toy_config=TOY, default=list(full.state_dict().keys()),
                default_shapes={k: list(v.shape) for k, v in full.state_dict().items()})
    kpath = os.path.join(HERE, "mfe_keys.json")
    with open(kpath, "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote", kpath, os.path.getsize(kpath), "bytes")


if __name__ == "__main__":
    main()
