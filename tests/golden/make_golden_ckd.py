"""Generate the golden fixtures of the canonical keypoint detector FROM THE REFERENCE ITSELF.

Run where the reference checkout is available (see make_golden.py), on the CPU:

    python tests/golden/make_golden_ckd.py

Imports the reference `modules.py` / `models.py` / `losses.py` / `utils.py` read-only.
`make_coordinate_grid_3d` calls `.cuda()` (utils.py:93-95); for the duration of this script
torch.Tensor.cuda is the identity (the arithmetic is unchanged: CPU fp32).  Stores plain tensors in
tests/golden/ckd.pt (in parts below 1 MiB, loaded with weights_only=True) and the state-dict key
lists in tests/golden/ckd_keys.json:

  softargmax  heatmap2kp(out2heatmap(z)) (utils.py:106-118) and dz for the loss sum(kp * G), seeded z
              [2, 3, 4, 8, 12] and [1, 15, 2, 5, 7] and seeded G
  resize      F.interpolate(x, mode="bilinear", scale_factor=s, align_corners=False,
              recompute_scale_factor=True) (models.py:978) on [2, 3, 64, 96] and [1, 3, 38, 50] at
              s = 0.25 and on [1, 3, 20, 36] at s = 0.5
  ckd         CKD(False, down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3) on a torch.rand image
              [2, 3, 64, 96]; the loss is sum(kp * g) with seeded g.  Inputs, kp, all parameter
              gradients, the BN buffers after the step, the eval-mode kp with those statistics,
              `init_sum` checksums of the initial parameters, and the largest voxel probability
              per keypoint (`peak`)
  losses      EquivarianceLoss, KeypointPriorLoss, DeformationPriorLoss (losses.py:198-240) with the
              gradients of their inputs on [3, 5, 3] keypoints; keypoints 0 and 1 of sample 0 are
              0.05 * sqrt(3) apart, below sqrt(Dt), so the hinge is active
All in training mode, seeded.

For `ckd` the script also runs a bf16 EMULATION of the reference: conv weights rounded to bf16, a
forward pre-hook on every conv and batch norm that rounds its input to bf16 straight-through
(x + (x.bfloat16().float() - x).detach()), and the same rounding of out_conv's output.  Its
deviation from the fp32 run is stored per output and per parameter gradient as rel-L2
(`emu_dev`); these numbers, not the product's own results, set the bf16 gates of
tests/test_ckd_gpu.py.
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, save_golden  # noqa: E402
from make_golden_hpe import buffers, grads, init_sums, rel_l2  # noqa: E402

TOY = dict(down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3)
CONVS = (torch.nn.Conv2d, torch.nn.Conv3d)


def ste(t):
    return t + (t.bfloat16().float() - t).detach()


def ckd_run(models, x, g, emulate):
    torch.manual_seed(101)
    net = models.CKD(False, **TOY).train()
    isum = init_sums(net)
    if emulate:
        for m in net.modules():
            if isinstance(m, CONVS + (torch.nn.modules.batchnorm._BatchNorm,)):
                m.register_forward_pre_hook(lambda _, args: (ste(args[0]),))
            if isinstance(m, CONVS):
                m.weight.data = m.weight.data.bfloat16().float()
        net.out_conv.register_forward_hook(lambda _, args, out: ste(out))
    net.out_conv.register_forward_hook(lambda _, args, out: net.__dict__.__setitem__("logits", out.detach()))
    kp = net(x)
    (kp * g).sum().backward()
    return net, isum, kp.detach()


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # make_coordinate_grid_3d calls .cuda()
    modules, models, losses = import_reference()
    import utils  # noqa: E402  (reference)
    torch.set_num_threads(8)
    out = {}

    gen = torch.Generator().manual_seed(111)
    sam = {}
    for name, shape in (("a", (2, 3, 4, 8, 12)), ("b", (1, 15, 2, 5, 7))):
        z = torch.randn(shape, generator=gen).requires_grad_(True)
        G = torch.randn(shape[0], shape[1], 3, generator=gen)
        kp = utils.heatmap2kp(utils.out2heatmap(z))
        (kp * G).sum().backward()
        sam[name] = dict(z=z.detach().clone(), G=G, kp=kp.detach(), dz=z.grad.clone())
    out["softargmax"] = sam

    rs = {}
    for name, shape, s in (("a", (2, 3, 64, 96), 0.25), ("b", (1, 3, 38, 50), 0.25), ("c", (1, 3, 20, 36), 0.5)):
        x = torch.rand(shape, generator=gen)
        y = F.interpolate(x, mode="bilinear", scale_factor=s, align_corners=False, recompute_scale_factor=True)
        rs[name] = dict(x=x, scale=torch.tensor(s), y=y)
    out["resize"] = rs

    gen = torch.Generator().manual_seed(102)
    x = torch.rand(2, 3, 64, 96, generator=gen)
    g = torch.randn(2, TOY["K"], 3, generator=gen)
    net, isum, kp = ckd_run(models, x, g, False)
    toy_keys = list(net.state_dict().keys())
    g32 = grads(net)
    bufs = buffers(net)
    peak = utils.out2heatmap(net.logits).flatten(2).max(dim=2).values   # how peaked the case is
    net.eval()
    with torch.no_grad():
        kp_eval = net(x)
    emu, _, ekp = ckd_run(models, x, g, True)
    ge = grads(emu)
    emu_dev = {"out": {"kp": rel_l2(ekp, kp)}, "grads": {k: rel_l2(ge[k], g32[k]) for k in g32}}
    out["ckd"] = dict(seed=torch.tensor(101), x=x, g=g, out=kp, grads=g32, buffers=bufs, out_eval=kp_eval,
                      init_sum=isum, emu_dev=emu_dev, peak=peak)
    print("toy CKD parameters:", sum(p.numel() for p in net.parameters()), "keys:", len(toy_keys))
    print("largest voxel probability per keypoint:", peak.tolist())
    print("bf16 emulation rel-L2, kp:", float(emu_dev["out"]["kp"]))
    print("bf16 emulation rel-L2, gradients:", {k: float(v) for k, v in emu_dev["grads"].items()})

    gen = torch.Generator().manual_seed(105)
    kp = (torch.rand(3, 5, 3, generator=gen) - 0.5) * 2
    kp[0, 1] = kp[0, 0] + 0.05
    rev = kp[:, :, :2] + 0.1 * torch.randn(3, 5, 2, generator=gen)
    delta = 0.1 * torch.randn(3, 5, 3, generator=gen)
    ls = {}
    a, b = kp.clone().requires_grad_(True), rev.clone().requires_grad_(True)
    loss = losses.EquivarianceLoss()(a, b)
    loss.backward()
    ls["equivariance"] = dict(loss=loss.detach(), d_kp=a.grad.clone(), d_rev=b.grad.clone())
    a = kp.clone().requires_grad_(True)
    loss = losses.KeypointPriorLoss()(a)
    loss.backward()
    ls["prior"] = dict(loss=loss.detach(), d_kp=a.grad.clone())
    a = delta.clone().requires_grad_(True)
    loss = losses.DeformationPriorLoss()(a)
    loss.backward()
    ls["deformation"] = dict(loss=loss.detach(), d_delta=a.grad.clone())
    out["losses"] = dict(kp=kp, rev=rev, delta=delta, **ls)

    for path in save_golden(out, "ckd.pt"):      # in parts below 1 MiB (tests/golden_io.py)
        print("wrote", path, os.path.getsize(path), "bytes")

    torch.manual_seed(0)
    full = models.CKD()
    keys = dict(toy=toy_keys, toy_config=TOY, toy_shapes={k: list(v.shape) for k, v in net.state_dict().items()},
                toy_params=sum(p.numel() for p in net.parameters()),
                default=list(full.state_dict().keys()),
                default_shapes={k: list(v.shape) for k, v in full.state_dict().items()},
                default_params=sum(p.numel() for p in full.parameters()))
    kpath = os.path.join(HERE, "ckd_keys.json")
    with open(kpath, "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote", kpath, os.path.getsize(kpath), "bytes")


if __name__ == "__main__":
    main()
