"""Generate the golden fixtures of the expression feature extractor FROM THE REFERENCE ITSELF.

Run where the reference checkout is available (see make_golden.py), on the CPU:

    python tests/golden/make_golden_efe.py

Imports the reference `modules.py` / `models.py` / `losses.py` / `utils.py` read-only (it copies
none of their text).  `make_coordinate_grid_3d` calls `.cuda()` (utils.py:93-95); for the duration
of this script torch.Tensor.cuda is the identity (the arithmetic is unchanged: CPU fp32), and
torch.randn is wrapped so that the noise flatten_vae_nl draws (models.py:561) is recorded.  Stores
plain tensors in tests/golden/efe.pt (in parts below 1 MiB, loaded with weights_only=True) and the
state-dict key lists in tests/golden/efe_keys.json:

  kpcat        torch.cat((z, kp2gaussian_3d(kpc, z.shape[2:])), 1) (models.py:790-791) and dz, dkpc for
               the loss sum(out * G), seeded z, kpc and G, on [2, 3, 4, 8, 12], [1, 15, 2, 5, 7],
               [1, 1, 2, 3, 4] (K = 1) and [2, 4, 3, 4, 6] (2K = 8: no pad channels).  In the first two
               one keypoint has a coordinate 1.5, outside the grid, and one sits exactly on a grid node
  resblock     ResBlock3D(30) on [1, 30, 4, 4, 64] and [1, 30, 5, 4, 64], ResBlock3D(6) on [2, 6, 4, 8, 8]
               and SameBlock3D(30, 15) on [1, 30, 2, 4, 64], with the batch-norm weights and biases
               re-drawn (perturb_bn: the test draws the same): output, input gradient, parameter
               gradients, BN buffers, eval-mode output
  efe          EFE_conv5(False, down_seq=[3, 8, 16, 32], up_seq=[16, 8, 8], D=4, K=3, n_res=2) built
               with seed 231, mix_out's batch-norm weight then multiplied by 0.1 (unscaled, the BN +
               ReLU in front of the T = 0.1 softmax saturates the toy's heatmap); x, x_a [2, 3, 64, 64],
               kpc in +-0.6; loss sum(kp * g), plus KLDivergenceLoss when train_vae.  One run with
               train_vae None and one with True: inputs, the recorded eps, all outputs, dkpc, all
               parameter gradients, the BN buffers, the eval-mode kp, `init_sum`, the largest voxel
               probability per keypoint (`peak`) and `emu_dev`
  contrastive  ContrastiveLoss_linear in both modes on [4, 32, 4, 4] pairs: loss, input and parameter
               gradients (of the 512 x 512 weights every 16th row: one whole is 1 MiB), BN buffers
All in training mode, seeded.

`emu_dev` is the deviation (rel-L2, per output and per parameter gradient) of a bf16 EMULATION of
the reference from its fp32 run: conv weights rounded to bf16, a forward pre-hook on every conv and
batch norm that rounds its input to bf16 straight-through, and the same rounding of the outputs of
`down`, `out_conv` and `mix_out`.  These numbers, not the product's own results, set the bf16 gates
of tests/test_efe_gpu.py.  The script asserts two conditions of the case (they are not
measurements): the largest voxel probability per keypoint is at most 0.5, and at most 2 of the
live parameter gradients (max |g| above 1e-4 of the largest) have an emulation deviation above 1/3.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, save_golden  # noqa: E402
from make_golden_hpe import buffers, grads, init_sums, rel_l2  # noqa: E402

TOY = dict(down_seq=[3, 8, 16, 32], up_seq=[16, 8, 8], D=4, K=3, n_res=2)
SEED = 231
MIX_OUT_BN = "mix_out.layers.layers.1.weight"
CONVS = (torch.nn.Conv2d, torch.nn.Conv3d)
DRAWS = []
GRAD_ROW_STEP = 16


def ste(t):
    return t + (t.bfloat16().float() - t).detach()


def perturb_bn(mod, seed):
    """Re-draw every batch norm's weight in [0.5, 1.5] and bias from N(0, 0.5) (module order)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if hasattr(m, "running_mean") and getattr(m, "weight", None) is not None:
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.5)


def block_case(ctor, seed, shape):
    torch.manual_seed(seed)
    blk = ctor().train()
    isum = init_sums(blk)
    perturb_bn(blk, seed + 3)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(*shape, generator=gen)
    xr = x.clone().requires_grad_(True)
    y = blk(xr)
    g = torch.randn(y.shape, generator=gen)
    (y * g).sum().backward()
    bufs = buffers(blk)
    blk.eval()
    with torch.no_grad():
        y_eval = blk(x)
    return dict(seed=torch.tensor(seed), x=x, g=g, out=y.detach(), dx=xr.grad.detach(), grads=grads(blk), buffers=bufs,
                out_eval=y_eval, init_sum=isum)


def kpcat_case(utils, gen, shape, special):
    N, K, D, H, W = shape
    z = torch.randn(shape, generator=gen).requires_grad_(True)
    kpc = (torch.rand(N, K, 3, generator=gen) - 0.5) * 1.8
    grid = utils.make_coordinate_grid_3d((D, H, W))
    if special:
        kpc[0, 0] = grid[D - 1, H // 2, W // 3]          # exactly on a grid node
        kpc[N - 1, K - 1, 1] = 1.5                         # outside the grid
    kpc.requires_grad_(True)
    out = torch.cat((z, utils.kp2gaussian_3d(kpc, spatial_size=shape[2:])), dim=1)
    G = torch.randn(out.shape, generator=gen)
    (out * G).sum().backward()
    return dict(z=z.detach().clone(), kpc=kpc.detach().clone(), G=G, out=out.detach(), dz=z.grad.clone(),
                dkpc=kpc.grad.clone())


def efe_run(models, losses, utils, inp, train_vae, emulate):
    torch.manual_seed(SEED)
    net = models.EFE_conv5(False, **TOY).train()
    isum = init_sums(net)
    with torch.no_grad():
        dict(net.named_parameters())[MIX_OUT_BN].mul_(0.1)
    if emulate:
        for m in net.modules():
            if isinstance(m, CONVS + (torch.nn.modules.batchnorm._BatchNorm,)):
                m.register_forward_pre_hook(lambda _, args: (ste(args[0]),))
            if isinstance(m, CONVS):
                m.weight.data = m.weight.data.bfloat16().float()
        for m in (net.down, net.out_conv, net.mix_out):
            m.register_forward_hook(lambda _, args, out: ste(out))
    net.mix_out.register_forward_hook(lambda _, args, out: net.__dict__.__setitem__("logits", out.detach()))
    kpc = inp["kpc"].clone().requires_grad_(True)
    torch.manual_seed(SEED + 1)
    del DRAWS[:]
    kp, x_c, x_a_c, (mu, ls), (x_vae, x_hat) = net(inp["x"], inp["x_a"], kpc, train_vae)
    eps = DRAWS[-1].view(-1, 16, 4, 4).clone()           # the one draw of the forward: flatten_vae_nl's
    loss = (kp * inp["g"]).sum()
    if train_vae:
        loss = loss + losses.KLDivergenceLoss()((mu, ls))
    loss.backward()
    outs = dict(kp=kp, x_c=x_c, x_a_c=x_a_c, x_vae=x_vae, x_hat=x_hat)
    if train_vae:
        outs.update(mu=mu, logstd=ls)
    outs = {k: v.detach().clone() for k, v in outs.items()}
    return net, isum, eps, outs, kpc.grad.clone()


def efe_case(models, losses, utils, inp, train_vae):
    net, isum, eps, outs, dkpc = efe_run(models, losses, utils, inp, train_vae, False)
    g32, bufs = grads(net), buffers(net)
    peak = utils.out2heatmap(net.logits).flatten(2).max(dim=2).values
    net.eval()
    with torch.no_grad():
        kp_eval = net(inp["x"], None, inp["kpc"], None)[0]
    emu, _, eeps, eouts, edkpc = efe_run(models, losses, utils, inp, train_vae, True)
    assert torch.equal(eps, eeps)
    ge = grads(emu)
    emu_dev = {"out": {k: rel_l2(eouts[k], outs[k]) for k in outs}, "dkpc": rel_l2(edkpc, dkpc),
               "grads": {k: rel_l2(ge[k], g32[k]) for k in g32}}
    top = max(float(v.abs().max()) for v in g32.values())
    live = [k for k, v in g32.items() if float(v.abs().max()) > 1e-4 * top]
    loose = [k for k in live if float(emu_dev["grads"][k]) > 1 / 3]
    tag = "train_vae" if train_vae else "no_vae"
    print(f"[{tag}] largest voxel probability per keypoint:", peak.tolist())
    print(f"[{tag}] bf16 emulation rel-L2, outputs:", {k: float(v) for k, v in emu_dev["out"].items()},
          "dkpc:", float(emu_dev["dkpc"]))
    print(f"[{tag}] bf16 emulation rel-L2, gradients: max over {len(live)} live keys",
          max(float(emu_dev["grads"][k]) for k in live), "above 1/3:", loose)
    assert float(peak.max()) <= 0.5, "the case saturates the heatmap: pick another seed"
    assert len(loose) <= 2, "the bf16 emulation moves too many gradients: pick another seed"
    return net, dict(eps=eps, out=outs, dkpc=dkpc, grads=g32, buffers=bufs, kp_eval=kp_eval, init_sum=isum, peak=peak,
                     emu_dev=emu_dev)


def contrastive_case(losses, mode, seed):
    torch.manual_seed(seed)
    crit = losses.ContrastiveLoss_linear(mode=mode).train()
    isum = init_sums(crit)
    perturb_bn(crit, seed + 3)
    gen = torch.Generator().manual_seed(seed + 1)
    f1 = torch.randn(4, 32, 4, 4, generator=gen).requires_grad_(True)
    f2 = torch.randn(4, 32, 4, 4, generator=gen).requires_grad_(True)
    loss = crit(f1, f2)
    loss.backward()
    # a 512 x 512 gradient alone is 1 MiB, the size limit of a committed file: rows 0, 16, 32, ... of those
    gr = {k: (p.grad[::GRAD_ROW_STEP] if p.grad.dim() == 2 else p.grad).detach().clone()
          for k, p in crit.named_parameters() if p.grad is not None}
    return crit, dict(seed=torch.tensor(seed), f1=f1.detach().clone(), f2=f2.detach().clone(), loss=loss.detach(),
                      d_f1=f1.grad.clone(), d_f2=f2.grad.clone(), grads=gr, buffers=buffers(crit), init_sum=isum)


def key_info(mod):
    return dict(keys=list(mod.state_dict().keys()), shapes={k: list(v.shape) for k, v in mod.state_dict().items()},
                params=sum(p.numel() for p in mod.parameters()))


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # make_coordinate_grid_3d calls .cuda()
    randn = torch.randn

    def recording_randn(*a, **k):
        t = randn(*a, **k)
        DRAWS.append(t.detach().clone())
        return t
    modules, models, losses = import_reference()
    import utils  # noqa: E402  (reference)
    torch.set_num_threads(8)
    out = {}

    gen = torch.Generator().manual_seed(241)
    out["kpcat"] = {name: kpcat_case(utils, gen, shape, special)
                    for name, shape, special in (("a", (2, 3, 4, 8, 12), True), ("b", (1, 15, 2, 5, 7), True),
                                                 ("k1", (1, 1, 2, 3, 4), False), ("k4", (2, 4, 3, 4, 6), False))}

    out["resblock"] = dict(
        c30_d4=block_case(lambda: modules.ResBlock3D(30, False), 251, (1, 30, 4, 4, 64)),
        c30_d5=block_case(lambda: modules.ResBlock3D(30, False), 255, (1, 30, 5, 4, 64)),
        c6=block_case(lambda: modules.ResBlock3D(6, False), 259, (2, 6, 4, 8, 8)),
        same30to15=block_case(lambda: modules.SameBlock3D(30, 15, False), 263, (1, 30, 2, 4, 64)))

    gen = torch.Generator().manual_seed(201)
    inp = dict(x=torch.rand(2, 3, 64, 64, generator=gen), x_a=torch.rand(2, 3, 64, 64, generator=gen),
               kpc=(torch.rand(2, TOY["K"], 3, generator=gen) - 0.5) * 1.2, g=torch.randn(2, TOY["K"], 3, generator=gen))
    torch.randn = recording_randn
    try:
        net, no_vae = efe_case(models, losses, utils, inp, None)
        _, with_vae = efe_case(models, losses, utils, inp, True)
    finally:
        torch.randn = randn
    out["efe"] = dict(seed=torch.tensor(SEED), **inp, no_vae=no_vae, train_vae=with_vae)
    print("toy EFE_conv5 parameters:", sum(p.numel() for p in net.parameters()), "keys:", len(net.state_dict()))

    con = {}
    for mode, seed in (("direction", 271), ("non-direction", 275)):
        crit, con[mode.replace("-", "_")] = contrastive_case(losses, mode, seed)
    out["contrastive"] = con

    for path in save_golden(out, "efe.pt"):      # in parts below 1 MiB (tests/golden_io.py)
        print("wrote", path, os.path.getsize(path), "bytes")

    torch.manual_seed(0)
    keys = dict(toy_config=TOY, toy=key_info(net), default=key_info(models.EFE_conv5()),
                same3d_30_15=key_info(modules.SameBlock3D(30, 15, False)),
                res3d_30=key_info(modules.ResBlock3D(30, False)),
                contrastive_default=key_info(losses.ContrastiveLoss_linear(mode="non-direction")),
                contrastive_direction=key_info(losses.ContrastiveLoss_linear()))
    for k in ("toy", "default", "same3d_30_15", "res3d_30", "contrastive_default"):
        print(k, "keys:", len(keys[k]["keys"]), "parameters:", keys[k]["params"])
    kpath = os.path.join(HERE, "efe_keys.json")
    with open(kpath, "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote", kpath, os.path.getsize(kpath), "bytes")


if __name__ == "__main__":
    main()
