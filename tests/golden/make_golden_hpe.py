"""Generate the golden fixtures of the head pose estimator FROM THE REFERENCE ITSELF.

Run where the reference checkout is available (see make_golden.py), on the CPU:

    python tests/golden/make_golden_hpe.py

Imports the reference `modules.py` / `models.py` / `losses.py` / `utils.py` read-only.
`HPE_EDE.__init__` calls `.cuda()` (models.py:1014); for the duration of this script
torch.Tensor.cuda is the identity (the arithmetic is unchanged: CPU fp32).  Stores plain tensors in
tests/golden/hpe.pt (in parts below 1 MiB, loaded with weights_only=True) and the state-dict key
lists in tests/golden/hpe_keys.json:

  stem        Sequential(ConvBlock2D("CNA", 3, 16, 7, 2, 3, False), MaxPool2d(3, 2, 1)) on [2, 3, 32, 48]
  bneck_id    ResBottleneck(32, 32, 1, False) on [2, 32, 8, 12]
  bneck_proj  ResBottleneck(16, 32, 1, False) on [2, 16, 8, 12]
  bneck_s2    ResBottleneck(32, 64, 2, False) on [2, 32, 8, 12]
  hpe         HPE_EDE(False, [16, 32, 64], [1, 1], n_bins=6, K=3) on [2, 3, 32, 48]; the loss is
              sum_i (output_i * g_i).sum() with seeded g_i
  pose        transform_kp (utils.py:53-59) on [3, 5, 3] keypoints with the gradients of all six
              inputs, and HeadPoseLoss (losses.py:224-231)
All in training mode, seeded.  Per case: inputs, outputs, parameter gradients, the input gradient
(not for stem / hpe: the image is data), the BN buffers after the step, the eval-mode output with
those statistics, and `init_sum` checksums of the initial parameters.

For `hpe` the script also runs a bf16 EMULATION of the reference: conv weights rounded to bf16 and
a forward pre-hook on every conv and batch norm that rounds its input to bf16 straight-through
(x + (x.bfloat16().float() - x).detach()).  Its deviation from the fp32 run is stored per output
and per parameter gradient as rel-L2 (`emu_dev`); these numbers, not the product's own results,
set the bf16 gates of tests/test_hpe_gpu.py.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, save_golden  # noqa: E402

TOY = dict(n_filters=[16, 32, 64], n_blocks=[1, 1], n_bins=6, K=3)
OUT_NAMES = ("yaw", "pitch", "roll", "t", "scale")


def grads(mod):
    return {k: p.grad.detach().clone() for k, p in mod.named_parameters()}


def init_sums(mod):
    return {k: v.detach().double().sum() for k, v in mod.state_dict().items() if v.is_floating_point()}


def buffers(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items() if "running" in k or "num_batches" in k}


def block_case(ctor, seed, shape, input_grad=True):
    torch.manual_seed(seed)
    blk = ctor().train()
    isum = init_sums(blk)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1))
    xr = x.clone().requires_grad_(input_grad)
    y = blk(xr)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 2))
    (y * g).sum().backward()
    bufs = buffers(blk)
    blk.eval()
    with torch.no_grad():
        y_eval = blk(x)
    out = dict(seed=torch.tensor(seed), x=x, g=g, out=y.detach(), grads=grads(blk), buffers=bufs, out_eval=y_eval,
               init_sum=isum)
    if input_grad:
        out["dx"] = xr.grad.detach()
    return out


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).float()


def hpe_run(models, x, gs, emulate):
    torch.manual_seed(91)
    net = models.HPE_EDE(False, **TOY).train()
    isum = init_sums(net)
    if emulate:
        def ste(_, args):
            t = args[0]
            return (t + (t.bfloat16().float() - t).detach(),)
        for m in net.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.modules.batchnorm._BatchNorm)):
                m.register_forward_pre_hook(ste)
            if isinstance(m, torch.nn.Conv2d):
                m.weight.data = m.weight.data.bfloat16().float()
    outs = net(x)
    sum((o * g).sum() for o, g in zip(outs, gs)).backward()
    return net, isum, [o.detach() for o in outs]


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # HPE_EDE.__init__ calls .cuda()
    modules, models, losses = import_reference()
    import utils  # noqa: E402  (reference)
    torch.set_num_threads(8)
    out = {}
    out["stem"] = block_case(lambda: torch.nn.Sequential(modules.ConvBlock2D("CNA", 3, 16, 7, 2, 3, False),
                                                         torch.nn.MaxPool2d(3, 2, 1)), 81, (2, 3, 32, 48), False)
    out["bneck_id"] = block_case(lambda: modules.ResBottleneck(32, 32, 1, False), 83, (2, 32, 8, 12))
    out["bneck_proj"] = block_case(lambda: modules.ResBottleneck(16, 32, 1, False), 85, (2, 16, 8, 12))
    out["bneck_s2"] = block_case(lambda: modules.ResBottleneck(32, 64, 2, False), 87, (2, 32, 8, 12))

    gen = torch.Generator().manual_seed(92)
    x = torch.rand(2, 3, 32, 48, generator=gen)
    shapes = ((2,), (2,), (2,), (2, 3), (2, 1, 1, 1))
    gs = [torch.randn(s, generator=gen) for s in shapes]
    net, isum, outs = hpe_run(models, x, gs, False)
    toy_keys = list(net.state_dict().keys())
    g32 = grads(net)
    bufs = buffers(net)
    net.eval()
    with torch.no_grad():
        outs_eval = net(x)
    emu, _, eouts = hpe_run(models, x, gs, True)
    ge = grads(emu)
    emu_dev = {"out": {n: rel_l2(a, b) for n, a, b in zip(OUT_NAMES, eouts, outs)},
               "grads": {k: rel_l2(ge[k], g32[k]) for k in g32}}
    out["hpe"] = dict(seed=torch.tensor(91), x=x, g=dict(zip(OUT_NAMES, gs)), out=dict(zip(OUT_NAMES, outs)),
                      grads=g32, buffers=bufs, out_eval=dict(zip(OUT_NAMES, outs_eval)), init_sum=isum,
                      emu_dev=emu_dev)
    print("toy HPE_EDE parameters:", sum(p.numel() for p in net.parameters()), "keys:", len(toy_keys))
    print("bf16 emulation rel-L2, outputs:", {k: float(v) for k, v in emu_dev["out"].items()})
    print("bf16 emulation rel-L2, gradients: max", max(float(v) for v in emu_dev["grads"].values()))

    gen = torch.Generator().manual_seed(95)
    kp = (torch.rand(3, 5, 3, generator=gen) - 0.5) * 2
    ang = [(torch.rand(3, generator=gen) - 0.5) * 1.5 for _ in range(3)]
    t = torch.randn(3, 3, generator=gen) * 0.1
    scale = 1 + 0.2 * torch.randn(3, 1, 1, 1, generator=gen)
    ins = [v.clone().requires_grad_(True) for v in [kp] + ang + [t, scale]]
    kp_t, R = utils.transform_kp(*ins)
    g_kp = torch.randn(kp_t.shape, generator=gen)
    g_R = torch.randn(R.shape, generator=gen)
    ((kp_t * g_kp).sum() + (R * g_R).sum()).backward()
    real = [(torch.rand(3, generator=gen) - 0.5) * 1.5 for _ in range(3)]
    est = [a.clone().requires_grad_(True) for a in ang]
    loss = losses.HeadPoseLoss()(*est, *real)
    loss.backward()
    names = ("kp", "yaw", "pitch", "roll", "t", "scale")
    out["pose"] = dict(inputs=dict(zip(names, [kp] + ang + [t, scale])), g_kp=g_kp, g_R=g_R, kp_out=kp_t.detach(),
                       R=R.detach(), d_inputs={n: v.grad.clone() for n, v in zip(names, ins)},
                       real=dict(zip(names[1:4], real)), loss=loss.detach(),
                       d_loss={n: v.grad.clone() for n, v in zip(names[1:4], est)})

    for path in save_golden(out, "hpe.pt"):      # in parts below 1 MiB (tests/golden_io.py)
        print("wrote", path, os.path.getsize(path), "bytes")

    torch.manual_seed(0)
    full = models.HPE_EDE()
    keys = dict(toy=toy_keys, toy_config=TOY, toy_shapes={k: list(v.shape) for k, v in net.state_dict().items()},
                default=list(full.state_dict().keys()),
                default_shapes={k: list(v.shape) for k, v in full.state_dict().items()})
    kpath = os.path.join(HERE, "hpe_keys.json")
    with open(kpath, "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote", kpath, os.path.getsize(kpath), "bytes")


if __name__ == "__main__":
    main()
