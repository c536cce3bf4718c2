"""Generate the golden fixtures of the patch discriminator and the adversarial training step
FROM THE REFERENCE ITSELF.

Run in the build container only (it needs /root/reference):

    python tests/golden/make_golden_disc.py

The reference's coordinate grid hard-codes `.cuda()` (utils.py:81-82); this container has no
GPU, so for the duration of this script torch.Tensor.cuda is the identity (the arithmetic is
unchanged: CPU fp32).  `losses.py` imports torchvision at the top; make_golden.import_reference
registers an inert placeholder.  Only plain tensors are stored (tests/golden_io.save_golden).

  discriminator.pt
    models.Discriminator(True, [8, 16, 32, 64], K=2) under torch.manual_seed(11), training mode,
    x_real / x_fake [2, 3, 32, 48] in [0, 1), kp [2, 2, 3] in [-1, 1]:
      init         the initial state dict
      real / fake  output and the four features of D(x_real), then D(x_fake)
      G, F         GANLoss(out_fake, True, False), FeatureMatchingLoss(feat_fake, feat_real)
      g_grads      gradients of G + 10 F w.r.t. x_fake ("x_fake") and every parameter
      G1, G2       GANLoss(out_fake, False, True), GANLoss(out_real, True, True) of a fresh
                   D(x_real), D(x_fake.detach()) pair (models as trainer.py:330-337), whose
                   outputs are real2 / fake2
      d_grads      gradients of G1 + G2 w.r.t. every parameter
      uv           the spectral-norm u / v buffers after the four forwards
    block: ConvBlock2D("CNA", 5, 16, 3, 2, 1, True, "instance", "leakyrelu") under
      torch.manual_seed(12) on x [3, 5, 20, 28]: init, x, output, the output gradient g and the
      gradients of sum(out * g) w.r.t. x and every parameter, u / v afterwards.

  adv_toy_step.pt
    The toy FaceVAE composition of make_golden.py (64^2, B = 4, torch.manual_seed(0)) with
    Discriminator(True, [8, 16, 32, 64], K=0) built right after it and kp = zeros(4, 0, 3);
    weights w_R = w_K = w_G = 1, w_F = 10, one torch.optim.Adam(lr=5e-5, betas=(0.5, 0.999)) per
    model; two iterations of logger.py:150-172 (generator update, then discriminator update):
      init_g / init_d, x, eps, losses [2, 6] (R, K, G, F, G1, G2 per iteration, weighted),
      d_grads1 (the discriminator's gradients of iteration 1), state_g / state_d after iteration 2.

  disc_keys.json   the state-dict keys of the default Discriminator().
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import TOY, RefFaceVAE, import_reference, inputs, save_golden  # noqa: E402

DOWN = [8, 16, 32, 64]


def clone_state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def grads_of(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def make_discriminator(modules, models, losses):
    torch.manual_seed(11)
    D = models.Discriminator(True, DOWN, K=2).train()
    out = dict(init=clone_state(D))
    g = torch.Generator().manual_seed(21)
    x_real = torch.rand(2, 3, 32, 48, generator=g)
    x_fake = torch.rand(2, 3, 32, 48, generator=g)
    kp = torch.rand(2, 2, 3, generator=g) * 2 - 1
    out.update(x_real=x_real, x_fake=x_fake, kp=kp)
    gan, fm = losses.GANLoss(), losses.FeatureMatchingLoss()

    xf = x_fake.clone().requires_grad_(True)
    o_r, f_r = D(x_real, kp)
    o_f, f_f = D(xf, kp)
    out["real"] = dict(output=o_r.detach().clone(), features=[t.detach().clone() for t in f_r])
    out["fake"] = dict(output=o_f.detach().clone(), features=[t.detach().clone() for t in f_f])
    G = gan(o_f, True, False)
    Fm = fm(f_f, f_r)
    (G + 10 * Fm).backward()
    out["G"], out["F"] = G.detach().clone(), Fm.detach().clone()
    out["g_grads"] = dict(x_fake=xf.grad.detach().clone(), **grads_of(D))

    D.zero_grad(set_to_none=True)
    o_r, _ = D(x_real, kp)
    o_f, _ = D(x_fake.detach(), kp)
    G1, G2 = gan(o_f, False, True), gan(o_r, True, True)
    (G1 + G2).backward()
    out["G1"], out["G2"] = G1.detach().clone(), G2.detach().clone()
    out["real2"], out["fake2"] = o_r.detach().clone(), o_f.detach().clone()
    out["d_grads"] = grads_of(D)
    out["uv"] = {k: v.detach().clone() for k, v in D.state_dict().items() if k.endswith(("weight_u", "weight_v"))}

    torch.manual_seed(12)
    blk = modules.ConvBlock2D("CNA", 5, 16, 3, 2, 1, True, "instance", "leakyrelu").train()
    b = dict(init=clone_state(blk))
    x = torch.randn(3, 5, 20, 28, generator=g)
    xr = x.clone().requires_grad_(True)
    y = blk(xr)
    gy = torch.randn(y.shape, generator=g)
    (y * gy).sum().backward()
    b.update(x=x, out=y.detach().clone(), g=gy, grads=dict(x=xr.grad.detach().clone(), **grads_of(blk)),
             uv={k: v.detach().clone() for k, v in blk.state_dict().items() if k.endswith(("weight_u", "weight_v"))})
    out["block"] = b
    print("discriminator.pt:", save_golden(out, "discriminator.pt"))


def make_adv_step(models, losses):
    torch.manual_seed(0)
    net = RefFaceVAE(models, TOY).train()
    D = models.Discriminator(True, DOWN, K=0).train()
    out = dict(init_g=clone_state(net), init_d=clone_state(D))
    opt_g = torch.optim.Adam(net.parameters(), lr=5e-5, betas=(0.5, 0.999))
    opt_d = torch.optim.Adam(D.parameters(), lr=5e-5, betas=(0.5, 0.999))
    kl, rec, gan, fm = losses.KLDivergenceLoss(), losses.ReconLoss(), losses.GANLoss(), losses.FeatureMatchingLoss()
    x, eps = inputs(TOY)
    kp = torch.zeros(x.shape[0], 0, 3)
    out.update(x=x, eps=eps)
    hist = []
    for it in range(2):
        opt_g.zero_grad()
        y, mu, logstd, _ = net(x, eps)
        o_r, f_r = D(x, kp)
        o_f, f_f = D(y, kp)
        lg = dict(R=1.0 * rec((x, y)), K=1.0 * kl((mu, logstd)), G=1.0 * gan(o_f, True, False), F=10.0 * fm(f_f, f_r))
        sum(lg.values()).backward()
        opt_g.step()
        opt_g.zero_grad()
        opt_d.zero_grad()
        o_r, _ = D(x, kp)
        o_f, _ = D(y.detach(), kp)
        ld = dict(G1=gan(o_f, False, True), G2=gan(o_r, True, True))
        sum(ld.values()).backward()
        if it == 0:
            out["d_grads1"] = grads_of(D)
        opt_d.step()
        opt_d.zero_grad()
        hist.append(torch.stack([v.detach() for v in list(lg.values()) + list(ld.values())]))
    out["losses"] = torch.stack(hist)
    out["state_g"], out["state_d"] = clone_state(net), clone_state(D)
    print("adv_toy_step.pt:", save_golden(out, "adv_toy_step.pt"))


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # the reference's grid calls .cuda()
    modules, models, losses = import_reference()
    make_discriminator(modules, models, losses)
    make_adv_step(models, losses)
    with open(os.path.join(HERE, "disc_keys.json"), "w") as f:
        json.dump(list(models.Discriminator().state_dict().keys()), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
