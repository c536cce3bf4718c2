"""Launch-family timing of the expression feature extractor: the default EFE_conv5() on 256 x 256
images, N = 2, bf16 -- the whole forward and forward + backward (with x_a and the VAE), and the parts
this module adds to the CKD-shaped chain.

    python tools/efebench.py [--batch 2] [--window 0.3] [--no-model] [--out profiles/efe/efebench.json]

Prints ONE JSON line, also written to --out (default profiles/efe/efebench.json).  Times are device
events over a warm-up and a timed window of at least --window seconds; the torch comparisons run in
alternating windows and report medians.

  kpcat_fwd / kpcat_bwd  fv_efe_kpcat_fwd and the two launches of fv_efe_kpcat_bwd on the logits
                         [N, 15, 16, 64, 64]; `vs_copy` = the time of a device-to-device copy moving the
                         same bytes / the pass time; beside the torch expression they replace
                         (cat(z, exp(-0.5 |grid - kp|^2 / var)), with autograd for the backward).
  mix_block              one ResBlock3D(30) of `mix` on the padded [N, 32, 16, 64, 64] volume beside the
                         AFE's ResBlock3D(32) on the same shape: the same conv and BN kernels, plus the
                         per-forward zero-padding of the 30-channel weights; `ratio` = mix / afe.
  mix_out                SameBlock3D(30, 15) on the padded volume.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import ops_efe  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ckdbench import med, vs_copy, window_time  # noqa: E402

CL3 = torch.channels_last_3d
BF16 = torch.bfloat16
VAR = 0.01


def bench_kpcat(shape, window, g, rounds=5):
    N, K, D, H, W = shape
    cp = fv.ops.pad_pow2(2 * K)
    z = torch.randn(shape, generator=g, device="cuda").to(BF16).contiguous(memory_format=CL3)
    kpc = (torch.rand(N, K, 3, generator=g, device="cuda") - 0.5) * 1.2
    G = torch.randn((N, cp, D, H, W), generator=g, device="cuda").to(BF16).contiguous(memory_format=CL3)
    new_f = lambda: ops_efe.kpcat_forward(z, kpc)                          # noqa: E731
    new_b = lambda: ops_efe.kpcat_backward(G, kpc, K)                      # noqa: E731
    lin = lambda n: 2 * (torch.arange(n, device="cuda", dtype=torch.float32) / (n - 1)) - 1   # noqa: E731
    grid = torch.stack([lin(W).view(1, 1, W).expand(D, H, W), lin(H).view(1, H, 1).expand(D, H, W),
                        lin(D).view(D, 1, 1).expand(D, H, W)], dim=3).view(1, 1, D, H, W, 3)

    def torch_f(zz=z, kk=kpc):
        gauss = torch.exp(-0.5 * ((grid - kk.view(N, K, 1, 1, 1, 3)) ** 2).sum(-1) / VAR)
        return torch.cat((zz, gauss.to(zz.dtype)), dim=1)

    zg, kg = z.clone().requires_grad_(True), kpc.clone().requires_grad_(True)
    G2 = G[:, :2 * K]

    def torch_fb():
        zg.grad = kg.grad = None
        torch_f(zg, kg).backward(G2)

    def new_fb():
        ops_efe.kpcat_forward(z, kpc)
        ops_efe.kpcat_backward(G, kpc, K)

    t = dict(new_f=[], torch_f=[], new_fb=[], torch_fb=[])
    for _ in range(rounds):
        t["torch_f"].append(window_time(torch_f, window / rounds))
        t["new_f"].append(window_time(new_f, window / rounds))
        t["torch_fb"].append(window_time(torch_fb, window / rounds))
        t["new_fb"].append(window_time(new_fb, window / rounds))
    zb, ob = z.numel() * 2, N * cp * D * H * W * 2
    res = dict(kpcat_fwd=vs_copy(window_time(new_f, window), zb + ob, window),
               kpcat_bwd=vs_copy(window_time(new_b, window), 2 * K * N * D * H * W * 2 + zb, window))
    res["kpcat_fwd"].update(torch_us=round(med(t["torch_f"]), 2), new_us_alternating=round(med(t["new_f"]), 2),
                            ratio_torch_over_new=round(med(t["torch_f"]) / med(t["new_f"]), 2))
    res["kpcat_fwd_bwd"] = dict(new_us=round(med(t["new_fb"]), 2), torch_us=round(med(t["torch_fb"]), 2),
                                ratio_torch_over_new=round(med(t["torch_fb"]) / med(t["new_fb"]), 2))
    return res


def bench_block(blk, x, window):
    xg = x.clone().requires_grad_(True)
    with torch.no_grad():
        gy = torch.randn_like(blk(x))

    def fwd():
        with torch.no_grad():
            blk(x)

    def step():
        for p in blk.parameters():
            p.grad = None
        xg.grad = None
        blk(xg).backward(gy)

    return fwd, step


def bench_mix(N, window, g, rounds=5):
    x = torch.randn((N, 32, 16, 64, 64), generator=g, device="cuda").to(BF16).contiguous(memory_format=CL3)
    x[:, 30:] = 0
    torch.manual_seed(1)
    mix = fv.ResBlock3D(30, False).cuda().train().set_compute_dtype(BF16)
    afe = fv.ResBlock3D(32, False).cuda().train().set_compute_dtype(BF16)
    same = fv.SameBlock3D(30, 15, False).cuda().train().set_compute_dtype(BF16)
    mf, ms = bench_block(mix, x, window)
    af, as_ = bench_block(afe, x, window)
    t = dict(mf=[], af=[], ms=[], as_=[])
    for _ in range(rounds):
        t["af"].append(window_time(af, window / rounds))
        t["mf"].append(window_time(mf, window / rounds))
        t["as_"].append(window_time(as_, window / rounds))
        t["ms"].append(window_time(ms, window / rounds))
    flops = 2 * 2.0 * N * 16 * 64 * 64 * 30 * 30 * 27
    res = dict(mix_block=dict(fwd_us=round(med(t["mf"]), 1), fwd_bwd_us=round(med(t["ms"]), 1),
                              afe_fwd_us=round(med(t["af"]), 1), afe_fwd_bwd_us=round(med(t["as_"]), 1),
                              ratio_fwd=round(med(t["mf"]) / med(t["af"]), 3),
                              ratio_fwd_bwd=round(med(t["ms"]) / med(t["as_"]), 3),
                              gflop_fwd_30ch=round(flops / 1e9, 3),
                              fwd_us_windows=[round(v, 1) for v in t["mf"]],
                              afe_fwd_us_windows=[round(v, 1) for v in t["af"]]))
    sf, ss = bench_block(same, x, window)
    res["mix_out"] = dict(fwd_us=round(window_time(sf, window), 1), fwd_bwd_us=round(window_time(ss, window), 1))
    return res


def bench_model(net, N, S, window):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(N, 3, S, S, generator=g, device="cuda")
    x_a = torch.rand(N, 3, S, S, generator=g, device="cuda")
    kpc = ((torch.rand(N, net.K, 3, generator=g, device="cuda") - 0.5) * 1.2).requires_grad_(True)
    eps = torch.randn(N, 16, 4, 4, generator=g, device="cuda")
    gk = torch.randn(N, net.K, 3, generator=g, device="cuda")
    kl = fv.KLDivergenceLoss()

    def step():
        for p in net.parameters():
            p.grad = None
        kpc.grad = None
        kp, _, _, ml, _ = net(x, x_a, kpc, True, eps)
        ((kp * gk).sum() + kl(ml)).backward()

    def fwd():
        with torch.no_grad():
            net(x, x_a, kpc, True, eps)

    torch.cuda.reset_peak_memory_stats()
    t_f = window_time(fwd, window, min_iters=2) / 1e3
    t_s = window_time(step, window, min_iters=2) / 1e3
    return dict(batch=N, resolution=S, parameters=sum(p.numel() for p in net.parameters()),
                forward_ms=round(t_f, 3), forward_backward_ms=round(t_s, 3),
                peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "efe", "efebench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("efebench needs a GPU")
    torch.manual_seed(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = dict(tool="efebench", device=torch.cuda.get_device_name(0), dtype="bf16", batch=a.batch, resolution=a.size,
               window_s=a.window)
    if not a.no_model:
        net = fv.EFE_conv5().cuda().train().set_compute_dtype(BF16)
        res["efe"] = bench_model(net, a.batch, a.size, a.window)
    fam = bench_kpcat((a.batch, 15, 16, 64, 64), max(a.window, 0.5), g)
    fam.update(bench_mix(a.batch, max(a.window, 0.5), g))
    res["families"] = fam
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
