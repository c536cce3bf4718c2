"""Launch-family timing of the canonical keypoint detector: the default CKD() on 256 x 256 images,
N = 2, bf16 -- the whole forward and forward + backward, every level on its own, and the new kernels
of csrc/ckd.hip against a device copy and against the torch ops they replace.

    python tools/ckdbench.py [--batch 2] [--window 0.3] [--no-model] [--out profiles/ckd/ckdbench.json]

Prints ONE JSON line, also written to --out (default profiles/ckd/ckdbench.json).  Times are device
events over a warm-up and a timed window of at least --window seconds.

  resize                 fv_ckd_resize_fwd: image read, NHWC conv input written; `vs_copy` = the time of
                         a device-to-device copy moving the same bytes / the pass time.
  down.0-4, mid_conv,    each level's module forward and forward + backward on its own (all its
  up.0-4, out_conv       launches: weight prep, conv, BN statistics and apply, their backward), with the
                         convolution's algorithmic FLOPs (2 x voxels x cin x cout x taps; x 3 with
                         both gradients, x 2 for down.0 whose input is data).
  softargmax_fwd / _bwd  the two forward launches and the backward pass against the copy, and in
                         alternating windows against the torch composition they replace (softmax over
                         the voxels, broadcast product with the grid, sum; autograd for the backward)
                         on the same tensor.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L  # noqa: E402
from facevae_amd import ops_ckd  # noqa: E402

CL, CL3 = torch.channels_last, torch.channels_last_3d
BF16 = torch.bfloat16
PEAK_HBM = 6.29e12
T = 0.1


def window_time(fn, window_s, min_iters=3):
    """us per call over a timed window of at least window_s seconds (after a warm-up)."""
    s = torch.cuda.current_stream()
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(min_iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    per = max(e0.elapsed_time(e1) / min_iters * 1e-3, 1e-6)
    iters = max(min_iters, int(window_s / per) + 1)
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def copy_time(nbytes, window):
    """us of a device-to-device copy that moves nbytes in all (nbytes / 2 read, nbytes / 2 written)."""
    n = max(int(nbytes) // 2, 1)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    return window_time(lambda: dst.copy_(src), window)


def vs_copy(us, nbytes, window):
    c = copy_time(nbytes, window)
    return dict(us=round(us, 2), mbytes=round(nbytes / 1e6, 3), tb_per_s=round(nbytes / (us * 1e-6) / 1e12, 3),
                copy_us=round(c, 2), vs_copy=round(c / us, 3))


def med(v):
    return sorted(v)[len(v) // 2]


def bench_level(name, mod, x, flops_fwd, need_dx, window):
    """A level's module on its own input: forward (no_grad) and forward + backward."""
    xg = x.clone().requires_grad_(need_dx)
    with torch.no_grad():
        gy = torch.randn_like(mod(x))

    def fwd():
        with torch.no_grad():
            mod(x)

    def step():
        for p in mod.parameters():
            p.grad = None
        xg.grad = None
        mod(xg).backward(gy)

    tf, ts = window_time(fwd, window), window_time(step, window)
    total = flops_fwd * (3 if need_dx else 2)
    return dict(fwd_us=round(tf, 1), fwd_bwd_us=round(ts, 1), gflop_fwd=round(flops_fwd / 1e9, 3),
                tflops_fwd=round(flops_fwd / (tf * 1e-6) / 1e12, 2), tflops_fwd_bwd=round(total / (ts * 1e-6) / 1e12, 2),
                out_shape=list(gy.shape))


def bench_levels(net, N, S, window, g):
    res = {}
    x = torch.rand(N, 3, S, S, generator=g, device="cuda")
    Ho = ops_ckd.resized(S, net.scale_factor)
    y = torch.empty((N, 8, Ho, Ho), dtype=BF16, device="cuda", memory_format=CL)
    us = window_time(lambda: L.call("fv_ckd_resize_fwd", L.FV_BF16, x.data_ptr(), N, S, S, Ho, Ho, y.data_ptr(), L.stream()),
                     window)
    res["resize"] = vs_copy(us, x.numel() * 4 + y.numel() * 2, window)
    us = window_time(lambda: F.interpolate(x, mode="bilinear", scale_factor=net.scale_factor, align_corners=False,
                                           recompute_scale_factor=True), window)
    res["resize"]["torch_interpolate_us"] = round(us, 2)
    h = y
    for i, blk in enumerate(net.down):
        conv = blk.layers[0].conv
        n_, _, hh, ww = h.shape
        res[f"down.{i}"] = bench_level(f"down.{i}", blk, h, 2.0 * n_ * hh * ww * conv.in_channels * conv.out_channels * 9,
                                       i > 0, window)
        with torch.no_grad():
            h = blk(h)
    n_, c_, hh, ww = h.shape
    res["mid_conv"] = bench_level("mid_conv", net.mid_conv, h, 2.0 * n_ * hh * ww * c_ * net.mid_conv.out_channels, True, window)
    with torch.no_grad():
        v = fv.ops3d.depth_split(net.mid_conv(h), net.C, net.D, BF16)
    for i, blk in enumerate(net.up):
        conv = blk.layers[1].conv
        n_, _, dd, hh, ww = v.shape
        res[f"up.{i}"] = bench_level(f"up.{i}", blk, v, 2.0 * n_ * dd * 4 * hh * ww * conv.in_channels * conv.out_channels * 27,
                                     True, window)
        with torch.no_grad():
            v = blk(v)
    n_, c_, dd, hh, ww = v.shape
    res["out_conv"] = bench_level("out_conv", net.out_conv, v, 2.0 * n_ * dd * hh * ww * c_ * net.out_conv.out_channels * 27,
                                  True, window)
    return res, (n_, net.out_conv.out_channels, dd, hh, ww)


def bench_softargmax(shape, window, g, rounds=5):
    N, K, D, H, W = shape
    z = torch.randn(shape, generator=g, device="cuda").to(BF16).contiguous(memory_format=CL3)
    G = torch.randn(N, K, 3, generator=g, device="cuda")
    kp, stat = ops_ckd.softargmax_forward(z, T)
    new_f = lambda: ops_ckd.softargmax_forward(z, T)                     # noqa: E731
    new_b = lambda: ops_ckd.softargmax_backward(z, G, stat, T)           # noqa: E731
    lin = lambda n: 2 * (torch.arange(n, device="cuda", dtype=torch.float32) / (n - 1)) - 1   # noqa: E731
    grid = torch.stack([lin(W).view(1, 1, W).expand(D, H, W), lin(H).view(1, H, 1).expand(D, H, W),
                        lin(D).view(D, 1, 1).expand(D, H, W)], dim=3)

    def torch_f(zz=z):
        heat = F.softmax(zz.float().reshape(N, K, -1) / T, dim=2).view(N, K, D, H, W)
        return (heat.unsqueeze(-1) * grid).sum(dim=(2, 3, 4))

    zg = z.clone().requires_grad_(True)

    def torch_fb():
        zg.grad = None
        (torch_f(zg) * G).sum().backward()

    def new_fb():
        ops_ckd.softargmax_backward(z, G, ops_ckd.softargmax_forward(z, T)[1], T)

    t = dict(new_f=[], torch_f=[], new_fb=[], torch_fb=[])
    for _ in range(rounds):
        t["torch_f"].append(window_time(torch_f, window / rounds))
        t["new_f"].append(window_time(new_f, window / rounds))
        t["torch_fb"].append(window_time(torch_fb, window / rounds))
        t["new_fb"].append(window_time(new_fb, window / rounds))
    zb = z.numel() * 2
    res = dict(softargmax_fwd=vs_copy(window_time(new_f, window), zb, window),
               softargmax_bwd=vs_copy(window_time(new_b, window), 2 * zb, window))
    res["softargmax_fwd"].update(torch_us=round(med(t["torch_f"]), 2), new_us_alternating=round(med(t["new_f"]), 2),
                                 ratio_torch_over_new=round(med(t["torch_f"]) / med(t["new_f"]), 2),
                                 new_us_windows=[round(v, 2) for v in t["new_f"]],
                                 torch_us_windows=[round(v, 2) for v in t["torch_f"]])
    res["softargmax_fwd_bwd"] = dict(new_us=round(med(t["new_fb"]), 2), torch_us=round(med(t["torch_fb"]), 2),
                                     ratio_torch_over_new=round(med(t["torch_fb"]) / med(t["new_fb"]), 2),
                                     new_us_windows=[round(v, 2) for v in t["new_fb"]],
                                     torch_us_windows=[round(v, 2) for v in t["torch_fb"]])
    # an empty launch pair on the same stream: the floor two dependent launches cannot go below
    e = torch.empty(64, device="cuda")
    res["two_small_launches_us"] = round(window_time(lambda: (e.add_(1), e.add_(1)), window), 2)
    return res


def bench_model(net, N, S, window):
    x = torch.rand(N, 3, S, S, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")
    g = torch.randn(N, net.out_conv.out_channels, 3, device="cuda")

    def step():
        for p in net.parameters():
            p.grad = None
        (net(x) * g).sum().backward()

    def fwd():
        with torch.no_grad():
            net(x)

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ckd", "ckdbench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ckdbench needs a GPU")
    torch.manual_seed(0)
    net = fv.CKD().cuda().train().set_compute_dtype(BF16)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = dict(tool="ckdbench", device=torch.cuda.get_device_name(0), dtype="bf16", batch=a.batch, resolution=a.size,
               window_s=a.window, peaks=dict(hbm_bytes_per_s=PEAK_HBM))
    if not a.no_model:
        res["ckd"] = bench_model(net, a.batch, a.size, a.window)
    fam, zshape = bench_levels(net, a.batch, a.size, a.window, g)
    fam.update(bench_softargmax(zshape, max(a.window, 0.5), g))
    res["families"] = fam
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
