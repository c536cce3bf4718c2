"""Timing of the equivariance transform's kernels (csrc/tps.hip) against a device copy and against
the torch composition they replace, run on the same GPU.

    python tools/tpsbench.py [--window 0.3] [--out profiles/tps/tpsbench.json]

Prints ONE JSON line, also written to --out.  Times are device events over a warm-up and timed
windows; the kernel and the torch composition alternate over --rounds windows (the medians are
reported, every window listed), each family timed for at least --window seconds in all.

  frame_b32, frame_b2    fv_tps_warp_frame_fwd on [32, 3, 256, 256] and [2, 3, 256, 256] fp32 frames,
                         default sigmas.  `vs_copy` = the time of a device-to-device copy moving the same
                         bytes (one read and one write of the frame) / the kernel's time.  The torch
                         composition is the reference's formulation restated on the GPU: the broadcast
                         [B, H*W, P*P, 2] differences, abs-sum, square, log, two products, the sum and
                         F.grid_sample(align_corners=True, padding_mode="reflection") on the [B, H, W, 2]
                         grid.  `rel_l2_vs_torch` compares the two results on the timed inputs.
  coords_fwd_bwd         WarpCoordsFn forward + backward on [32, 15, 2] points against the same
                         composition under torch autograd.
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
from facevae_amd import ops_tps  # noqa: E402
from facevae_amd.warp import make_coordinate_grid_2d  # noqa: E402

PEAK_HBM = 6.29e12
PTS = 5


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


def med(v):
    return sorted(v)[len(v) // 2]


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def torch_warp_coordinates(coords, theta, cparams, cpoints):
    """The reference's warp_coordinates in torch ops on the device of its arguments."""
    th = theta.unsqueeze(1)
    out = (torch.matmul(th[:, :, :, :2], coords.unsqueeze(-1)) + th[:, :, :, 2:]).squeeze(-1)
    d = (coords.view(coords.shape[0], -1, 1, 2) - cpoints.view(1, 1, -1, 2)).abs().sum(-1)
    r = d ** 2
    r = r * torch.log(d + 1e-6)
    r = r * cparams
    return out + r.sum(dim=2).view(theta.shape[0], coords.shape[1], 1)


def alternate(new, old, window, rounds):
    t = dict(new=[], old=[])
    for _ in range(rounds):
        t["old"].append(window_time(old, window / rounds))
        t["new"].append(window_time(new, window / rounds))
    return t


def bench_frame(B, S, window, rounds):
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.rand(B, 3, S, S, generator=g, device="cuda")
    torch.manual_seed(B)
    t = fv.Transform(B)
    theta, cparams, cpoints = t.theta.cuda(), t.control_params.cuda(), t.control_points.cuda()

    def new():
        return ops_tps.warp_frame(x, theta, cparams, PTS)

    def old():
        grid = make_coordinate_grid_2d((S, S), device="cuda").view(1, S * S, 2)
        grid = torch_warp_coordinates(grid, theta, cparams, cpoints).view(B, S, S, 2)
        return F.grid_sample(x, grid, align_corners=True, padding_mode="reflection")

    err = rel_l2(new(), old())
    nbytes = 2 * x.numel() * 4
    src, dst = torch.empty_like(x), torch.empty_like(x)
    tw = alternate(new, old, window, rounds)
    tc = alternate(new, lambda: dst.copy_(src), window, rounds)
    us, tus, cus = med(tw["new"]), med(tw["old"]), med(tc["old"])
    return dict(shape=[B, 3, S, S], us=round(us, 2), mbytes=round(nbytes / 1e6, 3),
                tb_per_s=round(nbytes / (us * 1e-6) / 1e12, 3), copy_us=round(cus, 2),
                us_beside_copy=round(med(tc["new"]), 2), vs_copy=round(cus / med(tc["new"]), 3),
                logs_per_s=round(B * S * S * PTS * PTS / (us * 1e-6), 0),
                torch_us=round(tus, 2), ratio_torch_over_new=round(tus / us, 2), rel_l2_vs_torch=err,
                new_us_windows=[round(v, 2) for v in tw["new"]], torch_us_windows=[round(v, 2) for v in tw["old"]],
                copy_us_windows=[round(v, 2) for v in tc["old"]])


def bench_coords(B, M, window, rounds):
    g = torch.Generator(device="cuda").manual_seed(3)
    c = ((torch.rand(B, M, 2, generator=g, device="cuda") - 0.5) * 2).requires_grad_(True)
    G = torch.randn(B, M, 2, generator=g, device="cuda")
    torch.manual_seed(3)
    t = fv.Transform(B)
    theta, cparams, cpoints = t.theta.cuda(), t.control_params.cuda(), t.control_points.cuda()

    def new():
        c.grad = None
        ops_tps.WarpCoordsFn.apply(c, theta, cparams, PTS).backward(G)
        return c.grad

    def old():
        c.grad = None
        torch_warp_coordinates(c, theta, cparams, cpoints).backward(G)
        return c.grad

    err = rel_l2(new().clone(), old().clone())
    tw = alternate(new, old, window, rounds)
    us, tus = med(tw["new"]), med(tw["old"])
    return dict(shape=[B, M, 2], us=round(us, 2), torch_us=round(tus, 2), ratio_torch_over_new=round(tus / us, 2),
                rel_l2_grad_vs_torch=err, new_us_windows=[round(v, 2) for v in tw["new"]],
                torch_us_windows=[round(v, 2) for v in tw["old"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tps", "tpsbench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tpsbench needs a GPU")
    w = max(a.window, 0.3)
    res = dict(tool="tpsbench", device=torch.cuda.get_device_name(0), dtype="fp32", points_tps=PTS, window_s=w,
               rounds=a.rounds, peaks=dict(hbm_bytes_per_s=PEAK_HBM))
    fam = dict(frame_b32=bench_frame(32, a.size, w, a.rounds), frame_b2=bench_frame(2, a.size, w, a.rounds),
               coords_fwd_bwd=bench_coords(32, 15, w, a.rounds))
    e = torch.empty(64, device="cuda")
    fam["one_small_launch_us"] = round(window_time(lambda: e.add_(1), w), 2)
    res["families"] = fam
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
