"""Launch-family timing of the head pose estimator's new kernels (csrc/pose.hip) at the shapes of
the default HPE_EDE() on 256 x 256 images, N = 6 (source, driving and transformed driving at
B = 2), bf16, and the whole HPE_EDE forward + backward.

    python tools/hpebench.py [--batch 6] [--window 0.3] [--no-model] [--out profiles/hpe/hpebench.json]

Prints ONE JSON line, also written to --out (default profiles/hpe/hpebench.json).  Times are device
events over a warm-up and a timed window of at least --window seconds.

  stem_fwd      fv_stem7s2_fwd (with BN records) against the route the code had before: the
                stride-1 7x7 forward (fv_conv2d_fwd on the 8-channel padded NHWC image, its layout
                pass not counted) followed by a subsample, in alternating windows; old / new.
  stem_wgrad    fv_stem7s2_bwd_weight against its HBM roof (image + dy read, slabs written and read).
  pool_fwd / pool_bwd / subsample_* / join / pose_*   elementwise and reduction passes: the bytes
                each must move over its time, against a device-to-device copy moving the same
                bytes (half read, half written) timed in the same run; `vs_copy` = copy time /
                pass time (1 = as fast as the copy).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L  # noqa: E402
from facevae_amd import ops  # noqa: E402

CL = torch.channels_last
BF16 = torch.bfloat16
PEAK_HBM = 6.29e12


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


def rnd(shape, g, dtype=BF16):
    return torch.randn(shape, generator=g, device="cuda").to(dtype).contiguous(memory_format=CL)


class _Affine:
    def __init__(self, c, g):
        self.scale = torch.rand(c, generator=g, device="cuda") + 0.5
        self.shift = torch.randn(c, generator=g, device="cuda")


def bench_stem(N, S, cout, window, g, rounds=5):
    dc, st = L.FV_BF16, L.stream()
    x = torch.rand(N, 3, S, S, generator=g, device="cuda")
    w = (torch.randn(cout, 3, 7, 7, generator=g, device="cuda") / 147 ** 0.5).contiguous()
    bias = torch.zeros(cout, device="cuda")
    wk = torch.empty(L.query("fv_stem7s2_wk_elems", cout), dtype=BF16, device="cuda")
    L.call("fv_stem7s2_weight_prep", dc, w.data_ptr(), cout, wk.data_ptr(), st)
    nb = L.query("fv_stem7s2_stats_blocks", N, S, S)
    stats = torch.empty(nb * 2 * cout, device="cuda")
    y = torch.empty((N, cout, S // 2, S // 2), dtype=BF16, device="cuda", memory_format=CL)
    new = lambda: L.call("fv_stem7s2_fwd", dc, x.data_ptr(), N, S, S, cout, wk.data_ptr(), bias.data_ptr(),  # noqa: E731
                         y.data_ptr(), stats.data_ptr(), st)
    # the route the code had before: stride-1 7x7 conv on the padded NHWC image, then every second pixel
    xb, cp = ops.to_nhwc(x, BF16)
    conv = fv.ConvBlock2D("CNA", 3, cout, 7, 1, 3, False).cuda().conv
    d = ops.desc(BF16, N, S, S, cp, 3, cout, cout, 7)
    cs = ops.ConvState(conv, d, BF16, "cuda", True, need_wt=False)
    yfull = torch.empty((N, cout, S, S), dtype=BF16, device="cuda", memory_format=CL)

    def old():
        ops.conv_forward(cs, xb, conv.bias, y=yfull, stats=True)
        L.call("fv_subsample2_fwd", dc, yfull.data_ptr(), N, S, S, cout, y.data_ptr(), st)

    med = lambda v: sorted(v)[len(v) // 2]    # noqa: E731
    t_old, t_new = [], []
    for _ in range(rounds):
        t_old.append(window_time(old, window / rounds))
        t_new.append(window_time(new, window / rounds))
    P = N * (S // 2) * (S // 2)
    flops = 2.0 * P * cout * 147
    res = dict(stem_fwd=dict(new_us=round(med(t_new), 2), old_us=round(med(t_old), 2),
                             ratio_old_over_new=round(med(t_old) / med(t_new), 3),
                             new_us_windows=[round(v, 2) for v in t_new], old_us_windows=[round(v, 2) for v in t_old],
                             tflops=round(flops / (med(t_new) * 1e-6) / 1e12, 2),
                             mbytes=round((x.numel() * 4 + P * cout * 2) / 1e6, 3),
                             share_of_hbm_roof=round((x.numel() * 4 + P * cout * 2) / PEAK_HBM / (med(t_new) * 1e-6), 4)))
    dy = rnd((N, cout, S // 2, S // 2), g)
    nws = L.query("fv_stem7s2_wgrad_ws_bytes", N, S, S, cout)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    dw, db = torch.empty_like(w), torch.empty(cout, device="cuda")
    us = window_time(lambda: L.call("fv_stem7s2_bwd_weight", dc, x.data_ptr(), dy.data_ptr(), N, S, S, cout, dw.data_ptr(),
                                    db.data_ptr(), ws.data_ptr(), st), window)
    nbytes = x.numel() * 4 + P * cout * 2 + 2 * nws
    res["stem_wgrad"] = dict(us=round(us, 2), mbytes=round(nbytes / 1e6, 3), gflop=round(flops / 1e9, 3),
                             bound="hbm", share_of_roof=round(nbytes / PEAK_HBM / (us * 1e-6), 4))
    return res


def bench_passes(N, S, window, g):
    st, dc = L.stream(), L.FV_BF16
    res = {}
    # max pool with the BN / ReLU prologue: the stem output once, the quarter-size tensor + argmax out
    C, H = 64, S // 2
    y = rnd((N, C, H, H), g)
    r = _Affine(C, g)
    z = torch.empty((N, C, H // 2, H // 2), dtype=BF16, device="cuda", memory_format=CL)
    am = torch.empty(z.numel(), dtype=torch.uint8, device="cuda")
    us = window_time(lambda: L.call("fv_maxpool3s2_fwd", dc, y.data_ptr(), N, H, H, C, r.scale.data_ptr(),
                                    r.shift.data_ptr(), 0.0, z.data_ptr(), am.data_ptr(), st), window)
    res["pool_fwd_prologue"] = vs_copy(us, y.numel() * 2 + z.numel() * 3, window)
    gz = rnd(tuple(z.shape), g)
    dx = torch.empty_like(y)
    us = window_time(lambda: L.call("fv_maxpool3s2_bwd", dc, gz.data_ptr(), am.data_ptr(), N, H, H, C, dx.data_ptr(), st),
                     window)
    res["pool_bwd"] = vs_copy(us, z.numel() * 3 + dx.numel() * 2, window)
    # subsample in front of the first stride-2 projection: [N, 256, S/4, S/4] -> half the side
    C, H = 256, S // 4
    x = rnd((N, C, H, H), g)
    xs = torch.empty((N, C, H // 2, H // 2), dtype=BF16, device="cuda", memory_format=CL)
    us = window_time(lambda: L.call("fv_subsample2_fwd", dc, x.data_ptr(), N, H, H, C, xs.data_ptr(), st), window)
    res["subsample_fwd"] = vs_copy(us, xs.numel() * 4, window)
    dxx = torch.empty_like(x)
    us = window_time(lambda: L.call("fv_subsample2_bwd", dc, xs.data_ptr(), N, H, H, C, dxx.data_ptr(), st), window)
    res["subsample_bwd"] = vs_copy(us, xs.numel() * 2 + dxx.numel() * 2, window)
    # the join of the largest bottlenecks: [N, 256, S/4, S/4], both affines
    ya, yb = rnd((N, C, H, H), g), rnd((N, C, H, H), g)
    ra, rb = _Affine(C, g), _Affine(C, g)
    out = torch.empty_like(ya)
    us = window_time(lambda: L.call("fv_bn2_add_relu_fwd", dc, ya.data_ptr(), ra.scale.data_ptr(), ra.shift.data_ptr(),
                                    yb.data_ptr(), rb.scale.data_ptr(), rb.shift.data_ptr(), N * H * H, C,
                                    out.data_ptr(), st), window)
    res["join"] = vs_copy(us, ya.numel() * 6, window)
    us = window_time(lambda: L.call("fv_add2", dc, ya.data_ptr(), yb.data_ptr(), ya.numel(), out.data_ptr(), st), window)
    res["add2"] = vs_copy(us, ya.numel() * 6, window)
    # pose head: [N, 2048, S/32, S/32], n_bins 66
    C, H, nbins = 2048, S // 32, 66
    h = rnd((N, C, H, H), g)
    feat = torch.empty((N, C), device="cuda")
    us = window_time(lambda: L.call("fv_pose_pool_fwd", dc, h.data_ptr(), N, H * H, C, feat.data_ptr(), st), window)
    res["pose_pool"] = vs_copy(us, h.numel() * 2 + feat.numel() * 4, window)
    rows = (nbins, nbins, nbins, 3, 1)
    ws_ = [torch.randn(rr, C, generator=g, device="cuda") / C ** 0.5 for rr in rows]
    bs_ = [torch.zeros(rr, device="cuda") for rr in rows]
    p5 = lambda ts: (ctypes.c_void_p * 5)(*[t.data_ptr() for t in ts])    # noqa: E731
    outp = torch.empty((N, 7), device="cuda")
    prob = torch.empty((N, 3, nbins), device="cuda")
    wp, bp = p5(ws_), p5(bs_)
    us = window_time(lambda: L.call("fv_pose_head_fwd", feat.data_ptr(), N, C, nbins, wp, bp, outp.data_ptr(),
                                    prob.data_ptr(), st), window)
    wbytes = sum(t.numel() for t in ws_) * 4
    res["pose_head_fwd"] = vs_copy(us, wbytes + feat.numel() * 4, window)
    dws, dbs = [torch.empty_like(t) for t in ws_], [torch.empty_like(t) for t in bs_]
    dwp, dbp = p5(dws), p5(dbs)
    gout = torch.randn(N, 7, generator=g, device="cuda")
    dh = torch.empty_like(h)
    wsb = torch.empty(L.query("fv_pose_head_ws_bytes", N, C, nbins), dtype=torch.uint8, device="cuda")
    us = window_time(lambda: L.call("fv_pose_head_bwd", dc, gout.data_ptr(), feat.data_ptr(), prob.data_ptr(), N, H * H, C,
                                    nbins, wp, dwp, dbp, dh.data_ptr(), wsb.data_ptr(), st), window)
    res["pose_head_bwd"] = vs_copy(us, 3 * wbytes + dh.numel() * 2, window)
    return res


def bench_model(N, S, window):
    torch.manual_seed(0)
    net = fv.HPE_EDE().cuda().train().set_compute_dtype(BF16)
    x = torch.rand(N, 3, S, S, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")

    def step():
        for p in net.parameters():
            p.grad = None
        yaw, pitch, roll, t, scale = net(x)
        (yaw.sum() + pitch.sum() + roll.sum() + t.sum() + scale.sum()).backward()

    def fwd():
        with torch.no_grad():
            net(x)

    t_f = window_time(fwd, window, min_iters=2) / 1e3
    t_s = window_time(step, window, min_iters=2) / 1e3
    return dict(batch=N, resolution=S, parameters=sum(p.numel() for p in net.parameters()),
                forward_ms=round(t_f, 3), forward_backward_ms=round(t_s, 3),
                peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpe", "hpebench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hpebench needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(0)
    fam = bench_stem(a.batch, a.size, 64, max(a.window, 0.5), g)
    fam.update(bench_passes(a.batch, a.size, a.window, g))
    res = dict(tool="hpebench", device=torch.cuda.get_device_name(0), dtype="bf16", batch=a.batch, resolution=a.size,
               window_s=a.window, peaks=dict(hbm_bytes_per_s=PEAK_HBM), families=fam)
    if not a.no_model:
        res["hpe"] = bench_model(a.batch, a.size, a.window)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
