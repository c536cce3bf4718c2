"""Launch-family timing of the patch discriminator at its default shapes (256x256, B=32, bf16,
K=15 keypoints), and the adversarial iteration next to the plain step.

    python tools/discbench.py [--batch 32] [--res 256] [--window 0.5] [--no-step] [--out FILE]

Prints ONE JSON line (also written to --out).  Per launch family: time per launch by device
events (warm-up, then a timed window of at least --window seconds), the algorithmic FLOPs and
bytes computed from the shapes below, and the share of the bounding roof -- the larger of
FLOPs / MFMA peak and bytes / HBM rate, over the measured time.  Peaks (MI355X_MICROARCH.md):
bf16 MFMA 2.5e15 FLOP/s dense, HBM 6.29e12 B/s measured streaming rate (8.0e12 spec).

"s2_vs_s1": for each stride-2 layer, the new forward against the only route of the parent tree,
fv_conv2d_fwd at stride 1 over the same input and weights (4x the outputs) followed by the
subsample, timed in alternating windows inside this one process; the ratio old / new and the
run-to-run spread (max - min over the median of the windows) of both.
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
PEAK_MFMA_BF16 = 2.5e15
PEAK_HBM = 6.29e12


def window_time(fn, window_s, min_iters=5):
    """us per call over a timed window of at least window_s seconds (after a warm-up)."""
    s = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(min_iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    per = max(e0.elapsed_time(e1) / min_iters * 1e-3, 1e-6)          # seconds per call
    iters = max(min_iters, int(window_s / per) + 1)
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def roof(us, flops, nbytes):
    t_f, t_b = flops / PEAK_MFMA_BF16, nbytes / PEAK_HBM
    bound = "mfma" if t_f >= t_b else "hbm"
    return dict(us=round(us, 2), gflop=round(flops / 1e9, 3), mbytes=round(nbytes / 1e6, 3), bound=bound,
                share_of_roof=round(max(t_f, t_b) / (us * 1e-6), 4))


def conv_shapes(B, H, K):
    """name, stride, cin_valid, cout, output side -- Discriminator() (models.py:1117-1128)"""
    return [("l0_s2", 2, 3 + K, 64, H // 2), ("l1_s2", 2, 64, 128, H // 4), ("l2_s2", 2, 128, 256, H // 8),
            ("l3_s1", 1, 256, 512, H // 8), ("l4_s1", 1, 512, 1, H // 8)]


def bench_conv(name, stride, cin, cout, Ho, B, window, g):
    dev = "cuda"
    Hi = Ho * stride
    cp = ops.pad_pow2(cin)
    x = torch.randn(B, cp, Hi, Hi, generator=g, device=dev).to(BF16).contiguous(memory_format=CL)
    w = (torch.randn(cout, cin, 3, 3, generator=g, device=dev) / (9 * cin) ** 0.5).contiguous()
    bias = torch.zeros(cout, device=dev)
    ldd = ops.pad_pow2(cout)
    nchw = cout % 8 != 0
    d = ops.desc(BF16, B, Ho, Ho, cp, cin, cout, cout, 3, nchw=nchw)
    dy = torch.randn(B, ldd, Ho, Ho, generator=g, device=dev).to(BF16).contiguous(memory_format=CL)
    if nchw:
        dy[:, cout:] = 0
    y = torch.empty((B, cout, Ho, Ho), dtype=torch.float32 if nchw else BF16, device=dev,
                    memory_format=torch.contiguous_format if nchw else CL)
    dx = torch.empty((B, cp, Hi, Hi), dtype=BF16, device=dev, memory_format=CL)
    dw, db = torch.empty_like(w), torch.empty(cout, device=dev)
    st = L.stream()
    pfx = "fv_conv2d_s2_" if stride == 2 else "fv_conv2d_"
    q = (lambda n: L.query(pfx + n, ctypes.byref(d)))
    if stride == 2:
        wk, wt = torch.empty(q("wk_elems"), dtype=BF16, device=dev), torch.empty(q("wt_elems"), dtype=BF16, device=dev)
        L.call("fv_conv2d_s2_weight_prep", ctypes.byref(d), w.data_ptr(), None, wk.data_ptr(), wt.data_ptr(), st)
        fwd = lambda: L.call("fv_conv2d_s2_fwd", ctypes.byref(d), Hi, Hi, x.data_ptr(), wk.data_ptr(), bias.data_ptr(),
                             y.data_ptr(), st)
        dgrad = lambda: L.call("fv_conv2d_s2_bwd_data", ctypes.byref(d), Hi, Hi, dy.data_ptr(), ldd, wt.data_ptr(),
                               dx.data_ptr(), st)
    else:
        wk = torch.empty(L.query("fv_conv_wk_elems", ctypes.byref(d)), dtype=BF16, device=dev)
        wt = torch.empty(L.query("fv_conv_wt_elems", ctypes.byref(d)), dtype=BF16, device=dev)
        L.call("fv_conv_weight_prep", ctypes.byref(d), w.data_ptr(), None, wk.data_ptr(), wt.data_ptr(), st)
        fwd = lambda: L.call("fv_conv2d_fwd", ctypes.byref(d), x.data_ptr(), wk.data_ptr(), bias.data_ptr(), None, None,
                             None, y.data_ptr(), None, st)
        dgrad = lambda: L.call("fv_conv2d_bwd_data", ctypes.byref(d), dy.data_ptr(), ldd, wt.data_ptr(), dx.data_ptr(), st)
    slab = torch.empty(q("wgrad_slab_elems"), device=dev)
    bslab = torch.empty(q("wgrad_bias_slab_elems"), device=dev)

    def wgrad():
        if stride == 2:
            L.call("fv_conv2d_s2_bwd_weight", ctypes.byref(d), Hi, Hi, x.data_ptr(), dy.data_ptr(), ldd, slab.data_ptr(),
                   bslab.data_ptr(), st)
            L.call("fv_conv2d_s2_wgrad_reduce", ctypes.byref(d), slab.data_ptr(), bslab.data_ptr(), dw.data_ptr(),
                   db.data_ptr(), st)
        else:
            L.call("fv_conv2d_bwd_weight", ctypes.byref(d), x.data_ptr(), None, None, dy.data_ptr(), ldd, slab.data_ptr(),
                   bslab.data_ptr(), st)
            L.call("fv_conv2d_wgrad_reduce", ctypes.byref(d), slab.data_ptr(), bslab.data_ptr(), dw.data_ptr(),
                   db.data_ptr(), st)

    flops = 2.0 * B * Ho * Ho * cout * cin * 9
    bx, by, bw = B * Hi * Hi * cp * 2, B * Ho * Ho * (cout * 4 if nchw else cout * 2), cout * cin * 9 * 2
    bdy = B * Ho * Ho * ldd * 2
    out = {name + "_fwd": roof(window_time(fwd, window), flops, bx + by + bw),
           name + "_dgrad": roof(window_time(dgrad, window), flops, bdy + bx + bw),
           name + "_wgrad": roof(window_time(wgrad, window), flops, bx + bdy + cout * cin * 9 * 4)}
    cmp_ = None
    if stride == 2:
        # the parent tree's only route: the stride-1 conv over the same input, then the subsample
        d1 = ops.desc(BF16, B, Hi, Hi, cp, cin, cout, cout, 3)
        wk1 = torch.empty(L.query("fv_conv_wk_elems", ctypes.byref(d1)), dtype=BF16, device=dev)
        L.call("fv_conv_weight_prep", ctypes.byref(d1), w.data_ptr(), None, wk1.data_ptr(), None, st)
        y1 = torch.empty((B, cout, Hi, Hi), dtype=BF16, device=dev, memory_format=CL)
        ysub = torch.empty((B, cout, Ho, Ho), dtype=BF16, device=dev, memory_format=CL)

        def old():
            L.call("fv_conv2d_fwd", ctypes.byref(d1), x.data_ptr(), wk1.data_ptr(), bias.data_ptr(), None, None, None,
                   y1.data_ptr(), None, st)
            ysub.copy_(y1[:, :, ::2, ::2])

        old()
        fwd()
        torch.cuda.synchronize()
        same = bool(torch.equal(ysub, y)) if not nchw else None
        maxdiff = float((ysub.float() - y.float()).abs().max())
        rounds = 6
        t_new, t_old = [], []
        for _ in range(rounds):
            t_old.append(window_time(old, window / rounds))
            t_new.append(window_time(fwd, window / rounds))
        med = lambda v: sorted(v)[len(v) // 2]
        spread = lambda v: (max(v) - min(v)) / med(v)
        cmp_ = dict(new_us=round(med(t_new), 2), old_us=round(med(t_old), 2), ratio_old_over_new=round(med(t_old) / med(t_new), 3),
                    spread_new=round(spread(t_new), 4), spread_old=round(spread(t_old), 4),
                    new_us_windows=[round(v, 2) for v in t_new], old_us_windows=[round(v, 2) for v in t_old],
                    outputs_equal=same, outputs_max_abs_diff=maxdiff)
    return out, cmp_


def bench_instance_norm(B, C, Hs, window, g):
    dev = "cuda"
    x = torch.randn(B, C, Hs, Hs, generator=g, device=dev).to(BF16).contiguous(memory_format=CL)
    dz = torch.randn(B, C, Hs, Hs, generator=g, device=dev).to(BF16).contiguous(memory_format=CL)
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.zeros(C, device=dev)
    z, dxo = torch.empty_like(x), torch.empty_like(x)
    mean, invstd = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
    dg, dbt, k = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty(B, 2, C, device=dev)
    ws = torch.empty(L.query("fv_in_ws_bytes", B, Hs, Hs, C) // 8, dtype=torch.float64, device=dev)
    st = L.stream()
    a = (B, Hs, Hs, C)
    stats = lambda: L.call("fv_in_stats", L.FV_BF16, x.data_ptr(), *a, 1e-5, mean.data_ptr(), invstd.data_ptr(),
                           ws.data_ptr(), st)
    fwd = lambda: L.call("fv_in_act_fwd", L.FV_BF16, x.data_ptr(), *a, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                         beta.data_ptr(), 0.2, z.data_ptr(), st)
    red = lambda: L.call("fv_in_act_bwd_reduce", L.FV_BF16, dz.data_ptr(), x.data_ptr(), *a, mean.data_ptr(),
                         invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 0.2, dg.data_ptr(), dbt.data_ptr(),
                         k.data_ptr(), ws.data_ptr(), st)
    app = lambda: L.call("fv_in_act_bwd_apply", L.FV_BF16, dz.data_ptr(), x.data_ptr(), *a, mean.data_ptr(),
                         invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 0.2, k.data_ptr(), dxo.data_ptr(), st)
    stats()
    n = B * C * Hs * Hs
    tag = f"in_c{C}_h{Hs}_"
    # elementwise counts per element: stats 3 (sum, square, sum), fwd 5, bwd_reduce 9, bwd_apply 12
    return {tag + "stats": roof(window_time(stats, window), 3.0 * n, 2 * n),
            tag + "fwd": roof(window_time(fwd, window), 5.0 * n, 4 * n),
            tag + "bwd_reduce": roof(window_time(red, window), 9.0 * n, 4 * n),
            tag + "bwd_apply": roof(window_time(app, window), 12.0 * n, 6 * n)}


def bench_input(B, H, K, window, g):
    dev = "cuda"
    x = torch.rand(B, 3, H, H, generator=g, device=dev)
    kp = torch.rand(B, K, 3, generator=g, device=dev) * 2 - 1
    cp = ops.pad_pow2(3 + K)
    out = torch.empty((B, cp, H, H), dtype=BF16, device=dev, memory_format=CL)
    f = lambda: L.call("fv_disc_input_fwd", L.FV_BF16, x.data_ptr(), kp.data_ptr(), B, H, H, K, 3, cp, out.data_ptr(),
                       L.stream())
    P = B * H * H
    # per pixel and keypoint: 2 subtractions, 2 squares, an add, a scale and an exponential
    return {"input_assembly": roof(window_time(f, window), 7.0 * P * K, P * 3 * 4 + P * cp * 2)}


def bench_steps(B, H, window):
    res = {}
    for name, wG, wF in (("plain_step_ms", 0.0, 0.0), ("adversarial_iteration_ms", 1.0, 10.0)):
        cfg = fv.FaceVAEConfig(H=H, w_G=wG, w_F=wF)
        tr = fv.FaceVAETrainer(None, None, None, lr=cfg.lr, cfg=cfg, compute_dtype=BF16, seed=0)
        x = torch.rand(B, 3, H, H, device="cuda")
        eps = tr.sample_eps(x)
        res[name] = round(window_time(lambda: tr.train_step(x, eps), window, min_iters=3) / 1e3, 3)
        del tr
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("discbench needs a GPU")
    B, H, K = a.batch, a.res, a.K
    g = torch.Generator(device="cuda").manual_seed(0)
    fam, cmp_ = {}, {}
    for name, stride, cin, cout, Ho in conv_shapes(B, H, K):
        f, c = bench_conv(name, stride, cin, cout, Ho, B, a.window, g)
        fam.update(f)
        if c is not None:
            cmp_[name] = c
    for C, Hs in ((64, H // 2), (128, H // 4), (256, H // 8), (512, H // 8)):
        fam.update(bench_instance_norm(B, C, Hs, a.window, g))
    fam.update(bench_input(B, H, K, a.window, g))
    res = dict(tool="discbench", device=torch.cuda.get_device_name(0), dtype="bf16", batch=B, res=H, K=K,
               window_s=a.window, peaks=dict(mfma_bf16_flops=PEAK_MFMA_BF16, hbm_bytes_per_s=PEAK_HBM),
               families=fam, s2_vs_s1=cmp_)
    if not a.no_step:
        res["steps"] = bench_steps(B, H, a.window)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
