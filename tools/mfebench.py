"""Launch-family timing of the motion field estimator's 3-D convs at the default MFE() shapes
(fs [N, 32, 16, 64, 64], bf16, K = 15), the whole MFE forward + backward, and the general
implicit-GEMM kernels against the direct 3-D kernels where both run.

    python tools/mfebench.py [--batch 2] [--window 0.3] [--no-model] [--out profiles/mfe/mfebench.json]

Prints ONE JSON line (also written to --out).  Per launch family: time per launch by device
events (warm-up, then a timed window of at least --window seconds), the algorithmic FLOPs and
bytes from the shapes, and the share of the bounding roof -- the larger of FLOPs / MFMA peak and
bytes / HBM rate, over the measured time.  Peaks (MI355X_MICROARCH.md): bf16 MFMA 2.5e15 FLOP/s
dense, HBM 6.29e12 B/s measured streaming rate.

"gemm_vs_direct": 64 -> 32 channels at [2, ., 16, 64, 64], bf16: the new kernels against the route
that shape had before (fv_conv3d_fwd / _bwd_data / _bwd_weight: the one-output-per-thread direct
kernels), timed in alternating windows inside this one process; old / new and the run-to-run
spread (max - min over the median of the windows) of both.
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
from facevae_amd import ops3d  # noqa: E402

CL3 = torch.channels_last_3d
BF16 = torch.bfloat16
PEAK_MFMA_BF16 = 2.5e15
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


def roof(us, flops, nbytes):
    t_f, t_b = flops / PEAK_MFMA_BF16, nbytes / PEAK_HBM
    return dict(us=round(us, 2), gflop=round(flops / 1e9, 3), mbytes=round(nbytes / 1e6, 3),
                bound="mfma" if t_f >= t_b else "hbm", share_of_roof=round(max(t_f, t_b) / (us * 1e-6), 4),
                tflops=round(flops / (us * 1e-6) / 1e12, 2))


def mfe_convs(D=16, S=64):
    """name, cin, cout, output side, ksize, upsample -- MFE() (models.py:1052-1058)"""
    down, up = [80, 64, 128, 256, 512, 1024], [1024, 512, 256, 128, 64, 32]
    out = [("compress", 32, 4, S, 1, False)]
    out += [(f"down{i}", down[i], down[i + 1], S >> i, 3, False) for i in range(5)]
    out += [(f"up{i}", up[i], up[i + 1], (S >> 5) << (i + 1), 3, True) for i in range(5)]
    out.append(("mask_conv", 112, 16, S, 7, False))
    return out


def gemm_fns(N, D, S, cin, cout, k, ups, g):
    dev = "cuda"
    Si = S // 2 if ups else S
    x = torch.randn(N, cin, D, Si, Si, generator=g, device=dev).to(BF16).contiguous(memory_format=CL3)
    dy = torch.randn(N, cout, D, S, S, generator=g, device=dev).to(BF16).contiguous(memory_format=CL3)
    w = (torch.randn(cout, cin, k, k, k, generator=g, device=dev) / (cin * k ** 3) ** 0.5).contiguous()
    bias = torch.zeros(cout, device=dev)
    d = ops3d.descg(BF16, N, D, S, S, cin, cout, k, ups)
    cs = ops3d.Conv3dgState(w, d, dev, True)
    y = torch.empty((N, cout, D, S, S), dtype=BF16, device=dev, memory_format=CL3)
    dx = torch.empty((N, cin, D, S, S), dtype=BF16, device=dev, memory_format=CL3)
    dw, db = torch.empty_like(w), torch.empty(cout, device=dev)
    ws = torch.empty(L.query("fv_conv3dg_wgrad_ws_bytes", ctypes.byref(d)), dtype=torch.uint8, device=dev)
    st = L.stream()
    fwd = lambda: L.call("fv_conv3dg_fwd", ctypes.byref(d), x.data_ptr(), cs.wk.data_ptr(), bias.data_ptr(), y.data_ptr(), st)
    dgrad = lambda: L.call("fv_conv3dg_bwd_data", ctypes.byref(d), dy.data_ptr(), cs.wt.data_ptr(), dx.data_ptr(), st)
    wgrad = lambda: L.call("fv_conv3dg_bwd_weight", ctypes.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(),
                           db.data_ptr(), ws.data_ptr(), st)
    keep = (x, dy, w, bias, cs, y, dx, dw, db, ws, d)
    return fwd, dgrad, wgrad, keep


def bench_family(name, N, D, S, cin, cout, k, ups, window, g):
    fwd, dgrad, wgrad, keep = gemm_fns(N, D, S, cin, cout, k, ups, g)
    V = N * D * S * S
    Vi = V // 4 if ups else V
    flops = 2.0 * V * cout * cin * k ** 3
    bx, by, bw = Vi * cin * 2, V * cout * 2, cout * cin * k ** 3 * 2
    res = {name + "_fwd": roof(window_time(fwd, window), flops, bx + by + bw),
           name + "_dgrad": roof(window_time(dgrad, window), flops, by + V * cin * 2 + bw),
           name + "_wgrad": roof(window_time(wgrad, window), flops, bx + by + 2 * bw)}
    del keep
    torch.cuda.empty_cache()
    return res


def gemm_vs_direct(window, g, rounds=5):
    N, D, S, cin, cout = 2, 16, 64, 64, 32
    fwd, dgrad, wgrad, keep = gemm_fns(N, D, S, cin, cout, 3, False, g)
    x, dy, w, bias = keep[0], keep[1], keep[2], keep[3]
    dev = "cuda"
    d3 = ops3d.desc3(BF16, N, D, S, S, cin, cout)
    nb = L.query("fv_conv3d_wk_bytes", ctypes.byref(d3))
    wk, wt = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)
    st = L.stream()
    L.call("fv_conv3d_weight_prep", ctypes.byref(d3), w.data_ptr(), wk.data_ptr(), wt.data_ptr(), st)
    y = torch.empty((N, cout, D, S, S), dtype=BF16, device=dev, memory_format=CL3)
    dx = torch.empty((N, cin, D, S, S), dtype=BF16, device=dev, memory_format=CL3)
    dw, db = torch.empty_like(w), torch.empty(cout, device=dev)
    nws = L.query("fv_conv3d_wgrad_ws_bytes", ctypes.byref(d3))
    ws = torch.empty(max(nws, 4), dtype=torch.uint8, device=dev)
    old = dict(
        fwd=lambda: L.call("fv_conv3d_fwd", ctypes.byref(d3), x.data_ptr(), wk.data_ptr(), bias.data_ptr(), None,
                           y.data_ptr(), None, st),
        dgrad=lambda: L.call("fv_conv3d_bwd_data", ctypes.byref(d3), dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), st),
        wgrad=lambda: L.call("fv_conv3d_bwd_weight", ctypes.byref(d3), x.data_ptr(), dy.data_ptr(), dw.data_ptr(),
                             db.data_ptr(), ws.data_ptr() if nws else None, st))
    new = dict(fwd=fwd, dgrad=dgrad, wgrad=wgrad)
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: (max(v) - min(v)) / med(v)
    res = {}
    for kind in ("fwd", "dgrad", "wgrad"):
        t_old, t_new = [], []
        for _ in range(rounds):
            t_old.append(window_time(old[kind], window / rounds))
            t_new.append(window_time(new[kind], window / rounds))
        res[kind] = dict(new_us=round(med(t_new), 2), old_us=round(med(t_old), 2),
                         ratio_old_over_new=round(med(t_old) / med(t_new), 3),
                         spread_new=round(spread(t_new), 4), spread_old=round(spread(t_old), 4),
                         new_us_windows=[round(v, 2) for v in t_new], old_us_windows=[round(v, 2) for v in t_old])
    return res


def bench_model(N, window):
    torch.manual_seed(0)
    mfe = fv.MFE().cuda().train().set_compute_dtype(BF16)
    g = torch.Generator(device="cuda").manual_seed(1)
    fs = torch.randn(N, 32, 16, 64, 64, generator=g, device="cuda").to(BF16).contiguous(memory_format=CL3)
    fs.requires_grad_(True)
    kp_s = (torch.rand(N, 15, 3, generator=g, device="cuda") * 2 - 1).requires_grad_(True)
    kp_d = (torch.rand(N, 15, 3, generator=g, device="cuda") * 2 - 1).requires_grad_(True)
    R = torch.eye(3, device="cuda").expand(N, 3, 3).contiguous()

    def step():
        for p in mfe.parameters():
            p.grad = None
        deformation, occlusion, mask = mfe(fs, kp_s, kp_d, R, R)
        (deformation.sum() + occlusion.sum() + mask.square().sum()).backward()

    def fwd():
        with torch.no_grad():
            mfe(fs, kp_s, kp_d, R, R)

    t_f = window_time(fwd, window, min_iters=2) / 1e3
    t_s = window_time(step, window, min_iters=2) / 1e3
    return dict(batch=N, forward_ms=round(t_f, 3), forward_backward_ms=round(t_s, 3),
                peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mfebench needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(0)
    fam = {}
    for name, cin, cout, S, k, ups in mfe_convs():
        fam.update(bench_family(name, a.batch, 16, S, cin, cout, k, ups, a.window, g))
    res = dict(tool="mfebench", device=torch.cuda.get_device_name(0), dtype="bf16", batch=a.batch,
               window_s=a.window, peaks=dict(mfma_bf16_flops=PEAK_MFMA_BF16, hbm_bytes_per_s=PEAK_HBM),
               families=fam, gemm_vs_direct=gemm_vs_direct(max(a.window, 0.5), g))
    if not a.no_model:
        res["mfe"] = bench_model(a.batch, a.window)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
