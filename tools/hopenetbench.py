"""Timing of the frozen Hopenet teacher (csrc/hopenet.hip, ops_hopenet.py) at the workload's shape:
N = 96 images (source, driving and transformed driving at B = 32), bf16, 224 x 224.

    python tools/hopenetbench.py [--batch 96] [--window 0.1] [--rounds 5] [--out profiles/hopenet/hopenetbench.json]

Prints ONE JSON line, also written to --out.  Times are device events; two sides of a comparison run
in alternating windows (--rounds windows of at least --window seconds each per side, so at least
rounds x window >= 0.3 s per family), reported as the median window with the window spread
(max - min).

  bottlenecks   the first block (with its projection) and a later block of each of the four stages:
                the frozen block (three or four launches) against the tree's ResBottleneck(cin, cout,
                stride).eval() under no_grad at the same shape -- the training route's forward, which
                is what the tree had for this arithmetic; new us, parent-route us, ratio.
  trunk         the 16 frozen blocks of layers (3, 4, 6, 3) chained, against the sum of the parent-route
                stage times weighted by the block counts.
  pointwise     fv_pw_infer_fwd against fv_conv2d_fwd with ksize = 1 on the same operands at the two
                1x1 shapes of each stage's later block; us, achieved TFLOP/s, ratio.
  prep          fv_hopenet_prep_fwd (256 x 256 -> 224 x 224) against a device copy of the same bytes.
  teacher       the whole teacher_angles at N = 96 and N = 6: ms, TFLOP/s, share of the bf16 MFMA peak.
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
from facevae_amd import ops_hopenet as OH  # noqa: E402
from facevae_amd.hopenet import Bottleneck  # noqa: E402

CL = torch.channels_last
BF16 = torch.bfloat16
PEAK_BF16 = 2516.6e12          # dense bf16 MFMA peak, DESIGN.md §6
STAGES = [(64, 256, 1, 56), (256, 512, 2, 56), (512, 1024, 2, 28), (1024, 2048, 2, 14)]   # cin, cout, stride, input side
LAYERS = (3, 4, 6, 3)


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


def alternate(sides, window, rounds):
    """sides: {name: fn} -> {name: (median us, spread us, windows)} over alternating windows."""
    t = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            t[k].append(window_time(fn, window))
    return {k: (med(v), max(v) - min(v), [round(x, 2) for x in v]) for k, v in t.items()}


def rnd(shape, g, dtype=BF16):
    return torch.randn(shape, generator=g, device="cuda").to(dtype).contiguous(memory_format=CL)


def randomise(bns, g):
    with torch.no_grad():
        for m in bns:
            c = m.num_features
            m.running_mean.copy_(0.2 * torch.randn(c, generator=g, device="cuda"))
            m.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g, device="cuda"))
            m.weight.copy_(0.5 + torch.rand(c, generator=g, device="cuda"))


def block_flops(N, cin, cout, stride, side, project):
    mid, so = cout // 4, side // stride
    f = 2.0 * N * side * side * cin * mid + 2.0 * N * so * so * mid * mid * 9 + 2.0 * N * so * so * mid * cout
    return f + (2.0 * N * so * so * cin * cout if project else 0.0)


def bench_bottlenecks(N, window, rounds, g):
    out, frozen = {}, {}
    for si, (cin, cout, stride, side) in enumerate(STAGES):
        for kind, (ci, st, sd) in (("first", (cin, stride, side)), ("later", (cout, 1, side // stride))):
            project = kind == "first"
            ds = None
            if project:
                ds = torch.nn.Sequential(torch.nn.Conv2d(ci, cout, 1, stride=st, bias=False), torch.nn.BatchNorm2d(cout))
            holder = Bottleneck(ci, cout // 4, st, ds).cuda().eval()
            randomise([m for m in holder.modules() if isinstance(m, torch.nn.BatchNorm2d)], g)
            blk = OH._FrozenBlock(holder, BF16)
            ref = fv.ResBottleneck(ci, cout, st, False).cuda().eval().set_compute_dtype(BF16)
            with torch.no_grad():
                for s in list(ref.layers) + ([ref.down_sample] if ref.project else []):
                    s.conv.bias.zero_()
            x = rnd((N, ci, sd, sd), g)

            def parent(ref=ref, x=x):
                with torch.no_grad():
                    ref(x)

            r = alternate({"new": lambda blk=blk, x=x: blk.forward(x), "parent": parent}, window, rounds)
            fl = block_flops(N, ci, cout, st, sd, project)
            name = f"layer{si + 1}.{kind}"
            out[name] = dict(cin=ci, cout=cout, stride=st, side=sd, new_us=round(r["new"][0], 2),
                             parent_route_us=round(r["parent"][0], 2), ratio_parent_over_new=round(r["parent"][0] / r["new"][0], 3),
                             new_spread_us=round(r["new"][1], 2), parent_spread_us=round(r["parent"][1], 2),
                             new_us_windows=r["new"][2], parent_us_windows=r["parent"][2],
                             new_tflops=round(fl / (r["new"][0] * 1e-6) / 1e12, 1))
            frozen[(si, kind)] = blk
            del ref
    return out, frozen


def bench_trunk(N, fam, frozen, window, rounds, g):
    chain = []
    for si, n in enumerate(LAYERS):
        chain += [frozen[(si, "first")]] + [frozen[(si, "later")]] * (n - 1)
    x = rnd((N, 64, 56, 56), g)

    def run():
        h = x
        for b in chain:
            h = b.forward(h)

    t = [window_time(run, window) for _ in range(rounds)]
    count = lambda si, kind: 1 if kind == "first" else LAYERS[si] - 1        # noqa: E731
    tot = lambda key: sum(fam[f"layer{si + 1}.{kind}"][key] * count(si, kind)  # noqa: E731
                          for si in range(4) for kind in ("first", "later"))
    parent, spread = tot("parent_route_us"), tot("parent_spread_us")
    return dict(frozen_chain_us=round(med(t), 1), frozen_chain_spread_us=round(max(t) - min(t), 1),
                frozen_sum_of_blocks_us=round(tot("new_us"), 1), parent_route_sum_us=round(parent, 1),
                parent_route_spread_sum_us=round(spread, 1), ratio_parent_over_new=round(parent / med(t), 3),
                faster_by_more_than_parent_spread=bool(parent - med(t) > spread))


def bench_pointwise(N, window, rounds, g):
    out = {}
    st = L.stream()
    for cin, cout, stride, side in STAGES:
        sd, mid = side // stride, cout // 4
        for ci, co in ((cout, mid), (mid, cout)):
            x = rnd((N, ci, sd, sd), g)
            w = (torch.randn(co, ci, generator=g, device="cuda") / ci ** 0.5).contiguous()
            bias = torch.randn(co, generator=g, device="cuda")
            wk = OH.pw_weight_prep(BF16, w, None)
            y = torch.empty((N, co, sd, sd), dtype=BF16, device="cuda", memory_format=CL)
            dn = OH.pw_desc(BF16, N, sd, sd, 1, ci, co)
            d = ops.desc(BF16, N, sd, sd, ci, ci, co, co, 1)
            wk1 = torch.empty(L.query("fv_conv_wk_elems", ctypes.byref(d)), dtype=BF16, device="cuda")
            L.call("fv_conv_weight_prep", ctypes.byref(d), w.data_ptr(), None, wk1.data_ptr(), None, st)
            new = lambda: L.call("fv_pw_infer_fwd", ctypes.byref(dn), x.data_ptr(), wk.data_ptr(), bias.data_ptr(), None,  # noqa: E731
                                 y.data_ptr(), st)
            old = lambda: L.call("fv_conv2d_fwd", ctypes.byref(d), x.data_ptr(), wk1.data_ptr(), bias.data_ptr(), None,    # noqa: E731
                                 None, None, y.data_ptr(), None, st)
            r = alternate({"new": new, "conv2d_k1": old}, window, rounds)
            fl = 2.0 * N * sd * sd * ci * co
            out[f"{ci}x{co}@{N * sd * sd}px"] = dict(
                new_us=round(r["new"][0], 2), conv2d_k1_us=round(r["conv2d_k1"][0], 2),
                ratio_conv2d_over_new=round(r["conv2d_k1"][0] / r["new"][0], 3), new_spread_us=round(r["new"][1], 2),
                conv2d_k1_spread_us=round(r["conv2d_k1"][1], 2), new_tflops=round(fl / (r["new"][0] * 1e-6) / 1e12, 1),
                conv2d_k1_tflops=round(fl / (r["conv2d_k1"][0] * 1e-6) / 1e12, 1),
                mbytes=round((x.numel() + y.numel() + w.numel()) * 2 / 1e6, 2))
    return out


def bench_prep(N, window, rounds, g):
    frames = torch.rand(N, 3, 256, 256, generator=g, device="cuda")
    nbytes = 2 * N * 3 * 224 * 224 * 4
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    r = alternate({"prep": lambda: OH.preprocess(frames), "copy": lambda: dst.copy_(src)}, window, rounds)
    return dict(us=round(r["prep"][0], 2), spread_us=round(r["prep"][1], 2), mbytes=round(nbytes / 1e6, 2),
                copy_us=round(r["copy"][0], 2), vs_copy=round(r["copy"][0] / r["prep"][0], 3))


def bench_teacher(N, window, rounds):
    torch.manual_seed(0)
    net = fv.Hopenet().cuda().set_compute_dtype(BF16)
    frames = torch.rand(N, 3, 256, 256, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda")
    t = [window_time(lambda: net.teacher_angles(frames), window, min_iters=2) for _ in range(rounds)]
    fl = 2.0 * N * 112 * 112 * 64 * 147
    for si, (cin, cout, stride, side) in enumerate(STAGES):
        fl += block_flops(N, cin, cout, stride, side, True) + (LAYERS[si] - 1) * block_flops(N, cout, cout, 1, side // stride, False)
    us = med(t)
    return dict(batch=N, ms=round(us / 1e3, 3), spread_ms=round((max(t) - min(t)) / 1e3, 3), gflop=round(fl / 1e9, 1),
                tflops=round(fl / (us * 1e-6) / 1e12, 1), share_of_bf16_peak=round(fl / (us * 1e-6) / PEAK_BF16, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hopenet", "hopenetbench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hopenetbench needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(0)
    fam, frozen = bench_bottlenecks(a.batch, a.window, a.rounds, g)
    res = dict(tool="hopenetbench", device=torch.cuda.get_device_name(0), dtype="bf16", batch=a.batch, resolution=224,
               window_s=a.window, rounds=a.rounds, peaks=dict(bf16_mfma_flops_per_s=PEAK_BF16), bottlenecks=fam,
               trunk=bench_trunk(a.batch, fam, frozen, a.window, a.rounds, g))
    del frozen
    res["pointwise"] = bench_pointwise(a.batch, a.window, a.rounds, g)
    res["prep"] = bench_prep(a.batch, a.window, a.rounds, g)
    res["teacher"] = [bench_teacher(a.batch, a.window, a.rounds), bench_teacher(6, a.window, a.rounds)]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
