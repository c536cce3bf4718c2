"""FaceVAE training-step benchmark (BASELINE.json metric: training images/sec of the
256x256 face-VAE step; MFMA utilisation).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--res 256] [--dtype bf16]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N

One step = zero_grad -> forward (AFE trunk, reparam, Generator trunk) -> MSE + KL ->
backward (+ RCCL gradient all-reduce, SyncBN collectives when N > 1) -> Adam, on synthetic
VoxCeleb-shaped frames x ~ U[0,1) [B,3,H,H] and eps ~ N(0,1), resident in HBM before the
timed region.  Weak scaling: B images per GPU.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line.  --full adds what takes
runs of its own: the dominant kernel's HIP-event timing (`roofline`), the CPU oracle's rate
(`cpu_baseline`) and the first step's `parity` against it.  --dump-outputs DIR writes what the
last timed step computed as DIR/<name>.npy (float32; the same arguments give the same inputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import ops  # noqa: E402

PEAK_BF16_TFLOPS = 2516.6   # 256 CU x 2.4 GHz x 4096 FLOP/clk (dense), MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
PEAK_FP8_TFLOPS = 5033.2    # dense e4m3 (scaled 16x16x128: 2x bf16 per clock), MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU")
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8"],
                    help="fp8: the 3x3 128-multiple-channel convs' fwd + dgrad on e4m3 (config C5)")
    ap.add_argument("--no-syncbn", action="store_true", help="per-rank BN statistics (labelled)")
    ap.add_argument("--full", action="store_true",
                    help="also time the dominant kernel with HIP events (roofline), run the CPU baseline and "
                         "report the first step's parity against it; a plain run times the steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float32, <= 64 MB in all)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0,
                    help="CPU-baseline budget of a --full run (0 = skip)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = every core this process may use")
    ap.add_argument("--graph", type=int, default=1,
                    help="1 (default): replay the captured step (StepGraph: one HIP graph at one process, "
                         "graph segments between the collectives at N > 1), 0: eager launches")
    ap.add_argument("--comm", default="rccl", choices=["rccl", "gloo"],
                    help="N > 1 collectives: rccl (one GPU per rank, the product path) or gloo (TorchComm: "
                         "ranks may share a GPU -- tests on the one-GPU box)")
    return ap.parse_args()


def usable_cores():
    """(cores this process can run on, os.cpu_count()): the CPU affinity set capped by the
    cgroup CPU quota (cpu.max), which is what a job on the GPU box actually gets -- there
    os.cpu_count() shows the whole machine."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(q) // int(per)))
    except (OSError, ValueError):
        pass
    return n, os.cpu_count()


def conv_launch_flops(d):
    """Algorithmic FLOPs of one conv launch (reference formulation)."""
    return 2.0 * d.n * d.h * d.w * d.cout * d.cin_valid * d.ksize * d.ksize


def cpu_baseline(args, cfg, B, gpu_first=None):
    """The oracle (fp32 torch-CPU restatement of the reference step, math identical to the
    reference trainer) at the per-GPU shape (B images at cfg.H), on every core this process
    may use.  Its first step starts from the same seed-0 initial weights and inputs as the GPU
    run: that step is the untimed warm-up AND the parity reference -- `gpu_first` = the GPU's
    first step (image, R, K) -> the "parity" record of the bench line.  Then whole B-image
    steps until cpu_seconds."""
    from oracle import facevae_cpu as O   # checker / baseline only
    cores, ncpu = usable_cores()
    threads = args.cpu_threads or cores
    torch.set_num_threads(threads)
    ocfg = O.OracleConfig(H=cfg.H, down_seq=cfg.down_seq, latent=cfg.latent, n_res=cfg.n_res,
                          up_seq=cfg.up_seq)
    sd = O.prepare_state(O.init_state(ocfg, 0))
    opt = O.adam_init(sd)
    x = torch.rand(B, 3, cfg.H, cfg.H, generator=torch.Generator().manual_seed(1234))
    eps = torch.randn(B, cfg.latent, cfg.latent_hw, cfg.latent_hw, generator=torch.Generator().manual_seed(1235))
    oo, _ = O.train_step(sd, opt, x, eps, ocfg)                  # warm-up + parity reference
    parity = None
    if gpu_first is not None:
        y, R, K = gpu_first
        parity = {"image_rel_l2": round(((y - oo["y"]).norm() / oo["y"].norm()).item(), 6),
                  "R_rel": round(abs(R - oo["R"].item()) / oo["R"].item(), 7),
                  "K_rel": round(abs(K - oo["K"].item()) / abs(oo["K"].item()), 7),
                  "what": f"first step of this run ({args.dtype} kernels) vs the fp32 CPU oracle on the same "
                          f"weights and inputs; the north_star 1e-3 bar is met by the kernels' fp32 mode "
                          f"(tests/test_layers_gpu.py), bf16 / fp8 storage deviates by construction"}
    n, t0 = 0, time.perf_counter()
    while True:
        O.train_step(sd, opt, x, eps, ocfg)
        n += 1
        dt = time.perf_counter() - t0
        if dt >= args.cpu_seconds or n >= 20:
            break
    return {"value": round(n * B / dt, 4), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
            "os_cpu_count": ncpu, "usable_cores": cores,
            "sample": f"oracle fp32 step at {cfg.H}x{cfg.H}, batch {B} (the per-GPU shape), {n} timed step(s) "
                      f"({dt:.1f} s) after 1 untimed step (the parity reference); {torch.get_num_threads()} threads "
                      f"= the cores this process may use (affinity {len(os.sched_getaffinity(0))} CPUs capped by "
                      f"the cgroup quota; os.cpu_count() = {ncpu} is the whole machine)"}, parity


PMC_FILE = os.path.join(ROOT, "profiles", "r6_pmc.json")


def pmc_counters(cfg, B, dtype, fam, avg_ms):
    """Counter figures of the dominant kernel from the committed PMC passes (tools/gpu.sh pmc
    -> profiles/r6_pmc.json, tools/pmc_collect.py): HBM bytes per launch ((2 x FETCH_SIZE +
    WRITE_SIZE) KiB, the gfx950 correction of MI355X_MICROARCH.md), the MFMA busy fraction
    (SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs)) and the effective clock.
    Measured on the default 256x256, B=32 bf16 configuration only; others report null."""
    if not (cfg.H == 256 and B == 32 and dtype == torch.bfloat16 and os.path.exists(PMC_FILE)):
        return {}
    d = json.load(open(PMC_FILE))
    dom = (d.get("dominant") or {}).get(fam)
    if not dom:
        return {}
    out = {"pmc_source": "profiles/r6_pmc.json (" + dom["kernel"] + ")"}
    if "hbm_bytes_per_launch" in dom:
        t = dom["hbm_bytes_per_launch"]
        act = B * cfg.latent_hw ** 2 * cfg.up_seq[0] * 2          # one bf16 activation of the res stack
        # forward launches of the family: Generator.in_conv + 2 per ResBlock; the second conv of
        # each ResBlock also reads the residual input (n_res of the 2 n_res + 1 launches)
        res_share = cfg.n_res / (2 * cfg.n_res + 1)
        out.update({"traffic": round(t), "traffic_unit": "bytes/launch (PMC)",
                    "traffic_gbs_at_avg": round(t / (avg_ms * 1e-3) / 1e9, 1),
                    "algorithmic_bytes": round(2 * act + res_share * act + cfg.up_seq[0] ** 2 * 9 * 2),
                    "algorithmic_bytes_what": "input + output + weights per launch, + the residual input "
                                              f"averaged over the family ({cfg.n_res} of {2 * cfg.n_res + 1} launches)"})
    if "mfma_busy_frac" in dom:
        out.update({"mfma_busy_counter": round(dom["mfma_busy_frac"], 4),
                    "eff_clock_ghz": round(dom["eff_clock_ghz"], 3) if dom.get("eff_clock_ghz") else None})
    return out


DUMP_SAMPLE_SEED = 4321
# largest number of elements written per array (float32): 8M + 2 x 2M + 1M + scalars < 64 MB
DUMP_CAPS = {"y": 8 << 20, "mu": 2 << 20, "logstd": 2 << 20, "params": 1 << 20}


def dump_outputs(path, tensors):
    """Write each tensor of `tensors` (name -> device tensor) as path/<name>.npy in float32.  An
    array above its DUMP_CAPS entry is written as a fixed sample: the elements of the flattened
    array at sorted indices drawn from a seeded generator, the same for every run of the same
    shapes."""
    os.makedirs(path, exist_ok=True)
    for name, t in tensors.items():
        t = t.detach().float().reshape(-1)
        cap = DUMP_CAPS.get(name)
        if cap is not None and t.numel() > cap:
            idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).integers(0, t.numel(), size=cap))
            t = t[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy().astype(np.float32))


def main():
    args = parse()

    def comm_count():
        """ranks the RCCL communicator spans (ncclCommCount), None without one"""
        c = fv.distributed.get_comm()
        return c.count() if isinstance(c, fv.distributed.RcclComm) else None

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        fv.distributed.init_dist(local, world, backend="gloo" if args.comm == "gloo" else "nccl",
                                 syncbn=not args.no_syncbn)
    torch.cuda.set_device(local if args.comm == "rccl" else local % torch.cuda.device_count())
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp8": torch.float8_e4m3fn}[args.dtype]
    cfg = fv.FaceVAEConfig(H=args.res)
    torch.manual_seed(0)
    model = fv.FaceVAE(cfg).cuda().train().set_compute_dtype(dtype)
    net = fv.distributed.DataParallel(model) if world > 1 else model
    opt = fv.Adam(model.parameters(), lr=cfg.lr, betas=cfg.betas)
    rec, kl = fv.ReconLoss(), fv.KLDivergenceLoss()
    B = args.batch
    g = torch.Generator().manual_seed(1234 + rank)
    x = torch.rand(B, 3, cfg.H, cfg.H, generator=g).cuda()
    eps = torch.randn(B, cfg.latent, cfg.latent_hw, cfg.latent_hw,
                      generator=torch.Generator().manual_seed(1235 + rank)).cuda()

    # d(w_R R + w_K K) seeded straight into the two loss terms (no ones-fill, add or scalar
    # multiplies in the backward); the weighted sum is formed only for the returned value
    w_seed = (torch.tensor(cfg.w_R, device="cuda"), torch.tensor(cfg.w_K, device="cuda"))

    dump = args.dump_outputs if rank == 0 else None
    held = {}      # --dump-outputs: the last step's image and latent moments (a captured step's static outputs)

    def step(keep=None):
        opt.zero_grad(set_to_none=True)
        y, mu, logstd = net(x, eps)
        R, K = rec((x, y)), kl((mu, logstd))
        torch.autograd.backward([R, K], list(w_seed))
        opt.step()
        if keep is not None:
            keep.extend([y.detach(), R.detach(), K.detach()])
        if dump:
            held.update(y=y.detach(), mu=mu.detach(), logstd=logstd.detach())
        return R.detach(), K.detach()

    # dominant kernel family: the ResBlock 3x3 256->256 convs at the latent resolution
    res_c = cfg.up_seq[0]

    def is_res(kind, d):
        return d.ksize == 3 and d.cin_valid == res_c and d.cout == res_c and d.h == cfg.latent_hw

    timer = ops.KernelTimer(is_res)
    ops.TIMER = timer

    use_graph = bool(args.graph)
    run = step
    # warm-up step 1 (from the initial weights): with --full its image and losses are the GPU
    # side of the parity record (compared with the CPU oracle's first step in cpu_baseline)
    gpu_first = None
    if args.full:
        first = []
        step(first)
        gpu_first = (first[0].float().cpu(), first[1].item(), first[2].item())
    else:
        step()
    if use_graph:
        # W - 1 more eager warm-up steps, then one step captured into a HIP graph; two untimed replays
        sg = fv.StepGraph(step, [opt], warmup=max(1, args.warmup - 1)).capture()
        run = sg.replay
        for _ in range(2):
            run()
    else:
        for _ in range(args.warmup - 1):
            step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    timer.enabled = args.full and not use_graph
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = run()
    t_host = time.perf_counter() - t0      # host time to issue K steps (launches are async)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t = time.perf_counter() - t0
    timer.enabled = False
    if dump:
        # what the last timed step returned (R, K) and computed: the image, the latent moments
        # and the weights after its Adam update (sampled where an array is large)
        params = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
        dump_outputs(dump, {"R": loss[0], "K": loss[1], "params": params, **held})
        del params
    if args.full and use_graph:
        # the roofline kernel's launch durations: HIP events around its launches over K eager
        # steps right after the graph-timed region (ROCm refuses event nodes inside a capture)
        timer.enabled = True
        for _ in range(args.steps):
            step()
        timer.enabled = False
    if world > 1:
        tt = torch.tensor([t], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        t = tt.item()
    loss = cfg.w_R * loss[0] + cfg.w_K * loss[1]          # the weighted sum (trainer.py:250-251)
    assert torch.isfinite(loss).item()

    ms = t / args.steps * 1e3
    ips = world * B * args.steps / t
    ev = timer.summary()
    # algorithmic FLOPs of one res-conv launch (fwd, dgrad and wgrad have equal work)
    P = B * cfg.latent_hw * cfg.latent_hw
    f_launch = 2.0 * P * res_c * res_c * 9
    fam = {k: sum(v) / len(v) for k, v in ev.items() if v}
    # the roofline kernel: the res conv's forward launches.  conv3_halo_fwd3 (forward and data
    # gradient, 27 launches) is the step's largest kernel by time.  Every launch runs in line on
    # the compute stream; the forward launches are the ones named "fwd" by the timer (the data
    # gradient runs the same kernel on the transposed weights and is reported beside it in
    # families_avg_ms, as is the weight gradient)
    dom = "fwd" if "fwd" in fam else (max(fam, key=lambda k: fam[k] * len(ev[k])) if fam else None)
    peak = {torch.bfloat16: PEAK_BF16_TFLOPS, torch.float32: PEAK_F32_TFLOPS,
            torch.float8_e4m3fn: PEAK_FP8_TFLOPS}[dtype]
    roof = None
    if dom is not None:
        ach = f_launch / (fam[dom] * 1e-3) / 1e12
        roof = {"bound": "mfma", "kernel": f"conv3x3 {res_c}->{res_c} {dom} @{cfg.latent_hw}x{cfg.latent_hw} B={B}",
                "achieved": round(ach, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                "avg_ms": round(fam[dom], 4), "flop_per_launch": f_launch, "traffic": None,
                "families_avg_ms": {k: round(v, 4) for k, v in fam.items()},
                "timing": ("HIP events on the launch stream, K eager steps after the graph-timed region"
                           if use_graph else "HIP events on the launch stream over the timed region")}
        roof.update(pmc_counters(cfg, B, dtype, dom, fam[dom]))
    from oracle.facevae_cpu import OracleConfig, flops_per_image
    _, f_img = flops_per_image(OracleConfig(H=cfg.H, down_seq=cfg.down_seq, latent=cfg.latent,
                                            n_res=cfg.n_res, up_seq=cfg.up_seq))
    step_util = ips / world * f_img / (peak * 1e12)
    # sub-pixel shortcut (flag it): the two UpBlock2D convs run nearest-x2 upsample
    # + 3x3 as 4 phases of a 2x2 conv at the low resolution (forward, data and weight gradient),
    # executing 4/9 of the reference MACs; utilisation above is on reference FLOPs
    subpix = dtype != torch.float32 and os.environ.get("FV_DISABLE_SUBPIX", "0") != "1"
    f_up = sum(2.0 * (cfg.H // 2 ** (len(cfg.up_seq) - 2 - i)) ** 2 * cfg.up_seq[i] * cfg.up_seq[i + 1] * 9
               for i in range(len(cfg.up_seq) - 1))        # forward FLOPs of the up convs per image
    f_exec = f_img - (5.0 / 9.0) * 3 * f_up if subpix else f_img
    out = {
        "metric": "training images/sec (256x256 face-VAE step)" if cfg.H == 256 else
                  f"training images/sec ({cfg.H}x{cfg.H} face-VAE step)",
        "value": round(ips, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic (x~U[0,1), eps~N(0,1); seed-0 random init)",
        "config": {"workload": f"FaceVAE step {cfg.H}x{cfg.H} (AFE trunk + reparam + Generator trunk, MSE+KL, Adam)",
                   "global_batch": B * world, "per_gpu_batch": B, "resolution": cfg.H,
                   "parallelism": f"dp{world}" + ("" if world == 1 else (" syncbn" if not args.no_syncbn else " local-bn"))},
        "host_issue_ms_per_step": round(t_host / args.steps * 1e3, 3),
        "launch": ("hip graph (one captured step replayed)" if world == 1 else
                   "hip graph segments between the collectives (StepGraph)") if use_graph else "eager",
        "comm": None if world == 1 else args.comm,
        "rccl_comm_count": comm_count(),
        "loss_last": round(loss.item(), 6),
        "mfma_util_step": round(step_util, 4),
        "step_flop_per_image": f_img,
        "subpixel_shortcut": {"active": subpix, "executed_flop_per_image": f_exec,
                              "mfma_util_step_executed": round(ips / world * f_exec / (peak * 1e12), 4),
                              "what": "UpBlock2D upsample+3x3 as 4 low-res 2x2 phases (fwd, dgrad, wgrad): 4/9 of "
                                      "the reference MACs; mfma_util_step is on reference FLOPs"},
        "roofline": roof,
        "cpu_baseline": None,
        "parity": None,
    }
    if args.full and rank == 0 and world == 1 and args.cpu_seconds > 0:
        out["cpu_baseline"], out["parity"] = cpu_baseline(args, cfg, B, gpu_first)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()


if __name__ == "__main__":
    main()
