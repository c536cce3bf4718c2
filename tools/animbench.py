"""Per-frame latency of the reenactment inference path at the default sizes (256 x 256 frames, the
full-size networks, bf16): the Animator (facevae_amd/animate.py: cached source, fused motion
kernels) against the unfused composition the existing forwards give -- MFE.forward +
Generator.forward in eval mode with the source side recomputed for every frame, as evaluate.py's
per-frame loop does -- and, to separate the two gains, the unfused motion path on a cached source
(fs computed once and repeated per frame).  Two more variants time the one-frame-at-a-time remedy:
"animator_fused_pose" is drive(fused_pose=True), still eager, and "animator_graph" is the replay of
Animator.capture(T), the copy_ of the frames into the static input included.

    python tools/animbench.py [--frames 1 8] [--window 0.5] [--rounds 3] [--profile-kernels]
                              [--out profiles/animate/animbench.json]

Prints ONE JSON line (also written to --out).  Per frame count T: ms per frame of each variant by
device events around whole calls (warm-up, then --rounds timed windows of at least --window
seconds per variant, the variants alternating inside this one process), the median and the spread
(max - min over the median) of the windows; the library entries called per drive (every fv_* entry
is one launch or a fixed few) and, with --profile-kernels, the device kernels per call counted by
torch's profiler (torch's own copy / cat / cast kernels included; a run of its own, not timed);
the bytes of the intermediates the fused kernels no longer write, from the shapes;
"motion_breakdown": us per call of the fused launches alone against the ops they replace; and
"graph_gain": the eager Animator's median minus the replay's over the eager median, next to the larger
of the two spreads, which it has to exceed to count as a gain.
"""
import argparse
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L  # noqa: E402

BF16 = torch.bfloat16


class CountingLib:
    """Proxy of the loaded library that counts the fv_* entries fetched for a call."""

    def __init__(self, lib):
        self._real, self.counts = lib, collections.Counter()

    def __getattr__(self, name):
        if name.startswith("fv_"):
            self.counts[name] += 1
        return getattr(self._real, name)


def timed_ms(fn, window_s, min_iters=2):
    """ms per call over a window of at least window_s seconds."""
    s = torch.cuda.current_stream()
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
    return e0.elapsed_time(e1) / iters


def device_kernels(fn):
    """Device kernels of one call, counted by torch's profiler."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))


def bytes_not_written(T, K=15, C2=4, D=16, S=64, es=2):
    """Per drive of T frames: the tensors MFE.forward / Generator.forward write and the fused path
    does not (the hourglass input itself is written once by both)."""
    V = D * S * S
    K1 = K + 1
    b = dict(sparse_motion_f32=T * K1 * V * 3 * 4, heat_f32=T * K1 * V * 4, heat_cast=T * K1 * V * es,
             sampled_volumes=T * K1 * C2 * V * es, logits_f32_copy=T * K1 * V * 4, mask_f32=T * K1 * V * 4)
    b["total"] = sum(b.values())
    return b


@torch.no_grad()
def motion_breakdown(T, window, K=15, C=32, C2=4, D=16, S=64):
    """us per call of the motion assembly alone at the default MFE shapes, fused against the ops
    MFE.forward / Generator.forward run for the same tensors (source repeated per frame), and of the
    3 x 3 inverse both need once."""
    from facevae_amd import warp
    g = torch.Generator(device="cuda").manual_seed(2)
    cl3 = torch.channels_last_3d
    fc = torch.randn(1, C2, D, S, S, generator=g, device="cuda").to(BF16).contiguous(memory_format=cl3)
    fs = torch.randn(1, C, D, S, S, generator=g, device="cuda").to(BF16).contiguous(memory_format=cl3)
    lg = torch.randn(T, K + 1, D, S, S, generator=g, device="cuda").to(BF16).contiguous(memory_format=cl3)
    kp_s = torch.rand(1, K, 3, generator=g, device="cuda") - 0.5
    kp_d = torch.rand(T, K, 3, generator=g, device="cuda") - 0.5
    Rs = fv.rotation_matrix_z(torch.full((1,), 0.1, device="cuda"))
    Rd = fv.rotation_matrix_x(torch.linspace(-0.2, 0.2, T, device="cuda"))
    J = warp.motion_jacobian(Rs, Rd)
    rep = lambda t: t.expand(T, *t.shape[1:])                          # noqa: E731
    fcr, fsr, ksr, Rsr = (rep(t).contiguous(memory_format=cl3) if t.dim() == 5 else rep(t).contiguous()
                          for t in (fc, fs, kp_s, Rs))
    sm = warp.create_sparse_motions(fcr, ksr, kp_d, Rsr, Rd)

    def unfused_input():
        heat = warp.create_heatmap_representations(fcr, ksr, kp_d)
        m = warp.create_sparse_motions(fcr, ksr, kp_d, Rsr, Rd)
        deformed = warp.create_deformed_source_image(fcr, m, BF16)
        inp = torch.cat([heat.to(BF16).permute(0, 3, 4, 5, 1, 2), deformed.permute(0, 3, 4, 5, 1, 2)], dim=5)
        return inp.reshape(T, D, S, S, -1).permute(0, 4, 1, 2, 3)

    def unfused_warp():
        deformation, _ = warp.deformation_from_mask(lg, sm)
        return warp.grid_sample_3d(fsr, deformation, BF16)

    fns = dict(fused_input=lambda: warp.mfe_input(fc, kp_s, kp_d, Rs, Rd, BF16, J=J), unfused_input=unfused_input,
               fused_warp=lambda: warp.motion_warp(lg, fs, kp_s, kp_d, Rs, Rd, BF16, J=J), unfused_warp=unfused_warp,
               inverse_3x3=lambda: torch.inverse(Rd))
    out = {}
    for name, fn in fns.items():
        fn()
        fn()
        out[name + "_us"] = round(timed_ms(fn, window / 2) * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--profile-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("animbench needs a GPU")
    torch.manual_seed(0)
    nets = dict(afe=fv.AFE(), ckd=fv.CKD(), hpe_ede=fv.HPE_EDE(), mfe=fv.MFE(), generator=fv.Generator())
    for m in nets.values():
        m.cuda().eval().set_compute_dtype(BF16)
    anim = fv.Animator(nets["afe"], nets["ckd"], nets["hpe_ede"], nets["mfe"], nets["generator"])
    g = torch.Generator(device="cuda").manual_seed(1)
    s = torch.rand(1, 3, a.size, a.size, generator=g, device="cuda")
    anim.set_source(s)
    counting = CountingLib(L.load())

    @torch.no_grad()
    def unfused(d, cached):
        T = d.shape[0]
        if cached:
            rep = lambda t: t.expand(T, *t.shape[1:]).contiguous()      # noqa: E731
            fs, kp_c, kp_s, Rs = rep(anim.fs), anim.kp_c, rep(anim.kp_s), rep(anim.Rs)
        else:
            sr = s.expand(T, -1, -1, -1).contiguous()
            fs, kp_c = nets["afe"](sr), nets["ckd"](sr)
            kp_s, Rs = fv.transform_kp(kp_c, *nets["hpe_ede"](sr))
        kp_d, Rd = fv.transform_kp(kp_c, *nets["hpe_ede"](d))
        deformation, occlusion, _ = nets["mfe"](fs, kp_s, kp_d, Rs, Rd)
        return nets["generator"](fs, deformation, occlusion)

    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    res = dict(tool="animbench", device=torch.cuda.get_device_name(0), dtype="bf16", size=a.size, window_s=a.window,
               rounds=a.rounds, frames={})
    for T in a.frames:
        d = torch.rand(T, 3, a.size, a.size, generator=g, device="cuda")
        cap = anim.capture(T)
        variants = dict(animator=lambda: anim.drive(d), unfused=lambda: unfused(d, False),
                        unfused_cached_source=lambda: unfused(d, True),
                        animator_fused_pose=lambda: anim.drive(d, fused_pose=True), animator_graph=lambda: cap(d))
        out = {}
        for name, fn in variants.items():            # warm-up and the counts of one call
            fn()
            fn()
            torch.cuda.synchronize()
            L._lib, counting.counts = counting, collections.Counter()
            fn()
            L._lib = counting._real
            out[name] = dict(entry_calls=sum(counting.counts.values()), entries=dict(sorted(counting.counts.items())),
                             device_kernels=device_kernels(fn) if a.profile_kernels else None,
                             windows_ms_per_frame=[])
        for _ in range(a.rounds):                    # alternating windows
            for name, fn in variants.items():
                out[name]["windows_ms_per_frame"].append(round(timed_ms(fn, a.window) / T, 4))
        for name in variants:
            w = out[name]["windows_ms_per_frame"]
            out[name].update(ms_per_frame=med(w), spread=round((max(w) - min(w)) / med(w), 4))
        out["animator_over_unfused"] = round(out["animator"]["ms_per_frame"] / out["unfused"]["ms_per_frame"], 4)
        out["animator_over_unfused_cached_source"] = round(
            out["animator"]["ms_per_frame"] / out["unfused_cached_source"]["ms_per_frame"], 4)
        eager, graph = out["animator"], out["animator_graph"]
        gain = (eager["ms_per_frame"] - graph["ms_per_frame"]) / eager["ms_per_frame"]
        out["graph_gain"] = dict(gain=round(gain, 4), larger_spread=max(eager["spread"], graph["spread"]),
                                 above_spread=gain > max(eager["spread"], graph["spread"]))
        out["bytes_not_written"] = bytes_not_written(T, S=a.size // 4)
        out["motion_breakdown"] = motion_breakdown(T, a.window, S=a.size // 4)
        res["frames"][str(T)] = out
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
