"""GPU tests of the reenactment inference path (csrc/animate.hip, warp.mfe_input / motion_warp /
frames_u8, MFE.infer, Generator.infer, Animator).

Kernel gates.  The fused kernels are compared with the fp64 CPU restatement (animate_reference.py,
from the oracle's functions) on dtype-rounded operands; the gate of each fused error is 2 x the
error of the existing unfused path (the parent's code: create_heatmap_representations +
create_sparse_motions + create_deformed_source_image + cat, and deformation_from_mask +
grid_sample_3d) measured on the same inputs in the same test, floored at 1e-6 rel-L2 so that a
bit-exact parent does not make the gate zero.  The factor allows a different but equally long fp32
evaluation order.  Module and end-to-end results in fp32 are held to the project's parity bar,
< 1e-3 relative against the reference fixtures; the bf16 end-to-end gate is 2 x the deviation of
the unfused bf16 composition from the same fixture, measured in the test.

Every test prints its measured errors (`pytest -s`); DESIGN.md section 17 has the tables measured
on an MI355X.
"""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import warp  # noqa: E402
import animate_reference as A  # noqa: E402
from animate_reference import BF16, F32, SHAPES, rel  # noqa: E402
from golden_io import load_golden  # noqa: E402

CL3 = torch.channels_last_3d
TOY_MFE = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)
FLOOR = 1e-6
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])


def _rep(t, n):
    return t if t.shape[0] == n else t.repeat(n, *([1] * (t.dim() - 1)))


def _cuda(m):
    return {k: v.cuda() for k, v in m.items()}


# ------------------------------------------------------------------ kernel a: the hourglass input

@DTYPES
@pytest.mark.parametrize("name", list(SHAPES))
def test_mfe_input_vs_fp64(name, dtype):
    N, Ns, K, C2, D, H, W = SHAPES[name]
    m = _cuda(A.motion_inputs(name))
    ref = A.mfe_input_fp64(name, dtype)
    fused = warp.mfe_input(m["fc"], m["kp_s"], m["kp_d"], m["Rs"], m["Rd"], dtype)
    assert fused.shape == ref.shape and fused.dtype == dtype and fused.is_contiguous(memory_format=CL3)
    # the parent's path needs the source repeated per driving sample
    fc, kp_s, Rs = _rep(m["fc"], N), _rep(m["kp_s"], N), _rep(m["Rs"], N)
    heat = warp.create_heatmap_representations(fc, kp_s, m["kp_d"])
    sm = warp.create_sparse_motions(fc, kp_s, m["kp_d"], Rs, m["Rd"])
    deformed = warp.create_deformed_source_image(fc, sm, dtype)
    unfused = torch.cat([heat.to(dtype), deformed], dim=2).view(N, -1, D, H, W)
    torch.cuda.synchronize()
    ef, eu = rel(fused, ref), rel(unfused, ref)
    gate = max(2 * eu, FLOOR)
    print(f"\nmfe_input {name} {'bf16' if dtype == BF16 else 'fp32'}: fused {ef:.3e} unfused {eu:.3e} gate {gate:.3e}"
          f" bit-equal {torch.equal(fused, unfused)}")
    assert ef <= gate, (ef, eu)
    f6 = fused.view(N, K + 1, C2 + 1, D, H, W)
    assert (f6[:, 0, 0] == 0).all()                              # k = 0 heat channel: exactly 0
    want = _rep(m["fc"].to(dtype), N)
    if all(A.identity_is_integral(s) for s in (D, H, W)):
        # the identity motion hits the voxel centres with weight exactly 1 at these sizes
        assert torch.equal(f6[:, 0, 1:], want)
    else:
        assert rel(f6[:, 0, 1:], want) <= gate


def test_identity_motion_is_exact_on_the_cpu_oracle_first():
    """The condition of the exactness assertion above, checked with the oracle before it is asked
    of the kernel.  In plain fp32 the source index of a voxel centre is integral at sizes 2, 3, 4, 5;
    under the contraction of `ix - floor(ix)` into one fma, which warp.hip's expression gets from
    hipcc and animate.hip keeps, only where size - 1 is a power of two (identity_is_integral).  The
    'centres' case has such sizes, and there the fp32 oracle returns fc bit for bit; the other cases
    are held to the gate instead."""
    N, Ns, K, C2, D, H, W = SHAPES["centres"]
    assert all(A.identity_is_integral(s) for s in (D, H, W))
    assert [s for s in range(2, 10) if A.identity_is_integral(s)] == [2, 3, 5, 9]
    for name in ("fixture", "odd_bcast", "tiny"):
        assert not all(A.identity_is_integral(s) for s in SHAPES[name][4:]), name
    fc = A.motion_inputs("centres")["fc"]
    grid = A.O.coordinate_grid_3d(D, H, W).unsqueeze(0)
    assert torch.equal(torch.nn.functional.grid_sample(fc, grid, align_corners=True), fc)


# ------------------------------------------------------------------ kernel b: blend + warp

@DTYPES
@pytest.mark.parametrize("C", [8, 32])
@pytest.mark.parametrize("name", list(SHAPES))
def test_motion_warp_vs_fp64(name, C, dtype):
    N, Ns, K, C2, D, H, W = SHAPES[name]
    m = _cuda(A.motion_inputs(name))
    fs_c, lg_c = A.volume(name, C, C), A.logits(name, C)
    rw, rd, rm = A.motion_warp_fp64(name, fs_c, lg_c, dtype)
    fs, lg = fs_c.cuda(), lg_c.cuda()
    w1, d1, p1 = warp.motion_warp(lg, fs, m["kp_s"], m["kp_d"], m["Rs"], m["Rd"], dtype, need_mask=True)
    w0, d0, p0 = warp.motion_warp(lg, fs, m["kp_s"], m["kp_d"], m["Rs"], m["Rd"], dtype)
    assert p0 is None and torch.equal(w0, w1) and torch.equal(d0, d1)      # the null probability pointer
    assert w1.dtype == dtype and w1.is_contiguous(memory_format=CL3) and d1.dtype == F32 and p1.dtype == F32
    assert w1.shape == rw.shape and d1.shape == rd.shape and p1.shape == rm.shape
    # the parent's path: repeated source, fp32 NCDHW logits, the sparse motions in memory
    fsr, kp_s, Rs = _rep(fs, N), _rep(m["kp_s"], N), _rep(m["Rs"], N)
    sm = warp.create_sparse_motions(fsr, kp_s, m["kp_d"], Rs, m["Rd"])
    du, pu = warp.deformation_from_mask(lg.to(dtype).float(), sm)
    wu = warp.grid_sample_3d(fsr, du, dtype)
    torch.cuda.synchronize()
    tag = f"motion_warp {name} C={C} {'bf16' if dtype == BF16 else 'fp32'}"
    for what, f, u, r in (("deformation", d1, du, rd), ("mask", p1, pu, rm), ("warped", w1, wu, rw)):
        ef, eu = rel(f, r), rel(u, r)
        gate = max(2 * eu, FLOOR)
        print(f"\n{tag}: {what} fused {ef:.3e} unfused {eu:.3e} gate {gate:.3e} bit-equal {torch.equal(f, u)}")
        assert ef <= gate, (what, ef, eu)
    sat = p1[0, :, 0, 0, 1, 0]                                             # the saturated voxel
    assert sat[K].item() == 1.0 and torch.isfinite(p1).all() and (sat[:K] < 1e-20).all()


def test_fused_ops_refuse_a_graph():
    m = _cuda(A.motion_inputs("tiny"))
    fc = m["fc"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        warp.mfe_input(fc, m["kp_s"], m["kp_d"], m["Rs"], m["Rd"], F32)
    kp = m["kp_d"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        warp.motion_warp(A.logits("tiny", 8).cuda(), A.volume("tiny", 8, 8).cuda(), m["kp_s"], kp, m["Rs"], m["Rd"], F32)
    with torch.no_grad():
        warp.mfe_input(fc, m["kp_s"], m["kp_d"], m["Rs"], m["Rd"], F32)
    with pytest.raises(fv._lib.FaceVAELibError, match="multiple of 8"):
        warp.motion_warp(A.logits("tiny", 8).cuda(), A.volume("tiny", 12, 8).cuda(), m["kp_s"], m["kp_d"], m["Rs"],
                         m["Rd"], F32)


# ------------------------------------------------------------------ kernel c: uint8 frames

def test_frames_u8_bit_equal_to_numpy():
    k = torch.arange(256, dtype=torch.float32) / 255
    special = torch.cat([k, torch.nextafter(k, torch.zeros(())), torch.tensor([-0.5, -1e-8, 0.0, 1.0, 1.0 + 1e-6, 7.0])])
    gen = torch.Generator().manual_seed(77)
    for shape in ((2, 3, 5, 7), (3, 3, 16, 20), (1, 3, 1, 1)):        # (1, 3, 1, 1): 6 bytes, the tail path
        n = 2 * shape[0] * 3 * shape[2] * shape[3]
        vals = torch.rand(n, generator=gen) * 1.4 - 0.2
        idx = torch.randperm(n, generator=gen)[:min(n // 2, special.numel())]
        vals[idx] = special[torch.randperm(special.numel(), generator=gen)[:idx.numel()]]
        if shape == (3, 3, 16, 20):
            vals[:special.numel()] = special                            # every special value at least once
        drv, img = vals[:n // 2].view(shape), vals[n // 2:].view(shape)
        want = A.frames_u8_numpy(drv, img)
        got = warp.frames_u8(drv.cuda(), img.cuda())
        assert got.dtype == torch.uint8 and got.shape == want.shape
        assert torch.equal(got.cpu(), want), shape


# ------------------------------------------------------------------ MFE.infer + the blend vs the reference

def test_mfe_infer_and_blend_match_reference_eval():
    gd = load_golden("mfe.pt")["mfe"]
    torch.manual_seed(int(gd["seed"]))
    mfe = fv.MFE(False, **TOY_MFE)
    mfe.load_state_dict(gd["buffers"], strict=False)          # the statistics eval_* were computed with
    mfe = mfe.cuda().eval().set_compute_dtype(F32)
    fs, kp_s, kp_d, Rs, Rd = (gd[k].cuda() for k in ("fs", "kp_s", "kp_d", "Rs", "Rd"))
    x, mask_logits, fc = mfe.infer(fs, kp_s, kp_d, Rs, Rd)
    assert not mask_logits.requires_grad and tuple(fc.shape) == (2, 3, 4, 8, 8)
    x2, ml2, _ = mfe.infer(None, kp_s, kp_d, Rs, Rd, fc=fc)    # the cached compress result
    assert torch.equal(x, x2) and torch.equal(mask_logits, ml2)
    _, deformation, mask = warp.motion_warp(mask_logits, fs, kp_s, kp_d, Rs, Rd, F32, need_mask=True)
    torch.cuda.synchronize()
    ed, em = rel(deformation, gd["eval_deformation"]), rel(mask, gd["eval_mask"])
    print(f"\nMFE.infer + motion_warp fp32 vs reference eval: deformation {ed:.2e} mask {em:.2e}")
    assert deformation.shape == gd["eval_deformation"].shape and mask.shape == gd["eval_mask"].shape
    assert ed < 1e-3 and em < 1e-3


# ------------------------------------------------------------------ Animator end to end

def _nets(mode):
    ctors = dict(afe=lambda: fv.AFE(False, [16, 32], n_res=1, C=8, D=4),
                 ckd=lambda: fv.CKD(False, down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3),
                 hpe_ede=lambda: fv.HPE_EDE(False, n_filters=[16, 32, 64], n_blocks=[1, 1], n_bins=6, K=3),
                 mfe=lambda: fv.MFE(False, **TOY_MFE), generator=lambda: fv.Generator(True, 1, [32, 16], D=4, C=8))
    isum = load_golden("animate.pt")["e2e"]["init_sum"]
    nets = {}
    for name, seed in A.SEEDS.items():
        torch.manual_seed(seed)
        net = ctors[name]()
        sd = net.state_dict()
        for k, v in isum[name].items():
            assert sd[k].double().sum().item() == v.item(), (name, k)
        A.perturb_stats(net, seed + 10)
        nets[name] = net.cuda().eval().set_compute_dtype(mode)
    return nets


def _animator(mode):
    n = _nets(mode)
    return fv.Animator(n["afe"], n["ckd"], n["hpe_ede"], n["mfe"], n["generator"]), n


@torch.no_grad()
def _unfused(n, s, d):
    """The composition the parent can already run: existing forwards in eval mode, the source side
    recomputed and repeated per driving frame."""
    T = d.shape[0]
    sr = s.expand(T, -1, -1, -1).contiguous()
    fs, kp_c = n["afe"](sr), n["ckd"](sr)
    kp_s, Rs = fv.transform_kp(kp_c, *n["hpe_ede"](sr))
    kp_d, Rd = fv.transform_kp(kp_c, *n["hpe_ede"](d))
    deformation, occlusion, _ = n["mfe"](fs, kp_s, kp_d, Rs, Rd)
    return n["generator"](fs, deformation, occlusion)


def test_animator_fp32_matches_reference():
    g = load_golden("animate.pt")["e2e"]
    anim, _ = _animator(F32)
    s, d = g["s"].cuda(), g["d"].cuda()
    gen = anim.set_source(s).drive(d)
    torch.cuda.synchronize()
    got = dict(kp_s=anim.kp_s, kp_d=anim.aux["kp_d"], deformation=anim.aux["deformation"],
               occlusion=anim.aux["occlusion"], generated=gen)
    errs = {k: rel(v, g[k]) for k, v in got.items()}
    print("\nAnimator fp32 vs reference: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in got.items():
        assert v.shape == g[k].shape and v.dtype == F32, k
        assert errs[k] < 1e-3, (k, errs[k])
    # batched against one source == each frame alone; a second call == the first: bit for bit
    one = torch.cat([anim.drive(d[i:i + 1]) for i in range(d.shape[0])])
    assert torch.equal(gen, one)
    assert torch.equal(anim.drive(d), gen)
    # uint8 frames == the yardstick applied to the float result
    u8 = anim.drive(d, as_uint8=True)
    assert torch.equal(u8.cpu(), A.frames_u8_numpy(d, gen))
    # new_pose = the frame's own estimated angles, zero delta: transform_kp's keypoints up to the
    # documented z-shift (0.33 - mean z over the call)
    yaw, pitch, roll, t, scale = anim.aux["pose"]
    kp_old = anim.aux["kp_d_old"].clone()
    anim.drive(d, new_pose=(yaw, pitch, roll))
    want = kp_old.clone()
    want[:, :, 2] += 0.33 - kp_old[:, :, 2].mean()
    e = rel(anim.aux["kp_d"], want)
    print(f"new_pose = own pose: kp_d vs transform_kp + z-shift {e:.2e}")
    assert e < 1e-5 and abs(anim.aux["kp_d"][:, :, 2].mean().item() - 0.33) < 1e-5


def test_animator_bf16_within_twice_the_unfused_deviation():
    g = load_golden("animate.pt")["e2e"]
    anim, n = _animator(BF16)
    s, d = g["s"].cuda(), g["d"].cuda()
    gen = anim.set_source(s).drive(d)
    ref_path = _unfused(n, s, d)
    torch.cuda.synchronize()
    ef, eu = rel(gen, g["generated"]), rel(ref_path, g["generated"])
    print(f"\nAnimator bf16 vs fp32 reference: generated fused {ef:.3e} unfused {eu:.3e} gate {2 * eu:.3e}")
    assert ef <= 2 * eu, (ef, eu)


def test_animator_peak_memory_below_unfused():
    """T = 4 frames against one source: the peak of drive() stays strictly below that of the unfused
    composition on four repeated sources (no sparse-motion / heat / per-motion sample tensors, no
    repeated fs)."""
    g = load_golden("animate.pt")["e2e"]
    anim, n = _animator(BF16)
    s = g["s"].cuda()
    d = torch.cat([g["d"], g["d"].flip(3)]).cuda()
    anim.set_source(s)

    def peak(fn):
        fn()                                                   # warm: code objects, cached workspaces
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del out
        return p
    fused, unfused = peak(lambda: anim.drive(d)), peak(lambda: _unfused(n, s, d))
    print(f"\npeak memory over the baseline, T = 4: Animator.drive {fused} B, unfused {unfused} B")
    assert fused < unfused
