"""GPU parity of the motion field estimator: the general 3-D implicit-GEMM conv kernels
(fv_conv3dg_*) against torch.nn.functional.conv3d in fp64 on the CPU on the same dtype-rounded
operands, DownBlock3D / UpBlock3D / MFE against the reference fixtures (tests/golden/mfe.pt),
and the AFE -> MFE -> Generator composition.

Gates.  bf16-stored outputs (y and dx in bf16 mode): rel-L2 <= 4e-3 and |d| <= 1.6e-2 max|ref|
(tests/test_afe3d_gpu.py: output rounded to bf16, fp32 accumulation, independent of K).
fp32-stored results (y and dx in fp32 mode, dW and db in both modes): rel-L2 <= 1e-5 where the
reduction length K <= 864 (the project's gate); for longer K the yardstick is torch's own fp32
conv3d (and its gradients) against the same fp64 result, gate = max(1e-5, 4 x that error): a
different but equally long fp32 summation order.  K = taps * cin (forward), taps * cout (data
gradient), voxels (weight and bias gradients).

Blocks and MFE in fp32 mode: < 1e-3 relative on outputs, input gradients, parameter gradients
and running statistics (the project's parity bar).  The bias of a conv in front of a
training-mode BatchNorm has a mathematically zero gradient (the reference's value is round-off
noise), so it is gated in absolute terms against the scale of its conv's weight gradient.

Every test prints its measured errors (`pytest -s`); DESIGN.md section 11 has the tables measured
on an MI355X.
"""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L, ops3d  # noqa: E402
from golden_io import load_golden  # noqa: E402

CL3 = torch.channels_last_3d
BF16, F32 = torch.bfloat16, torch.float32

# (N, cin, cout, D, H, W of the output, ksize, upsample)
CASES = {
    "80to64_k3": (2, 80, 64, 3, 4, 6, 3, False),        # cin not a power of two; K straddles taps
    "24to40_border": (1, 24, 40, 2, 2, 2, 3, False),    # every voxel on the border; < one tile; cout % 16 != 0
    "512to1024_deep": (1, 512, 1024, 2, 2, 2, 3, False),  # K = 13,824 forward; 8-voxel K, largest dW
    "16to8_ups": (2, 16, 8, 2, 4, 4, 3, True),          # upsample gather (input 2x2x2)
    "112to16_k7": (1, 112, 16, 4, 8, 8, 7, False),      # D < ksize, most depth taps outside
    "32to4_k1": (1, 32, 4, 2, 3, 5, 1, False),          # cout < 8; 30 voxels
    "64to32_split": (3, 64, 32, 5, 6, 10, 3, False),    # several voxel tiles, voxel split in wgrad
    # cout tiles x voxel tiles = 4 x 64 = 256: the threshold from which cout > 32 runs the 64 x 128
    # tile (every smaller case above with cout > 32 takes the 32 x 64 tile of the deep levels)
    "8to256_bigtile": (1, 8, 256, 2, 64, 64, 3, False),
}
TOY = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def maxd(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def _operands(name, dtype):
    N, cin, cout, D, H, W, k, ups = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    Hi, Wi = (H // 2, W // 2) if ups else (H, W)
    x = torch.randn(N, cin, D, Hi, Wi, generator=g).to(dtype).float()
    w = (torch.randn(cout, cin, k, k, k, generator=g) / math.sqrt(cin * k ** 3)).to(dtype).float()
    b = torch.randn(cout, generator=g)
    gy = torch.randn(N, cout, D, H, W, generator=g).to(dtype).float()
    return x, w, b, gy


def _torch_ref(name, dtype, prec):
    """(y, dx, dw, db) of torch's conv3d on the CPU in precision `prec` on the rounded operands."""
    N, cin, cout, D, H, W, k, ups = CASES[name]
    x, w, b, gy = _operands(name, dtype)
    xx, ww, bb = (t.to(prec).requires_grad_(True) for t in (x, w, b))
    xi = F.interpolate(xx, scale_factor=(1, 2, 2), mode="nearest") if ups else xx
    y = F.conv3d(xi, ww, bb, 1, k // 2)
    (y * gy.to(prec)).sum().backward()
    return y.detach(), xx.grad, ww.grad, bb.grad


_REFS = {}


def refs(name, dtype):
    """fp64 reference and torch's own fp32 error against it, computed once per (case, dtype)."""
    key = (name, dtype)
    if key not in _REFS:
        r64 = _torch_ref(name, dtype, torch.float64)
        r32 = _torch_ref(name, dtype, torch.float32)
        _REFS[key] = (r64, tuple(rel(a, b) for a, b in zip(r32, r64)))
    return _REFS[key]


def run_kernels(name, dtype):
    N, cin, cout, D, H, W, k, ups = CASES[name]
    x, w, b, gy = _operands(name, dtype)
    d = ops3d.descg(dtype, N, D, H, W, cin, cout, k, ups)
    cs = ops3d.Conv3dgState(w.cuda().contiguous(), d, "cuda", True)
    xb = x.cuda().to(dtype).contiguous(memory_format=CL3)
    gyb = gy.cuda().to(dtype).contiguous(memory_format=CL3)
    y = ops3d.conv3dg_forward(cs, xb, b.cuda())
    dx, dw, db = ops3d.conv3dg_backward(cs, xb, gyb)
    torch.cuda.synchronize()
    return y, dx, dw, db, (cs, xb, gyb)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(CASES))
def test_conv3dg_kernels_vs_torch_fp64(name, dtype):
    N, cin, cout, D, H, W, k, ups = CASES[name]
    (ry, rdx, rdw, rdb), e32 = refs(name, dtype)
    y, dx, dw, db, _ = run_kernels(name, dtype)
    assert y.shape == ry.shape and dx.shape == rdx.shape and dw.shape == rdw.shape
    taps, vox = k ** 3, N * D * H * W
    klen = {"y": taps * cin, "dx": taps * cout, "dw": vox, "db": vox}
    got = {"y": y.float(), "dx": dx.float(), "dw": dw, "db": db}
    ref = {"y": ry, "dx": rdx, "dw": rdw, "db": rdb}
    err32 = dict(zip(("y", "dx", "dw", "db"), e32))
    errs = {q: rel(got[q], ref[q]) for q in got}
    gates = {}
    for q in got:
        if dtype == BF16 and q in ("y", "dx"):
            gates[q] = 4e-3
        else:
            gates[q] = 1e-5 if klen[q] <= 864 else max(1e-5, 4 * err32[q])
    print(f"\nconv3dg {name} {'bf16' if dtype == BF16 else 'fp32'}: " + "  ".join(
        f"{q} err {errs[q]:.2e} (torch fp32 {err32[q]:.2e}, K {klen[q]}, gate {gates[q]:.1e})" for q in got))
    for q in got:
        assert errs[q] <= gates[q], (q, errs[q], gates[q])
        if dtype == BF16 and q in ("y", "dx"):
            assert maxd(got[q], ref[q]) <= 1.6e-2 * ref[q].abs().max().item(), q


def test_wgrad_is_bit_reproducible():
    """The split weight gradient (7 voxel splits at this shape) sums its slabs in a fixed order."""
    for dtype in (BF16, F32):
        _, _, dw1, db1, (cs, xb, gyb) = run_kernels("64to32_split", dtype)
        _, dw2, db2 = ops3d.conv3dg_backward(cs, xb, gyb)
        torch.cuda.synchronize()
        assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


@pytest.mark.parametrize("kw", [dict(cin=12), dict(ksize=5), dict(ups=True, w=5)])
def test_unsupported_descriptors_raise(kw):
    a = dict(cin=16, ksize=3, ups=False, w=6)
    a.update(kw)
    d = ops3d.descg(F32, 1, 2, 4, a["w"], a["cin"], 8, a["ksize"], a["ups"])
    assert L.query("fv_conv3dg_wk_bytes", ctypes.byref(d)) == 0
    with pytest.raises(L.FaceVAELibError):
        ops3d.Conv3dgState(torch.zeros(8, a["cin"], a["ksize"], a["ksize"], a["ksize"], device="cuda"), d, "cuda", True)
    x = torch.zeros(1, a["cin"], 2, 4, a["w"], device="cuda").contiguous(memory_format=CL3)
    buf = torch.zeros(1 << 16, device="cuda")
    with pytest.raises(L.FaceVAELibError):
        L.call("fv_conv3dg_fwd", ctypes.byref(d), L.ptr(x), L.ptr(buf), None, L.ptr(buf), L.stream())


# ------------------------------------------------------------------ blocks and MFE vs the reference

def _dead_bias(k):
    """Bias of a conv directly in front of a training-mode BN: zero gradient in exact arithmetic."""
    return k.endswith("layers.0.bias") and "layers" in k.rsplit("layers.0.bias", 1)[0]


def _check_param_grads(mod, gold, tol, label):
    worst = ("", 0.0)
    named = dict(mod.named_parameters())
    assert set(named) == set(gold)
    for k, p in named.items():
        assert p.grad is not None, k
        if _dead_bias(k):
            wk = k[:-len("bias")] + "weight"
            assert maxd(p.grad, gold[k]) <= tol * gold[wk].abs().max().item(), k
            continue
        e = rel(p.grad, gold[k])
        if e > worst[1]:
            worst = (k, e)
        assert e < tol, (k, e)
    print(f"{label}: worst parameter gradient {worst[0]} {worst[1]:.2e}")


def _check_buffers(mod, gold, tol):
    sd = mod.state_dict()
    for k, v in gold.items():
        if v.is_floating_point():
            assert rel(sd[k], v) < tol, k
        else:
            assert torch.equal(sd[k].cpu(), v), k


def _check_init(mod, gold):
    sd = mod.state_dict()
    for k, v in gold.items():
        assert sd[k].double().sum().item() == v.item(), k


@pytest.mark.parametrize("case", ["down3d", "up3d"])
def test_blocks_fp32_match_reference(case):
    gd = load_golden("mfe.pt")[case]
    torch.manual_seed(int(gd["seed"]))
    blk = fv.DownBlock3D(16, 24, False) if case == "down3d" else fv.UpBlock3D(24, 8, False)
    _check_init(blk, gd["init_sum"])
    blk = blk.cuda().train().set_compute_dtype(F32)
    x = gd["x"].cuda().requires_grad_(True)
    y = blk(x)
    assert y.shape == gd["out"].shape
    (y.float() * gd["g"].cuda()).sum().backward()
    torch.cuda.synchronize()
    ey, edx = rel(y, gd["out"]), rel(x.grad, gd["dx"])
    print(f"\n{case} fp32 vs reference: out {ey:.2e} dx {edx:.2e}")
    assert ey < 1e-3 and edx < 1e-3
    _check_param_grads(blk, gd["grads"], 1e-3, case)
    _check_buffers(blk, gd["buffers"], 1e-3)
    blk.eval()
    with torch.no_grad():
        ye = blk(gd["x"].cuda())
    assert rel(ye, gd["out_eval"]) < 1e-3


def _run_mfe(mode):
    gd = load_golden("mfe.pt")["mfe"]
    torch.manual_seed(int(gd["seed"]))
    mfe = fv.MFE(False, **TOY)
    _check_init(mfe, gd["init_sum"])
    mfe = mfe.cuda().train().set_compute_dtype(mode)
    ins = [gd[k].cuda().requires_grad_(True) for k in ("fs", "kp_s", "kp_d")]
    deformation, occlusion, mask = mfe(ins[0], ins[1], ins[2], gd["Rs"].cuda(), gd["Rd"].cuda())
    ((deformation * gd["g_def"].cuda()).sum() + (occlusion * gd["g_occ"].cuda()).sum()
     + (mask * gd["g_mask"].cuda()).sum()).backward()
    torch.cuda.synchronize()
    return gd, mfe, ins, (deformation, occlusion, mask)


def test_mfe_fp32_matches_reference():
    gd, mfe, ins, outs = _run_mfe(F32)
    errs = {}
    for name, t in zip(("deformation", "occlusion", "mask"), outs):
        assert t.shape == gd[name].shape and t.dtype == F32
        errs[name] = rel(t, gd[name])
    for name, t in zip(("d_fs", "d_kp_s", "d_kp_d"), ins):
        errs[name] = rel(t.grad, gd[name])
    print("\nMFE fp32 vs reference: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-3, (k, v)
    _check_param_grads(mfe, gd["grads"], 1e-3, "MFE fp32")
    _check_buffers(mfe, gd["buffers"], 1e-3)
    mfe.eval()
    with torch.no_grad():
        ev = mfe(gd["fs"].cuda(), gd["kp_s"].cuda(), gd["kp_d"].cuda(), gd["Rs"].cuda(), gd["Rd"].cuda())
    for name, t in zip(("eval_deformation", "eval_occlusion", "eval_mask"), ev):
        assert rel(t, gd[name]) < 1e-3, name


# bf16 MFE against the fp32 reference fixture: the deterministic deviations measured on an MI355X
# (deformation 5.46e-4, occlusion 8.61e-4, mask 1.21e-3, d_fs 7.63e-2,
# d_kp_s 7.20e-2, d_kp_d 7.03e-2, parameter gradients median 5.70e-2 / worst 1.69e-1 at
# compress.bias), gated at 2 x measured.  The step's existing bf16 gates that cover the same
# kind of quantity are looser or equal and stay the ceiling: 1e-2 for an output, 0.35 for the
# worst parameter gradient.
BF16_GATES = dict(deformation=1.1e-3, occlusion=1.8e-3, mask=2.5e-3, d_fs=0.153, d_kp_s=0.144, d_kp_d=0.141,
                  param_median=0.114, param_worst=0.34)


def test_mfe_bf16_vs_fp32_reference():
    gd, mfe, ins, outs = _run_mfe(BF16)
    errs = {}
    for name, t in zip(("deformation", "occlusion", "mask"), outs):
        errs[name] = rel(t, gd[name])
    for name, t in zip(("d_fs", "d_kp_s", "d_kp_d"), ins):
        errs[name] = rel(t.grad, gd[name])
    pe = sorted((rel(p.grad, gd["grads"][k]), k) for k, p in mfe.named_parameters() if not _dead_bias(k))
    errs["param_median"] = pe[len(pe) // 2][0]
    errs["param_worst"] = pe[-1][0]
    print("\nMFE bf16 vs fp32 reference: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f"  (worst: {pe[-1][1]})")
    for k, v in errs.items():
        assert v <= BF16_GATES[k], (k, v, BF16_GATES[k])


def test_afe_mfe_generator_compose():
    torch.manual_seed(5)
    afe = fv.AFE(False, [16, 32], n_res=1, C=8, D=4).cuda().train()
    mfe = fv.MFE(False, **TOY).cuda().train()
    gen = fv.Generator(True, 1, [32, 16], D=4, C=8).cuda().train()
    for m in (afe, mfe, gen):
        m.set_compute_dtype(BF16)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 16, 16, generator=g).cuda()              # AFE: [2, 8, 4, 8, 8]
    kp_s = ((torch.rand(2, 3, 3, generator=g) - 0.5) * 1.6).cuda()
    kp_d = ((torch.rand(2, 3, 3, generator=g) - 0.5) * 1.6).cuda()
    R = torch.eye(3).expand(2, 3, 3).contiguous().cuda()
    fs = afe(x)
    assert tuple(fs.shape) == (2, 8, 4, 8, 8)
    deformation, occlusion, mask = mfe(fs, kp_s, kp_d, R, R)
    img = gen(fs, deformation, occlusion)
    assert tuple(img.shape) == (2, 3, 16, 16) and torch.isfinite(img).all()
    img.float().square().sum().backward()
    torch.cuda.synchronize()
    for p in (mfe.compress.weight, mfe.down[0].layers[0].conv.weight, mfe.mask_conv.weight, mfe.occlusion_conv.weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum().item() > 0
