"""GPU tests of the graph-captured Animator frame path: the fused pose kernels (fv_pose_kp_fwd,
fv_pose_kp_new_fwd), the uint8 way in (fv_frames_from_u8), Animator.drive(fused_pose=True),
Animator.capture / CapturedDrive (replay, set_source in place, new_pose, uint8 in and out, stream)
and an EFE in the captured loop.

Kernel gates.  The pose kernels are compared with the fp64 CPU restatement (pose_reference.py, held to
the reference fixtures by test_pose_fused_cpu.py) on fp32 inputs; the gate of each error is 2 x the error
of the existing torch path (transform_kp / transform_kp_with_new_pose + warp.motion_jacobian) measured
on the same inputs in the same test, floored at 1e-6 rel-L2, as in test_animate_gpu.py.  Against the two
reference fixtures the kernels are held to the project's parity bar, < 1e-3.  A captured replay is held
to torch.equal with the eager drive(fused_pose=True) call it recorded: the same kernels on the same
inputs.  Every test prints its measured errors (`pytest -s`).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import pose, warp  # noqa: E402
from facevae_amd.data import u8_to_float  # noqa: E402
import animate_reference as A  # noqa: E402
import pose_reference as P  # noqa: E402
from animate_reference import BF16, F32  # noqa: E402
from golden_io import load_golden  # noqa: E402
from pose_reference import rel  # noqa: E402
from test_efe_cpu import TOY as EFE_TOY  # noqa: E402

TOY_MFE = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)
FLOOR = 1e-6
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
AUX = ("kp_d", "Rd", "deformation", "occlusion")


def _cuda(m):
    return {k: v.cuda() for k, v in m.items()}


def _gate(tag, names, fused, torch_path, ref):
    for what, f, u, r in zip(names, fused, torch_path, ref):
        ef, eu = rel(f, r), rel(u, r)
        gate = max(2 * eu, FLOOR)
        print(f"\n{tag}: {what} fused {ef:.3e} torch {eu:.3e} gate {gate:.3e}")
        assert f.shape == r.shape and f.dtype == F32, what
        assert ef <= gate, (what, ef, eu)


# ------------------------------------------------------------------ the pose kernels

@pytest.mark.parametrize("with_Rs", [True, False], ids=["Rs", "noRs"])
@pytest.mark.parametrize("name", list(P.CASES))
def test_pose_kp_vs_fp64(name, with_Rs):
    a = P.pose_inputs(name)
    g = _cuda(a)
    Rs = a["Rs"] if with_Rs else None
    args = ("kp_c", "yaw", "pitch", "roll", "t", "scale")
    ref = P.transform_kp_fp64(*(a[k] for k in args), Rs)
    got = pose.pose_kp(*(g[k] for k in args), g["Rs"] if with_Rs else None)
    kp_t, R_t = fv.transform_kp(*(g[k] for k in args))
    torch.cuda.synchronize()
    if with_Rs:
        _gate(f"pose_kp {name}", ("kp", "R", "J"), got, (kp_t, R_t, warp.motion_jacobian(g["Rs"], R_t)), ref)
    else:
        assert got[2] is None
        _gate(f"pose_kp {name} no Rs", ("kp", "R"), got[:2], (kp_t, R_t), ref[:2])
    again = pose.pose_kp(*(g[k] for k in args), g["Rs"] if with_Rs else None)
    assert all(torch.equal(x, y) for x, y in zip(got, again) if x is not None)


@pytest.mark.parametrize("with_Rs", [True, False], ids=["Rs", "noRs"])
@pytest.mark.parametrize("name", list(P.CASES))
def test_pose_kp_new_vs_fp64(name, with_Rs):
    N, Nc, Ns, K = P.CASES[name]
    a = P.pose_inputs(name)
    g = _cuda(a)
    kp_in = (a["scale"].view(N, 1, 1) * a["kp_c"]).contiguous()          # fp32-rounded, as the caller forms it
    rest = ("yaw", "pitch", "roll", "t", "delta", "new_yaw", "new_pitch", "new_roll")
    ref = P.transform_kp_new_fp64(kp_in, *(a[k] for k in rest), a["Rs"] if with_Rs else None)
    got = pose.pose_kp_new(kp_in.cuda(), *(g[k] for k in rest), g["Rs"] if with_Rs else None)
    kp_t, R_t = fv.transform_kp_with_new_pose(kp_in.cuda(), *(g[k] for k in rest))
    torch.cuda.synchronize()
    if with_Rs:
        _gate(f"pose_kp_new {name}", ("kp", "R", "J"), got, (kp_t, R_t, warp.motion_jacobian(g["Rs"], R_t)), ref)
    else:
        assert got[2] is None
        _gate(f"pose_kp_new {name} no Rs", ("kp", "R"), got[:2], (kp_t, R_t), ref[:2])
    mz = got[0][:, :, 2].double().mean().item()
    print(f"pose_kp_new {name}: |mean z - 0.33| = {abs(mz - 0.33):.2e}")
    assert abs(mz - 0.33) < 1e-5
    again = pose.pose_kp_new(kp_in.cuda(), *(g[k] for k in rest), g["Rs"] if with_Rs else None)
    assert all(torch.equal(x, y) for x, y in zip(got, again) if x is not None)


def test_pose_kernels_match_the_reference_fixtures():
    gd = load_golden("hpe.pt")["pose"]
    i = _cuda(gd["inputs"])
    kp, R, J = pose.pose_kp(i["kp"], i["yaw"], i["pitch"], i["roll"], i["t"], i["scale"])
    e1 = (rel(kp, gd["kp_out"]), rel(R, gd["R"]))
    g = load_golden("animate.pt")["new_pose"]
    c = _cuda({k: v for k, v in g.items() if k not in ("kp", "rot")})
    kp2, R2, _ = pose.pose_kp_new(c["kp_c"], c["yaw"], c["pitch"], c["roll"], c["t"], c["delta"], c["new_yaw"],
                                  c["new_pitch"], c["new_roll"])
    e2 = (rel(kp2, g["kp"]), rel(R2, g["rot"]))
    print(f"\npose_kp vs hpe.pt: kp {e1[0]:.2e} R {e1[1]:.2e}; pose_kp_new vs animate.pt: kp {e2[0]:.2e} R {e2[1]:.2e}")
    assert J is None and max(e1) < 1e-3 and max(e2) < 1e-3


def test_pose_ops_refuse_a_graph_and_bad_shapes():
    g = _cuda(P.pose_inputs("b"))
    args = [g[k] for k in ("kp_c", "yaw", "pitch", "roll", "t", "scale")]
    kp = args[0].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        pose.pose_kp(kp, *args[1:])
    with torch.no_grad():
        pose.pose_kp(kp, *args[1:])
    with pytest.raises(ValueError, match="Rs"):
        pose.pose_kp(*args, Rs=g["Rs"].repeat(2, 1, 1))
    with pytest.raises(ValueError, match="kp_c"):
        pose.pose_kp(args[0].repeat(2, 1, 1), *args[1:])
    # the single block's bound: 65536 keypoints
    N, K = 4097, 16
    z = torch.zeros(N, device="cuda")
    with pytest.raises(fv._lib.FaceVAELibError, match="N K <= 65536"):
        pose.pose_kp_new(torch.zeros(N, K, 3, device="cuda"), z, z, z, torch.zeros(N, 3, device="cuda"),
                         torch.zeros(N, K, 3, device="cuda"), z, z, z)


# ------------------------------------------------------------------ uint8 in

def _bytes(shape, seed):
    n = int(np.prod(shape))
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n,), generator=gen, dtype=torch.int64)
    if n >= 256:
        x[torch.randperm(n, generator=gen)[:256]] = torch.arange(256)      # every byte value at least once
    return x.to(torch.uint8).view(shape)


def test_frames_from_u8_bit_equal_to_u8_to_float():
    seen = set()
    for i, shape in enumerate(((1, 1, 1, 3), (2, 5, 7, 3), (3, 16, 20, 3))):   # 3 bytes: the tail path alone
        x = _bytes(shape, 90 + i)
        seen |= set(x.flatten().tolist())
        want = torch.from_numpy(u8_to_float(x.numpy())).permute(0, 3, 1, 2)
        got = warp.frames_from_u8(x.cuda())
        assert got.dtype == F32 and got.is_contiguous() and tuple(got.shape) == (shape[0], 3, shape[1], shape[2])
        assert torch.equal(got.cpu(), want), shape
        # a buffer that starts off a 4-byte boundary: the byte-load path
        flat = torch.zeros(x.numel() + 1, dtype=torch.uint8, device="cuda")
        flat[1:] = x.flatten().cuda()
        assert flat[1:].data_ptr() % 4 == 1
        assert torch.equal(warp.frames_from_u8(flat[1:].view(shape)).cpu(), want), shape
        # and back out: the left half of the side-by-side frame is the input
        back = warp.frames_u8(got, got)
        W = shape[2]
        assert torch.equal(back[:, :, :W].cpu(), x) and torch.equal(back[:, :, W:].cpu(), x), shape
    assert seen == set(range(256))
    with pytest.raises(RuntimeError, match="uint8"):
        warp.frames_from_u8(torch.zeros(1, 2, 2, 3, device="cuda"))


# ------------------------------------------------------------------ Animator: fused pose, capture

_NETS = {}


def _nets(mode):
    """The seeded toy networks of tests/golden/animate.pt, built once per compute dtype (an Animator only
    reads them)."""
    if mode not in _NETS:
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
        _NETS[mode] = nets
    return _NETS[mode]


def _animator(mode, efe=None):
    n = _nets(mode)
    return fv.Animator(n["afe"], n["ckd"], n["hpe_ede"], n["mfe"], n["generator"], efe)


def _frames(seed, T=2):
    return torch.rand(T, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).cuda()


def _snapshot(out, aux):
    return dict(out=out.clone(), **{k: aux[k].clone() for k in AUX})


def _eager(anim, d, **kw):
    out = anim.drive(d, fused_pose=True, **kw)
    return _snapshot(out, anim.aux)


def _same(got, want, tag):
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (tag, k)


def test_drive_fused_pose_fp32_matches_reference():
    g = load_golden("animate.pt")["e2e"]
    anim = _animator(F32).set_source(g["s"].cuda())
    d = g["d"].cuda()

    def run(**kw):
        gen = anim.drive(d, **kw)
        return dict(kp_d=anim.aux["kp_d"], deformation=anim.aux["deformation"], occlusion=anim.aux["occlusion"],
                    generated=gen)
    default, fused = run(), run(fused_pose=True)
    torch.cuda.synchronize()
    for k in fused:
        ef, eu = rel(fused[k], g[k]), rel(default[k], g[k])
        gate = max(2 * eu, FLOOR)
        print(f"\ndrive fp32 vs reference: {k} fused_pose {ef:.3e} default {eu:.3e} gate {gate:.3e}")
        assert fused[k].shape == g[k].shape and ef < 1e-3 and ef <= gate, (k, ef, eu)
    # nothing in the fused call waits for the host: torch raises on any synchronising call in this mode
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = anim.drive(d, fused_pose=True)
        anim.drive(d, new_pose=(0.1, -0.2, 0.05), as_uint8=True, fused_pose=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again, fused["generated"])
    # uint8 frames and a float new_pose go through the same call
    u8 = anim.drive(d, as_uint8=True, fused_pose=True)
    assert torch.equal(u8.cpu(), A.frames_u8_numpy(d, fused["generated"]))
    anim.drive(d, new_pose=(0.1, -0.2, 0.05), fused_pose=True)
    kp_f = anim.aux["kp_d"].clone()
    anim.drive(d, new_pose=(0.1, -0.2, 0.05))
    e = rel(kp_f, anim.aux["kp_d"])
    print(f"new_pose kp_d, fused_pose vs default: {e:.2e}")
    assert e < 1e-5 and abs(kp_f[:, :, 2].mean().item() - 0.33) < 1e-5


@DTYPES
@pytest.mark.parametrize("T", [2, 1])
def test_capture_replay_equals_eager(T, dtype):
    g = load_golden("animate.pt")["e2e"]
    anim = _animator(dtype).set_source(g["s"].cuda())
    d = g["d"].cuda()[:T].contiguous()
    want = _eager(anim, d)
    cap = anim.capture(T)
    assert isinstance(cap, fv.CapturedDrive)
    out = cap(d)
    assert out.dtype == F32 and tuple(out.shape) == (T, 3, 64, 64)
    _same(_snapshot(out, cap.aux), want, "fixture frames")
    ptrs = [out.data_ptr()] + [cap.aux[k].data_ptr() for k in AUX]
    d2 = _frames(41, T)
    want2 = _eager(anim, d2)
    out2 = cap(d2)
    _same(_snapshot(out2, cap.aux), want2, "seeded frames")
    assert not torch.equal(want2["out"], want["out"])
    assert [out2.data_ptr()] + [cap.aux[k].data_ptr() for k in AUX] == ptrs
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for i in range(20):
        cap(d if i % 2 else d2)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base
    _same(_snapshot(cap.out, cap.aux), want, "after twenty replays")


def test_set_source_after_capture_drives_the_new_source():
    g = load_golden("animate.pt")["e2e"]
    anim = _animator(F32).set_source(g["s"].cuda())
    d = g["d"].cuda()
    cap = anim.capture(2)
    first = cap(d).clone()
    s2 = _frames(43, 1)
    anim.set_source(s2)
    want = _eager(_animator(F32).set_source(s2), d)
    _same(_snapshot(cap(d), cap.aux), want, "second source")
    assert not torch.equal(first, want["out"])
    with pytest.raises(ValueError, match="capture again"):
        anim.set_source(_frames(44, 2))
    with pytest.raises(ValueError, match="capture again"):
        anim.set_source(torch.rand(1, 3, 32, 32, device="cuda"))
    _same(_snapshot(cap(d), cap.aux), want, "after the refused sources")


def test_capture_new_pose_takes_new_angles_every_replay():
    g = load_golden("animate.pt")["e2e"]
    anim = _animator(F32).set_source(g["s"].cuda())
    d = g["d"].cuda()
    cap = anim.capture(2, new_pose=True)
    last = None
    for angles in ((0.0, 0.0, 0.0), (0.2, -0.1, 0.3), (torch.tensor([0.3, -0.3]).cuda(), 0.1, torch.tensor(-0.2).cuda())):
        want = _eager(anim, d, new_pose=angles)
        got = _snapshot(cap(d, new_pose=angles), cap.aux)
        _same(got, want, angles)
        assert last is None or not torch.equal(got["kp_d"], last)
        last = got["kp_d"]
    with pytest.raises(ValueError, match="new_pose"):
        cap(d)
    with pytest.raises(ValueError, match="new_pose"):
        anim.capture(2)(d, new_pose=(0.0, 0.0, 0.0))


def test_capture_uint8_in_and_out_and_stream():
    g = load_golden("animate.pt")["e2e"]
    anim = _animator(BF16).set_source(g["s"].cuda())
    cap = anim.capture(2, as_uint8=True, u8_in=True)
    chunks = [_bytes((2, 64, 64, 3), 60 + i).numpy() for i in range(5)]
    singles = []
    for i, c in enumerate(chunks):
        out = cap(torch.from_numpy(c).cuda())
        assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 64, 128, 3)
        singles.append(out.cpu())
        if i < 2:
            df = torch.from_numpy(u8_to_float(c)).permute(0, 3, 1, 2).contiguous()
            gen = anim.drive(df.cuda(), fused_pose=True)
            assert torch.equal(singles[i], A.frames_u8_numpy(df, gen.cpu())), i
    streamed = list(cap.stream(iter(chunks)))
    assert len(streamed) == 5
    for i, (a, b) in enumerate(zip(streamed, singles)):
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and np.array_equal(a, b.numpy()), i
    assert list(cap.stream([])) == []
    assert np.array_equal(next(cap.stream(chunks[3:])), singles[3].numpy())       # a stream left early, then reused
    assert np.array_equal(list(cap.stream(chunks[:1]))[0], singles[0].numpy())
    with pytest.raises(ValueError, match="captured for"):
        list(cap.stream([chunks[0][:1]]))
    with pytest.raises(RuntimeError, match="u8_in"):
        next(anim.capture(2).stream(chunks))


@DTYPES
def test_capture_with_an_efe_in_the_loop(dtype):
    """The smallest EFE_conv5 configuration of tests/test_efe_gpu.py (test_efe_cpu.TOY: two halvings
    to the 4 x 4 code at scale 0.25) takes 64 x 64 frames, the size of the animate.pt toy networks, and
    K = 3 as they do; graph against eager, no reference needed."""
    g = load_golden("animate.pt")["e2e"]
    torch.manual_seed(306)
    efe = fv.EFE_conv5(False, **EFE_TOY)
    A.perturb_stats(efe, 316)
    efe = efe.cuda().eval().set_compute_dtype(dtype)
    anim = _animator(dtype, efe).set_source(g["s"].cuda())
    d = g["d"].cuda()
    want = _eager(anim, d)
    assert not torch.equal(anim.aux["kp_d"], anim.aux["kp_d_old"])       # the EFE moved the keypoints
    cap = anim.capture(2)
    _same(_snapshot(cap(d), cap.aux), want, "efe")
    angles = (0.1, 0.0, -0.1)
    want = _eager(anim, d, new_pose=angles)                             # a non-zero expression offset
    cap = anim.capture(2, new_pose=True)
    _same(_snapshot(cap(d, new_pose=angles), cap.aux), want, "efe new_pose")


def test_capture_errors():
    g = load_golden("animate.pt")["e2e"]
    anim = _animator(F32)
    with pytest.raises(RuntimeError, match="set_source"):
        anim.capture(2)
    anim.set_source(g["s"].cuda())
    anim.mfe.train()
    try:
        with pytest.raises(RuntimeError, match=r"eval\(\)"):
            anim.capture(2)
    finally:
        anim.mfe.eval()
    with pytest.raises(ValueError, match="warm-up"):
        anim.capture(2, warmup=0)
    cap = anim.capture(2)
    d = g["d"].cuda()
    for bad in (d[:1], d[:, :, :32], d.half(), torch.zeros(2, 64, 64, 3, dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError, match="captured for"):
            cap(bad)
    two = _animator(F32).set_source(_frames(45, 2))
    with pytest.raises(ValueError, match="source batch"):
        two.capture(3)
