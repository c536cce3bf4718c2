"""GPU parity of the patch-discriminator family: the stride-2 3x3 convolution (forward, data and
weight gradient), instance norm + LeakyReLU, the input assembly, the Discriminator module and the
losses against the reference fixture (tests/golden/discriminator.pt), and the adversarial
training iteration against tests/golden/adv_toy_step.pt.

Tolerances: the kernel cases use the project's own (tests/test_kernels_gpu.py): relative L2 below
1e-5 in fp32 mode (exact-fp32 MFMA) and below 2e-2 * 1.5 in bf16 against the fp32 torch op on the
CPU; the instance-norm backward follows test_bn_act_bwd_pooled.  The module cases in fp32 mode use
the gates of test_toy_training_step_matches_reference_fp32 / test_spectral_norm."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L  # noqa: E402
from facevae_amd import ops  # noqa: E402
from golden_io import load_golden  # noqa: E402

CL = torch.channels_last
TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2 * 1.5}
CANARY = 1024.0          # exact in bf16
GUARD = 4096


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(numel, dtype):
    """(flat buffer of numel + GUARD elements filled with the canary, its first numel elements)"""
    buf = torch.full((numel + GUARD,), CANARY, dtype=dtype, device="cuda")
    return buf, buf[:numel]


# ------------------------------------------------------------------------ stride-2 conv
S2_CASES = [
    # N, cin_valid, cout, H_out, W_out
    (2, 5, 16, 16, 24),      # channel padding 5 -> 8, K = 72 not a multiple of the 32-deep k step
    (2, 18, 64, 8, 8),       # the default first layer's channels, 18 -> 32
    (2, 64, 128, 6, 10),     # P = 120: less than one pixel tile
    (3, 32, 32, 10, 14),     # P = 420: tiles straddle image and sample boundaries
    (1, 128, 256, 4, 4),     # deep K, tiny plane
    (2, 16, 24, 9, 7),       # odd output size, cout not a multiple of 16
]
_S2_REF = {}


def s2_reference(case):
    """fp32 torch reference on the CPU, computed once per case and shared by the three tests."""
    if case not in _S2_REF:
        N, cin, cout, H, W = case
        g = gen(1000 + cin + cout)
        x = torch.randn(N, cin, 2 * H, 2 * W, generator=g).requires_grad_(True)
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).requires_grad_(True)
        b = torch.randn(cout, generator=g).requires_grad_(True)
        dy = torch.randn(N, cout, H, W, generator=g)
        y = F.conv2d(x, w, b, stride=2, padding=1)
        dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
        _S2_REF[case] = tuple(t.detach() for t in (x, w, b, dy, y, dx, dw, db))
    return _S2_REF[case]


def s2_setup(case, dtype, need_wt=False):
    N, cin, cout, H, W = case
    x, w = s2_reference(case)[:2]
    xb, cp = ops.to_nhwc(x.cuda(), dtype)
    ldy = ops.pad_pow2(cout)
    d = ops.desc(dtype, N, H, W, cp, cin, cout, ldy, 3)
    wk = torch.empty(L.query("fv_conv2d_s2_wk_elems", ctypes.byref(d)), dtype=dtype, device="cuda")
    wt = torch.empty(L.query("fv_conv2d_s2_wt_elems", ctypes.byref(d)), dtype=dtype, device="cuda") if need_wt else None
    wc = w.cuda().contiguous()
    L.call("fv_conv2d_s2_weight_prep", ctypes.byref(d), wc.data_ptr(), None, wk.data_ptr(), L.ptr(wt), L.stream())
    return d, xb, cp, ldy, wk, wt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", S2_CASES)
def test_conv_s2_fwd(case, dtype):
    N, cin, cout, H, W = case
    x, w, b, dy, y_ref = s2_reference(case)[:5]
    d, xb, cp, ldy, wk, _ = s2_setup(case, dtype)
    buf, y = guarded(N * H * W * ldy, dtype)
    L.call("fv_conv2d_s2_fwd", ctypes.byref(d), 2 * H, 2 * W, xb.data_ptr(), wk.data_ptr(), b.cuda().data_ptr(),
           y.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert bool((buf[y.numel():] == CANARY).all()), "output written past its end"
    got = y.view(N, H, W, ldy)[..., :cout].permute(0, 3, 1, 2).float()
    r = rel(got, y_ref)
    print(f"s2 fwd {case} {dtype}: rel {r:.3e}")
    assert r < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", S2_CASES)
def test_conv_s2_bwd_data(case, dtype):
    N, cin, cout, H, W = case
    dy, dx_ref = s2_reference(case)[3], s2_reference(case)[5]
    d, xb, cp, ldy, _, wt = s2_setup(case, dtype, need_wt=True)
    dyb, ldd = ops.to_nhwc(dy.cuda(), dtype)          # channel stride pad_pow2(cout), padding 0
    buf, dx = guarded(N * 2 * H * 2 * W * cp, dtype)
    L.call("fv_conv2d_s2_bwd_data", ctypes.byref(d), 2 * H, 2 * W, dyb.data_ptr(), ldd, wt.data_ptr(), dx.data_ptr(),
           L.stream())
    torch.cuda.synchronize()
    assert bool((buf[dx.numel():] == CANARY).all()), "dx written past its end"
    full = dx.view(N, 2 * H, 2 * W, cp)
    assert bool((full[..., cin:] == 0).all()), "padded input channels of dx must be 0"
    r = rel(full[..., :cin].permute(0, 3, 1, 2).float(), dx_ref)
    print(f"s2 dgrad {case} {dtype}: rel {r:.3e}")
    assert r < TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", S2_CASES)
def test_conv_s2_bwd_weight(case, dtype):
    N, cin, cout, H, W = case
    ref = s2_reference(case)
    dy, dw_ref, db_ref = ref[3], ref[6], ref[7]
    d, xb, cp, ldy, _, _ = s2_setup(case, dtype)
    dyb, ldd = ops.to_nhwc(dy.cuda(), dtype)
    slab = torch.empty(L.query("fv_conv2d_s2_wgrad_slab_elems", ctypes.byref(d)), device="cuda")
    bslab = torch.empty(L.query("fv_conv2d_s2_wgrad_bias_slab_elems", ctypes.byref(d)), device="cuda")
    L.call("fv_conv2d_s2_bwd_weight", ctypes.byref(d), 2 * H, 2 * W, xb.data_ptr(), dyb.data_ptr(), ldd, slab.data_ptr(),
           bslab.data_ptr(), L.stream())
    dw = torch.empty(cout, cin, 3, 3, device="cuda")
    db = torch.empty(cout, device="cuda")
    L.call("fv_conv2d_s2_wgrad_reduce", ctypes.byref(d), slab.data_ptr(), bslab.data_ptr(), dw.data_ptr(), db.data_ptr(),
           L.stream())
    torch.cuda.synchronize()
    rw, rb = rel(dw, dw_ref), rel(db, db_ref)
    print(f"s2 wgrad {case} {dtype}: dw {rw:.3e} db {rb:.3e}")
    assert rw < TOL[dtype] and rb < TOL[dtype]


def test_conv_s2_odd_input_is_reported_not_aborted():
    d = ops.desc(torch.float32, 1, 4, 4, 8, 8, 16, 16, 3)
    with pytest.raises(L.FaceVAELibError, match="odd sizes are not supported") as e:
        L.call("fv_conv2d_s2_fwd", ctypes.byref(d), 9, 8, 1, 1, None, 1, L.stream())
    assert f"({L.FV_E_UNSUPPORTED})" in str(e.value)
    with pytest.raises(L.FaceVAELibError, match="odd sizes are not supported"):
        L.call("fv_conv2d_s2_bwd_data", ctypes.byref(d), 8, 7, 1, 16, 1, 1, L.stream())
    with pytest.raises(L.FaceVAELibError, match="odd sizes are not supported"):
        L.call("fv_conv2d_s2_bwd_weight", ctypes.byref(d), 7, 7, 1, 1, 16, 1, None, L.stream())
    blk = fv.ConvBlock2D("CNA", 3, 8, 3, 2, 1, True, "instance", "leakyrelu").cuda().set_compute_dtype(torch.float32)
    with pytest.raises(L.FaceVAELibError, match="odd sizes are not supported"):
        blk(torch.rand(1, 3, 9, 8, device="cuda"))


# ------------------------------------------------------------------------ instance norm
IN_CASES = [
    (2, 16, 16, 24),
    (3, 64, 4, 6),        # a plane of 24 pixels, smaller than a wave
    (2, 512, 4, 4),
    (2, 256, 32, 32),     # a plane split over several blocks
    (1, 8, 2, 64),
]
# forward: fp32 rounding of a handful of operations per element; bf16: the output is rounded once
# to bf16 (relative error <= 2^-9 per element, so relative L2 <= 2^-9 = 1.95e-3), gate at 2x
IN_FWD_TOL = {torch.float32: 1e-5, torch.bfloat16: 4e-3}
IN_BWD_TOL = {torch.float32: (1e-4, 2e-4), torch.bfloat16: (1e-2, 2e-2)}   # (dgamma / dbeta, dx)
_IN_REF = {}


def in_reference(case, dtype):
    """Inputs (rounded to the compute dtype, so the reference sees what the kernel sees) and the
    fp32 torch results on the CPU, once per (case, dtype)."""
    key = (case, dtype)
    if key not in _IN_REF:
        N, C, H, W = case
        g = gen(2000 + C + H)
        scale = 0.5 + 1.5 * torch.rand(N, C, 1, 1, generator=g)          # per plane, in [0.5, 2]
        x = (torch.randn(N, C, H, W, generator=g) * scale).to(dtype).float()
        dout = torch.randn(N, C, H, W, generator=g).to(dtype).float()
        gamma = torch.rand(C, generator=g) + 0.5
        beta = torch.randn(C, generator=g) * 0.1
        xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = F.leaky_relu(F.instance_norm(xr, weight=gr, bias=br, eps=1e-5), 0.2)
        dx, dg, db = torch.autograd.grad(y, (xr, gr, br), dout)
        _IN_REF[key] = (x, dout, gamma, beta, y.detach(), dx, dg, db)
    return _IN_REF[key]


def in_run(x, dout, gamma, beta, dtype):
    xb = x.cuda().to(dtype).contiguous(memory_format=CL)
    gc, bc = gamma.cuda(), beta.cuda()
    z, mean, invstd = ops.in_act_forward(xb, gc, bc, 0.2, 1e-5)
    db_ = dout.cuda().to(dtype).contiguous(memory_format=CL)
    dx, dg, dbt = ops.in_act_backward(db_, xb, mean, invstd, gc, bc, 0.2)
    torch.cuda.synchronize()
    return z, dx, dg, dbt


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", IN_CASES)
def test_instance_norm_act(case, dtype):
    x, dout, gamma, beta, y_ref, dx_ref, dg_ref, db_ref = in_reference(case, dtype)
    z, dx, dg, dbt = in_run(x, dout, gamma, beta, dtype)
    r = (rel(z.float(), y_ref), rel(dx.float(), dx_ref), rel(dg, dg_ref), rel(dbt, db_ref))
    print(f"instance norm {case} {dtype}: y {r[0]:.3e} dx {r[1]:.3e} dgamma {r[2]:.3e} dbeta {r[3]:.3e}")
    tp, tx = IN_BWD_TOL[dtype]
    assert r[0] < IN_FWD_TOL[dtype]
    assert r[1] < tx and r[2] < tp and r[3] < tp
    # bit-reproducible: no atomics in any of the sums
    z2, dx2, dg2, dbt2 = in_run(x, dout, gamma, beta, dtype)
    assert torch.equal(dg, dg2) and torch.equal(dbt, dbt2) and torch.equal(dx, dx2) and torch.equal(z, z2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_instance_norm_samples_are_isolated(dtype):
    case = (2, 16, 16, 24)
    x, dout, gamma, beta = in_reference(case, dtype)[:4]
    z, dx, _, _ = in_run(x, dout, gamma, beta, dtype)
    x2 = x.clone()
    x2[0] *= 100
    z2, dx2, _, _ = in_run(x2, dout, gamma, beta, dtype)
    assert torch.equal(z[1], z2[1]) and torch.equal(dx[1], dx2[1])
    assert not torch.equal(z[0], z2[0])


# ------------------------------------------------------------------------ input assembly
def disc_input_reference(x, kp, K):
    """torch restatement of kp2gaussian_2d + cat (utils.py:79-88, 121-127; models.py:1131-1132)."""
    N, _, H, W = x.shape
    if K == 0:
        return x
    gy = 2 * (torch.arange(H) / (H - 1)) - 1
    gx = 2 * (torch.arange(W) / (W - 1)) - 1
    grid = torch.stack([gx.view(1, W).expand(H, W), gy.view(H, 1).expand(H, W)], 2)      # [..., 0] = width axis
    diff = grid.view(1, 1, H, W, 2) - kp[:, :, :2].view(N, K, 1, 1, 2)
    heat = torch.exp(-0.5 * (diff ** 2).sum(-1) / 0.01)
    return torch.cat([x, heat], 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,K", [((2, 3, 12, 20), 2), ((1, 3, 8, 8), 0)])
def test_disc_input(shape, K, dtype):
    g = gen(31)
    x = torch.rand(shape, generator=g)
    kp = torch.rand(shape[0], K, 3, generator=g) * 2 - 1
    ref = disc_input_reference(x, kp, K)
    out = ops.DiscInputFn.apply(x.cuda(), kp.cuda() if K else None, K, dtype)
    torch.cuda.synchronize()
    cp = ops.pad_pow2(3 + K)
    assert out.shape == (shape[0], cp, shape[2], shape[3]) and out.dtype == dtype and out.is_contiguous(memory_format=CL)
    assert bool((out[:, 3 + K:] == 0).all()), "padding channels must be exactly 0"
    got = out[:, :3 + K].float().cpu()
    if dtype == torch.float32:
        assert (got - ref).abs().max() < 1e-6
    else:
        # one bf16 ulp of the reference value (values in [0, 1]: ulp = 2^-8 * 2^floor(log2 v))
        ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)
        assert bool(((got - ref).abs() <= ulp).all())


# ------------------------------------------------------------------------ module and losses
@pytest.fixture(scope="module")
def gold():
    return load_golden("discriminator.pt")


def run_discriminator(gold, dtype):
    """The fixture's sequence (make_golden_disc.py): D(x_real), D(x_fake), G + 10 F backward;
    then a fresh pair and G1 + G2 backward."""
    D = fv.Discriminator(True, [8, 16, 32, 64], K=2)
    D.load_state_dict(gold["init"])
    D = D.cuda().train().set_compute_dtype(dtype)
    x_real, kp = gold["x_real"].cuda(), gold["kp"].cuda()
    xf = gold["x_fake"].cuda().requires_grad_(True)
    gan, fm = fv.GANLoss(), fv.FeatureMatchingLoss()
    o_r, f_r = D(x_real, kp)
    o_f, f_f = D(xf, kp)
    G, Fm = gan(o_f, True, False), fm(f_f, f_r)
    (G + 10 * Fm).backward()
    res = dict(real=(o_r, f_r), fake=(o_f, f_f), G=G, F=Fm,
               g_grads=dict(x_fake=xf.grad.clone(), **{n: p.grad.clone() for n, p in D.named_parameters()}))
    D.zero_grad(set_to_none=True)
    o_r2, _ = D(x_real, kp)
    o_f2, _ = D(xf.detach(), kp)
    G1, G2 = gan(o_f2, False, True), gan(o_r2, True, True)
    (G1 + G2).backward()
    torch.cuda.synchronize()
    res.update(G1=G1, G2=G2, d_grads={n: p.grad.clone() for n, p in D.named_parameters()},
               uv={k: v for k, v in D.state_dict().items() if k.endswith(("weight_u", "weight_v"))})
    return res


def is_dead_bias(k):
    """a conv bias in front of an instance norm: the norm removes it, its gradient is rounding noise"""
    return k.endswith("layers.0.bias") and not k.startswith("layers.4.")


def test_discriminator_matches_reference_fp32(gold):
    r = run_discriminator(gold, torch.float32)
    for which in ("real", "fake"):
        out, feats = r[which]
        assert out.dtype == torch.float32 and out.shape == gold[which]["output"].shape and out.is_contiguous()
        assert rel(out, gold[which]["output"]) < 1e-4
        assert len(feats) == 4
        for f, fr in zip(feats, gold[which]["features"]):
            assert f.shape == fr.shape and rel(f.float(), fr) < 1e-4
    for k in ("G", "F", "G1", "G2"):
        assert abs(r[k].item() - gold[k].item()) < 1e-4 * abs(gold[k].item()), k
    assert rel(r["g_grads"]["x_fake"], gold["g_grads"]["x_fake"]) < 1e-4
    for name in ("g_grads", "d_grads"):
        for k, gr in gold[name].items():
            if k == "x_fake":
                continue
            if is_dead_bias(k):
                assert (r[name][k].cpu() - gr).abs().max() < 1e-4, (name, k)
            else:
                assert rel(r[name][k], gr) < 1e-3, (name, k)
    assert len(gold["uv"]) == 10
    for k, v in gold["uv"].items():
        assert rel(r["uv"][k], v) < 1e-5, k


def test_conv_block_s2_instance_matches_reference_fp32(gold):
    c = gold["block"]
    blk = fv.ConvBlock2D("CNA", 5, 16, 3, 2, 1, True, "instance", "leakyrelu")
    blk.load_state_dict(c["init"])
    blk = blk.cuda().train().set_compute_dtype(torch.float32)
    x = c["x"].cuda().requires_grad_(True)
    y = blk(x)
    (y.float() * c["g"].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert y.shape == c["out"].shape and rel(y.float(), c["out"]) < 1e-4
    assert rel(x.grad, c["grads"]["x"]) < 1e-4
    for k, p in blk.named_parameters():
        if is_dead_bias(k):
            assert (p.grad.cpu() - c["grads"][k]).abs().max() < 1e-4, k
        else:
            assert rel(p.grad, c["grads"][k]) < 1e-3, k
    for k, v in c["uv"].items():
        assert rel(blk.state_dict()[k], v) < 1e-5, k


# bf16 deviations from the fp32 fixture: deterministic, measured on the MI355X (DESIGN.md, bf16
# gate table): output 7.71e-3, worst feature 8.56e-3, x_fake gradient 1.15e-1, parameter gradients
# median 9.03e-2 / worst 2.39e-1.  Each gate is 2x the measured value, except where that would be
# looser than the existing bf16 step gates (image 1e-2, worst gradient 0.35): those two keep the
# existing gate
BF16_GATES = dict(output=1e-2, feature=1.7e-2, x_grad=0.23, grad_median=0.18, grad_worst=0.35)


def test_discriminator_bf16_deviation(gold):
    r = run_discriminator(gold, torch.bfloat16)
    dev = dict(output=max(rel(r[w][0], gold[w]["output"]) for w in ("real", "fake")),
               feature=max(rel(f.float(), fr) for w in ("real", "fake") for f, fr in zip(r[w][1], gold[w]["features"])),
               x_grad=rel(r["g_grads"]["x_fake"], gold["g_grads"]["x_fake"]))
    gr = sorted(rel(r[name][k], g) for name in ("g_grads", "d_grads") for k, g in gold[name].items()
                if k != "x_fake" and not is_dead_bias(k))
    dev["grad_median"], dev["grad_worst"] = gr[len(gr) // 2], gr[-1]
    print("discriminator bf16 deviation:", {k: f"{v:.3e}" for k, v in dev.items()})
    for k, v in dev.items():
        assert v < BF16_GATES[k], (k, v)


# ------------------------------------------------------------------------ adversarial step
def adv_cfg(w_G, w_F):
    cfg = fv.FaceVAEConfig.toy()
    cfg.w_G, cfg.w_F, cfg.disc_down_seq = w_G, w_F, (8, 16, 32, 64)
    return cfg


def test_adversarial_toy_step_matches_reference_fp32():
    from oracle import facevae_cpu as O      # checker only: the names of the dead conv biases
    g = load_golden("adv_toy_step.pt")
    cfg = adv_cfg(1.0, 10.0)
    tr = fv.FaceVAETrainer(None, None, None, lr=cfg.lr, cfg=cfg, compute_dtype=torch.float32)
    tr.model.load_state_dict(g["init_g"])
    tr.discriminator.load_state_dict(g["init_d"])
    x, eps = g["x"].cuda(), g["eps"].cuda()
    iters = 2
    hist = []
    for it in range(iters):
        out = tr.train_step(x, eps)
        assert list(out) == ["R", "K", "G", "F", "G1", "G2", "y"]
        hist.append(torch.stack([out[k].double().cpu() for k in ("R", "K", "G", "F", "G1", "G2")]))
        if it == 0:
            for k, p in tr.discriminator.named_parameters():
                if is_dead_bias(k):
                    assert (p.grad.cpu() - g["d_grads1"][k]).abs().max() < 1e-4, k
                else:
                    assert rel(p.grad, g["d_grads1"][k]) < 1e-3, k
    torch.cuda.synchronize()
    got = torch.stack(hist)
    print("adversarial losses:", got.tolist(), "reference:", g["losses"].tolist())
    assert torch.allclose(got, g["losses"].double(), rtol=1e-3, atol=0)
    dead_g = {s.prefix + ".bias" for s in O.conv_specs(O.OracleConfig.toy())
              if s.block == "cna" or (s.block == "nac" and ".layers.0.layers.2" in s.prefix)}
    for model, ref, dead in ((tr.model, g["state_g"], lambda k: k in dead_g),
                             (tr.discriminator, g["state_d"], is_dead_bias)):
        sd = model.state_dict()
        assert list(sd) == list(ref)
        for k, v in ref.items():
            if not v.is_floating_point():
                assert torch.equal(sd[k].cpu(), v), k
            elif dead(k):
                assert (sd[k].cpu() - v).abs().max() <= 2 * iters * cfg.lr + 1e-6, k
            else:
                assert rel(sd[k], v) < 1e-3, k


def test_zero_adversarial_weights_is_the_plain_step():
    """w_G = w_F = 0: no discriminator, the output dict has R, K, y only, and one step equals the
    plain iteration (zero_grad, forward, weighted backward, one Adam per model) bit for bit."""
    g = load_golden("adv_toy_step.pt")
    cfg = adv_cfg(0.0, 0.0)
    tr = fv.FaceVAETrainer(None, None, None, lr=cfg.lr, cfg=cfg, compute_dtype=torch.float32)
    assert not tr.adversarial and not hasattr(tr, "discriminator") and tr.d_optimizers == {}
    tr.model.load_state_dict(g["init_g"])
    x, eps = g["x"].cuda(), g["eps"].cuda()
    out = tr.train_step(x, eps)
    assert list(out) == ["R", "K", "y"]

    m = fv.FaceVAE(fv.FaceVAEConfig.toy())
    m.load_state_dict(g["init_g"])
    m = m.cuda().train().set_compute_dtype(torch.float32)
    opts = [fv.Adam(sub.parameters(), lr=cfg.lr, betas=cfg.betas) for sub in (m.afe, m.generator)]
    y, mu, logstd = m(x, eps)
    R, K = fv.ReconLoss()((x, y)), fv.KLDivergenceLoss()((mu, logstd))
    torch.autograd.backward([R, K], [torch.tensor(cfg.w_R, device="cuda"), torch.tensor(cfg.w_K, device="cuda")])
    for o in opts:
        o.step()
    torch.cuda.synchronize()
    assert torch.equal(out["y"], y) and torch.equal(out["R"], cfg.w_R * R.detach()) and torch.equal(out["K"], cfg.w_K * K.detach())
    sd, ref = tr.model.state_dict(), m.state_dict()
    for k in ref:
        assert torch.equal(sd[k], ref[k]), k


def test_adversarial_mode_refuses_graph_capture():
    with pytest.raises(ValueError, match="HIP graph"):
        fv.FaceVAETrainer(None, None, None, lr=5e-5, cfg=adv_cfg(1.0, 0.0), graph=True)


def test_adversarial_checkpoint_round_trip(tmp_path):
    cfg = adv_cfg(1.0, 10.0)
    x = torch.rand(2, 3, 64, 64, generator=gen(5)).cuda()
    eps = torch.randn(2, 16, 32, 32, generator=gen(6)).cuda()
    log = str(tmp_path / "log.txt")
    tr = fv.FaceVAETrainer(str(tmp_path), None, None, lr=cfg.lr, cfg=cfg, compute_dtype=torch.float32, seed=3,
                           log_file_name=log)
    tr.train_step(x, eps)
    tr.save_cpk()
    tr2 = fv.FaceVAETrainer(str(tmp_path), None, None, lr=cfg.lr, cfg=cfg, compute_dtype=torch.float32, seed=4,
                            log_file_name=log)
    assert not torch.equal(tr2.discriminator.state_dict()["layers.0.layers.0.weight_orig"],
                           tr.discriminator.state_dict()["layers.0.layers.0.weight_orig"])
    tr2.load_cpk(0)
    for a, b in ((tr.discriminator, tr2.discriminator), (tr.model, tr2.model)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    oa, ob = tr.d_optimizers["discriminator"].state_dict(), tr2.d_optimizers["discriminator"].state_dict()
    assert oa["param_groups"] == ob["param_groups"] and list(oa["state"]) == list(ob["state"]) and len(oa["state"]) == 18
    for i, st in oa["state"].items():
        for k, v in st.items():
            assert torch.equal(v.cpu(), ob["state"][i][k].cpu()), (i, k)
    # the restored trainer continues exactly as the original
    o1, o2 = tr.train_step(x, eps), tr2.train_step(x, eps)
    torch.cuda.synchronize()
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
