"""GPU parity of the expression feature extractor EFE_conv5.

Gates (DESIGN.md sections 2 and 13, the ones of tests/test_ckd_gpu.py).  fp32-stored results
(everything in fp32 mode; dW, db, dgamma, dbeta, dkpc in both modes): rel-L2 <= 1e-5 against torch
fp64 on the operands the launch read.  bf16-stored results with fp32 accumulation: rel-L2 <= 4e-3
and max |d| <= 1.6e-2 max|ref|.  Blocks and modules in fp32 mode against the reference fixture
(tests/golden/efe.pt): 1e-4 for a block, 1e-3 for the module.  The module in bf16 mode against the
fp32 fixture: 3 x the deviation of the bf16 EMULATION of the reference stored in the fixture for
that quantity (tests/golden/make_golden_efe.py).  The bias of a conv whose output only reaches
shift-invariant consumers (a training-mode batch norm, the softmax) has a mathematically zero
gradient; it is gated in absolute terms against the scale of its conv's weight gradient, as in
tests/test_ckd_gpu.py.

Part 1: the new kernels of csrc/efe.hip (fv_efe_kpcat_fwd / _bwd).
Part 2: ResBlock3D at a padded channel count and SameBlock3D: fp32 against the fixture, bf16 per
launch (every conv and BN launch of the block against torch fp64 on what it read, through the
ops.CHECK hook), and the pad channels, which must stay exactly zero.
Part 3: the existing kernels at shapes only EFE_conv5 brings.
Part 4: the toy EFE_conv5 against the fixture in both train_vae modes, the default EFE_conv5 once
at 256 x 256, the CKD -> transform_kp -> EFE_conv5 -> MFE chain, and ContrastiveLoss_linear.

Every test prints its measured errors (`pytest -s`); DESIGN.md section 14 has the tables.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L, ops, ops3d, ops_efe  # noqa: E402
from golden_io import load_golden  # noqa: E402
from test_ckd_gpu import Launches, gate, maxd, rel, verify_launch  # noqa: E402  (helpers only)
from test_efe_cpu import TOY, perturb_bn  # noqa: E402

CL, CL3 = torch.channels_last, torch.channels_last_3d
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
CKD_TOY = dict(down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3)
MFE_TOY = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)
VAR = 0.01
MIX_OUT_BN = "mix_out.layers.layers.1.weight"

_GOLD = {}


def gold(case):
    if not _GOLD:
        _GOLD.update(load_golden("efe.pt"))
    return _GOLD[case]


def run_captured(fn):
    chk = Launches()
    ops.CHECK = chk
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.CHECK = None
    return out, chk.rows


# ------------------------------------------------------------------ part 1: fv_efe_kpcat_*

def grid32(D, H, W):
    """make_coordinate_grid_3d (utils.py:91-103) in fp32: [D, H, W, 3], (x along W, y along H, z along D)."""
    ax = [2 * (torch.arange(n).float() / (n - 1)) - 1 for n in (D, H, W)]
    zz, yy, xx = torch.meshgrid(*ax, indexing="ij")
    return torch.stack([xx, yy, zz], dim=-1)


def kpcat_ref(z, kpc, G):
    """fp64 on the operands the launch reads: z / G in their storage values, kpc and the grid in fp32."""
    N, K, D, H, W = z.shape
    kp = kpc.double().requires_grad_(True)
    diff = grid32(D, H, W).double().view(1, 1, D, H, W, 3) - kp.view(N, K, 1, 1, 1, 3)
    gauss = torch.exp(-0.5 * (diff ** 2).sum(-1) / float(torch.tensor(VAR, dtype=F32)))
    out = torch.cat([z.double(), gauss], dim=1)
    (out * G.double()).sum().backward()
    return out.detach(), kp.grad


def kpcat_inputs(name, dtype):
    gd = gold("kpcat")[name]
    z = gd["z"].to(dtype)
    N, K = z.shape[:2]
    cp = ops.pad_pow2(2 * K)
    G = torch.zeros(N, cp, *z.shape[2:])
    G[:, :2 * K] = gd["G"]
    # the pad channels of an incoming gradient carry no information; they must not leak anywhere
    G[:, 2 * K:] = 7.0
    return gd, z, gd["kpc"], G.to(dtype)


@DTYPES
@pytest.mark.parametrize("name", ["a", "b", "k1", "k4"])
def test_kpcat_forward(name, dtype):
    gd, z, kpc, G = kpcat_inputs(name, dtype)
    N, K, D, H, W = z.shape
    cp = ops.pad_pow2(2 * K)
    zb = z.cuda().contiguous(memory_format=CL3)
    out = ops_efe.kpcat_forward(zb, kpc.cuda())
    torch.cuda.synchronize()
    assert tuple(out.shape) == (N, cp, D, H, W) and out.dtype == dtype and out.is_contiguous(memory_format=CL3)
    out = out.cpu()
    assert torch.equal(out[:, :K], z)                                   # the logits, bit for bit
    assert (out[:, 2 * K:] == 0).all() and out[:, 2 * K:].numel() == N * (cp - 2 * K) * D * H * W
    ref, _ = kpcat_ref(z, kpc, G[:, :2 * K])
    print(f"\nkpcat fwd {name} {'bf16' if dtype == BF16 else 'fp32'} K={K} Cp={cp}:")
    gate("gaussians vs fp64", out[:, K:2 * K], ref[:, K:], dtype == BF16)
    gate("gaussians vs the reference fixture", out[:, K:2 * K], gd["out"][:, K:], dtype == BF16)
    if name in ("a", "b"):
        assert ref[:, K:].max().item() == 1.0                           # the keypoint that sits on a grid node
        assert kpc.abs().max().item() == 1.5                            # and the one outside the grid


@DTYPES
@pytest.mark.parametrize("name", ["a", "b", "k1", "k4"])
def test_kpcat_backward(name, dtype):
    gd, z, kpc, G = kpcat_inputs(name, dtype)
    N, K, D, H, W = z.shape
    gb = G.cuda().contiguous(memory_format=CL3)
    dz, dkpc = ops_efe.kpcat_backward(gb, kpc.cuda(), K)
    dz2, dkpc2 = ops_efe.kpcat_backward(gb, kpc.cuda(), K)
    torch.cuda.synchronize()
    assert tuple(dz.shape) == (N, K, D, H, W) and dz.dtype == dtype and dz.is_contiguous(memory_format=CL3)
    assert torch.equal(dz.cpu(), G[:, :K])                              # the slice, bit for bit
    assert torch.equal(dz, dz2) and torch.equal(dkpc, dkpc2)            # reruns are bit-identical
    _, ref = kpcat_ref(z, kpc, G[:, :2 * K])
    print(f"\nkpcat bwd {name} {'bf16' if dtype == BF16 else 'fp32'}:")
    gate("dkpc vs fp64", dkpc, ref, False)
    if dtype == F32:
        gate("dkpc vs the reference fixture", dkpc, gd["dkpc"], False)
        gate("dz vs the reference fixture", dz, gd["dz"], False)


@DTYPES
def test_kpcat_autograd(dtype):
    gd, z, kpc, G = kpcat_inputs("a", dtype)
    K = z.shape[1]
    zg = z.cuda().contiguous(memory_format=CL3).requires_grad_(True)
    kg = kpc.cuda().requires_grad_(True)
    out = ops_efe.KpCatFn.apply(zg, kg)
    (out.float() * G.cuda().float()).sum().backward()
    torch.cuda.synchronize()
    _, ref = kpcat_ref(z, kpc, G[:, :2 * K])
    assert torch.equal(zg.grad.cpu(), G[:, :K]) and kg.grad.dtype == F32
    gate("autograd dkpc", kg.grad, ref, False)


@DTYPES
def test_kpcat_backward_many_blocks(dtype):
    """The default EFE_conv5's volume: 482 chunk blocks per sample meet the fixed-order merge."""
    N, K, D, H, W = 1, 15, 16, 64, 64
    g = torch.Generator().manual_seed(401)
    kpc = (torch.rand(N, K, 3, generator=g) - 0.5) * 1.6
    G = torch.randn(N, 32, D, H, W, generator=g).to(dtype)
    z = torch.zeros(N, K, D, H, W)
    assert L.query("fv_efe_kpcat_ws_bytes", N, K, 32, D, H, W) >= 64 * K * 3 * 8       # more chunks than a wave's lanes
    gb = G.cuda().contiguous(memory_format=CL3)
    dz, dkpc = ops_efe.kpcat_backward(gb, kpc.cuda(), K)
    dz2, dkpc2 = ops_efe.kpcat_backward(gb, kpc.cuda(), K)
    torch.cuda.synchronize()
    assert torch.equal(dz, dz2) and torch.equal(dkpc, dkpc2)
    assert torch.equal(dz.cpu(), G[:, :K])
    _, ref = kpcat_ref(z, kpc, G[:, :2 * K])
    print(f"\nkpcat bwd [1, 15, 16, 64, 64] {'bf16' if dtype == BF16 else 'fp32'}:")
    gate("dkpc vs fp64", dkpc, ref, False)
    out = ops_efe.kpcat_forward(z.to(dtype).cuda().contiguous(memory_format=CL3), kpc.cuda())
    outr, _ = kpcat_ref(z, kpc, G[:, :2 * K])
    gate("gaussians vs fp64", out[:, K:2 * K], outr[:, K:], dtype == BF16)
    assert (out[:, 2 * K:] == 0).all() and (out[:, :K] == 0).all()


def test_kpcat_rejects_what_it_cannot_take():
    z = torch.zeros(1, 3, 1, 4, 4, device="cuda").contiguous(memory_format=CL3)
    with pytest.raises(L.FaceVAELibError, match="1002"):
        ops_efe.kpcat_forward(z, torch.zeros(1, 3, 3, device="cuda"))                  # D = 1
    g = torch.zeros(1, 16, 2, 4, 4, device="cuda").contiguous(memory_format=CL3)
    with pytest.raises(L.FaceVAELibError, match="1002"):
        ops_efe.kpcat_backward(g, torch.zeros(1, 3, 3, device="cuda"), 3)              # Cp = 16 for K = 3
    with pytest.raises(ValueError, match="keypoints"):
        ops_efe.KpCatFn.apply(torch.zeros(1, 3, 2, 4, 4, device="cuda"), torch.zeros(1, 4, 3, device="cuda"))


# ------------------------------------------------------------------ part 2: padded ResBlock3D, SameBlock3D

def _n5(t, c=None):
    t = t.detach().cpu().double().contiguous()
    return t if c is None else t[:, :c].contiguous()


def verify_launch3(kind, row, dtype):
    """A captured launch against torch fp64 on the operands it read: the 3x3x3 convs ("fwd3", "bwd3")
    and the BN backward with the residual's addend; everything else is tests/test_ckd_gpu.py's."""
    b16 = dtype == BF16
    if kind in ("fwd3", "bwd3"):
        d = row["d"]
        fast = L.query("fv_conv3d_stats_blocks", ctypes.byref(d)) > 0
        w = (row["w"].to(dtype) if fast else row["w"]).double().cpu()     # the MFMA weight image is bf16
        tag = f"{kind} {d.cin}->{d.cout} {d.d}x{d.h}x{d.w}{' mfma' if fast else ' direct'}"
    if kind == "fwd3":
        y = F.conv3d(_n5(row["x"]), w, row["bias"].double().cpu(), 1, 1)
        if row["res"] is not None:
            y = y + _n5(row["res"])
        gate(tag + (" y+res" if row["res"] is not None else " y"), row["y"], y, b16)
    elif kind == "bwd3":
        x, dy = _n5(row["x"]), _n5(row["dy"])
        gate(tag + " dx", row["dx"], F.conv_transpose3d(dy, w, None, 1, 1), b16)
        gate(tag + " dW", row["dw"], torch.nn.grad.conv3d_weight(x, w.shape, dy, 1, 1), False)
        e = (row["db"].double().cpu() - dy.sum((0, 2, 3, 4))).norm().item() / dy.abs().sum((0, 2, 3, 4)).norm().item()
        print(f"  {tag} db: |d| / sum|dy| {e:.2e} (gate 1e-05)")
        assert e <= 1e-5, (tag, e)
    elif kind in ("fwdg", "bwdg"):
        d = row["d"]
        assert not d.upsample
        w = row["w"].to(dtype).double().cpu()              # the weight image holds the weights in `dtype`
        tag = f"{kind} {d.cin}->{d.cout} k{d.ksize} {d.d}x{d.h}x{d.w}"
        if kind == "fwdg":
            gate(tag + " y", row["y"], F.conv3d(_n5(row["x"]), w, row["bias"].double().cpu(), 1, d.ksize // 2), b16)
        else:
            x, dy = _n5(row["x"]), _n5(row["dy"])
            gate(tag + " dx", row["dx"], F.conv_transpose3d(dy, w, None, 1, d.ksize // 2), b16)
            gate(tag + " dW", row["dw"], torch.nn.grad.conv3d_weight(x, w.shape, dy, 1, d.ksize // 2), False)
            e = (row["db"].double().cpu() - dy.sum((0, 2, 3, 4))).norm().item() / dy.abs().sum((0, 2, 3, 4)).norm().item()
            print(f"  {tag} db: |d| / sum|dy| {e:.2e} (gate 1e-05)")
            assert e <= 1e-5, (tag, e)
    elif kind == "bn_bwd" and row["addend"] is not None:
        y, r = _n5(row["y"]), row["r"]
        C, n = y.shape[1], y.shape[0] * y.shape[2] * y.shape[3]
        assert row["count"] == n and not row["pool"]
        tag = f"bn-bwd+addend {C}ch {y.shape[2]}x{y.shape[3]}"
        v = lambda t: t.double().cpu().view(1, C, 1, 1)       # noqa: E731
        xhat = (y - v(r["mean"])) * v(r["invstd"])
        zz = xhat * v(row["gamma"]) + v(row["beta"])
        da = _n5(row["dout"]) * torch.where(zz > 0, torch.ones_like(zz), torch.full_like(zz, row["slope"]))
        dbeta, dgamma = da.sum((0, 2, 3)), (da * xhat).sum((0, 2, 3))
        dx = v(row["gamma"]) * v(r["invstd"]) * (da - dbeta.view(1, C, 1, 1) / n - xhat * dgamma.view(1, C, 1, 1) / n)
        gate(tag + " dgamma", row["dg"], dgamma, False)
        gate(tag + " dbeta", row["dbt"], dbeta, False)
        gate(tag + " dx", row["dx"], dx + _n5(row["addend"]), b16)
    else:
        verify_launch(kind, row, dtype)


BLOCKS = {"c30_d4": (lambda: fv.ResBlock3D(30, False), 30), "c30_d5": (lambda: fv.ResBlock3D(30, False), 30),
          "c6": (lambda: fv.ResBlock3D(6, False), 6), "same30to15": (lambda: fv.SameBlock3D(30, 15, False), 30)}


def _block(name, mode):
    gd = gold("resblock")[name]
    seed = int(gd["seed"])
    torch.manual_seed(seed)
    blk = BLOCKS[name][0]()
    perturb_bn(blk, seed + 3)
    return gd, blk.cuda().train().set_compute_dtype(mode)


def _dead_bias_block(k):
    """A conv bias in front of a training-mode batch norm has a zero gradient in exact arithmetic:
    the conv of SameBlock3D (C, N, A) and the first conv of a ResBlock3D (N, A, C twice)."""
    return k in ("layers.layers.0.bias", "layers.0.layers.2.bias")


def _dead_bias_module(k):
    """Inside EFE_conv5: the conv of every CNA block (layers.0 in front of its BN); every conv of `mix`
    (layers.2 of an N, A, C block: its output reaches the next batch norm, the residual sum, and
    from there only batch norms and mix_out's 1x1x1 conv in front of a batch norm); out_conv, which
    feeds `mix` the same way."""
    if k.startswith("mix."):
        return k.endswith("layers.2.bias")
    return k.endswith("layers.0.bias") or k == "out_conv.bias"


def _check_param_grads(mod, gd, tol, label, dead, per_key=None):
    named = dict(mod.named_parameters())
    assert set(named) == set(gd)
    over, worst = [], ("", 0.0)
    for k, p in named.items():
        assert p.grad is not None, k
        assert tuple(p.grad.shape) == tuple(gd[k].shape), k           # reference shapes (30-channel weights)
        if dead(k):
            wk = k[:-len("bias")] + "weight"
            lim = (tol if per_key is None else 3 * max(per_key[wk].item(), 2.0 ** -9)) * gd[wk].abs().max().item()
            d = maxd(p.grad, gd[k])
            print(f"    {k}: |d| {d:.2e} (zero-gradient bias, gate {lim:.2e})")
            assert d <= lim, (k, d, lim)
            continue
        e = rel(p.grad, gd[k])
        lim = tol if per_key is None else 3 * per_key[k].item()
        print(f"    {k}: {e:.2e}" + ("" if per_key is None else f" (emulation {per_key[k].item():.2e}, gate {lim:.2e})"))
        if e > worst[1]:
            worst = (k, e)
        if e > lim:
            over.append((k, e, lim))
    print(f"{label}: worst parameter gradient {worst[0]} {worst[1]:.2e}")
    assert not over, over


def _check_buffers(mod, bufs, tol):
    sd = mod.state_dict()
    for k, v in bufs.items():
        if v.is_floating_point():
            assert rel(sd[k], v) < tol, (k, rel(sd[k], v))
        else:
            assert torch.equal(sd[k].cpu(), v), (k, sd[k], v)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_fp32_matches_reference(name):
    gd, blk = _block(name, F32)
    x = gd["x"].cuda().requires_grad_(True)
    out = blk(x)
    (out.float() * gd["g"].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(gd["out"].shape) and tuple(x.grad.shape) == tuple(gd["x"].shape)
    print(f"\n{name} fp32 vs reference: out {rel(out, gd['out']):.2e}  dx {rel(x.grad, gd['dx']):.2e}")
    assert rel(out, gd["out"]) < 1e-4 and rel(x.grad, gd["dx"]) < 1e-4
    _check_param_grads(blk, gd["grads"], 1e-4, name, _dead_bias_block)
    _check_buffers(blk, gd["buffers"], 1e-4)
    blk.eval()
    with torch.no_grad():
        ev = blk(gd["x"].cuda())
    assert rel(ev, gd["out_eval"]) < 1e-4, rel(ev, gd["out_eval"])


@DTYPES
@pytest.mark.parametrize("name", ["c30_d4", "c30_d5", "c6"])
def test_padded_resblock_per_launch(name, dtype):
    """Every launch of the block at its real shapes and data, and the pad channels: the block is fed
    the padded layout (C -> Cp with a zero pad), as inside EFE_conv5.mix."""
    gd, blk = _block(name, dtype)
    C = BLOCKS[name][1]
    cp = ops.pad_pow2(C)
    x = ops3d.pad_channels(gd["x"].to(dtype).cuda().contiguous(memory_format=CL3), cp).requires_grad_(True)
    gy = ops3d.pad_channels(gd["g"].to(dtype).cuda().contiguous(memory_format=CL3), cp)

    def step():
        out = blk(x)
        out.backward(gy)
        return out

    out, rows = run_captured(step)
    kinds = sorted(k for k, _ in rows)
    assert kinds == ["bn_bwd", "bn_bwd", "bn_fwd", "bn_fwd", "bwd3", "bwd3", "fwd3", "fwd3"], kinds
    d = [r for k, r in rows if k == "fwd3"][0]["d"]
    assert (d.cin, d.cout) == (cp, cp)
    fast = L.query("fv_conv3d_stats_blocks", ctypes.byref(d)) > 0
    assert fast == (dtype == BF16 and cp == 32), "c32 in bf16 at W = 64 must take the MFMA kernels"
    print(f"\nResBlock3D({C}) at {cp} channels on {list(gd['x'].shape)} {'bf16' if dtype == BF16 else 'fp32'}, "
          f"per launch:")
    for kind, row in rows:
        verify_launch3(kind, row, dtype)
    # the layout is kept (no pad / cut copies) and the pad channels are exactly zero everywhere
    assert tuple(out.shape) == (x.shape[0], cp) + tuple(x.shape[2:]) and tuple(x.grad.shape) == tuple(x.shape)
    assert out.is_contiguous(memory_format=CL3)
    assert (out[:, C:] == 0).all() and (x.grad[:, C:] == 0).all()
    for kind, row in rows:
        for key in ("y", "out", "dx"):
            t = row.get(key)
            if isinstance(t, torch.Tensor) and t.dim() >= 4 and t.shape[1] == cp:
                assert (t[:, C:] == 0).all(), (kind, key)
    for k, p in blk.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.shape[0] == C, k
    # fed C channels, the same block pads on entry and cuts on exit: the same numbers
    for p in blk.parameters():
        p.grad = None
    x2 = gd["x"].to(dtype).cuda().requires_grad_(True)
    out2 = blk(x2)
    out2.backward(gy[:, :C])
    assert tuple(out2.shape) == tuple(gd["x"].shape) and tuple(x2.grad.shape) == tuple(gd["x"].shape)
    assert torch.equal(out2, out[:, :C]) and torch.equal(x2.grad, x.grad[:, :C])


def test_pow2_channel_counts_run_the_existing_function():
    """A count that is already 8 * 2^k runs ops3d.ResBlock3DFn, as before."""
    blk = fv.ResBlock3D(8, False).cuda().train().set_compute_dtype(F32)
    out = blk(torch.randn(1, 8, 2, 4, 4, device="cuda").requires_grad_(True))
    assert type(out.grad_fn).__name__ == "ResBlock3DFnBackward"
    blk = fv.ResBlock3D(6, False).cuda().train().set_compute_dtype(F32)
    out = blk(torch.randn(1, 6, 2, 4, 4, device="cuda").requires_grad_(True))
    assert out.shape[1] == 6


@DTYPES
def test_same_block_3d_at_efe_shapes(dtype):
    """SameBlock3D(32, 32) on [1, 32, 2, 4, 64] (up's second-to-last block) and SameBlock3D(30, 15) fed
    the 32-channel padded layout (mix_out), against fp64 autograd on the same rounded operands."""
    for cin, cout, feed in ((32, 32, 32), (30, 15, 32)):
        torch.manual_seed(420 + cout)
        blk = fv.SameBlock3D(cin, cout, False)
        perturb_bn(blk, 421)
        g = torch.Generator().manual_seed(422)
        x = torch.randn(1, cin, 2, 4, 64, generator=g).to(dtype).float()
        gz = torch.randn(1, cout, 2, 4, 64, generator=g).to(dtype).float()
        ps = {k: v.detach().double().requires_grad_(True) for k, v in blk.named_parameters()}
        w64 = ps["layers.layers.0.weight"]
        wr = w64 + (w64.detach().to(dtype).double() - w64).detach()
        xx = x.double().requires_grad_(True)
        yb = F.conv3d(xx, wr, ps["layers.layers.0.bias"])
        ref = F.batch_norm(yb, None, None, ps["layers.layers.1.weight"], ps["layers.layers.1.bias"], True, 0.1, 1e-5).relu()
        (ref * gz.double()).sum().backward()
        blk = blk.cuda().train().set_compute_dtype(dtype)
        xg = x.cuda().to(dtype).contiguous(memory_format=CL3)
        if feed != cin:
            xg = ops3d.pad_channels(xg, feed)
        xg.requires_grad_(True)

        def step():
            out = blk(xg)
            (out.float() * gz.cuda()).sum().backward()
            return out

        out, rows = run_captured(step)
        assert sorted(k for k, _ in rows) == ["bn_bwd", "bn_fwd", "bwdg", "fwdg"]
        d = [r for k, r in rows if k == "fwdg"][0]["d"]
        assert (d.cin, d.cout, d.ksize) == (feed, ops.pad_pow2(cout), 1)
        print(f"\nSameBlock3D({cin}, {cout}) fed {feed} channels {'bf16' if dtype == BF16 else 'fp32'}, per launch:")
        for kind, row in rows:
            verify_launch3(kind, row, dtype)
        assert tuple(out.shape) == (1, cout, 2, 4, 64) and tuple(xg.grad.shape) == (1, feed, 2, 4, 64)
        assert (xg.grad[:, cin:] == 0).all()
        named = dict(blk.named_parameters())
        print(f"  block against fp64 autograd: out {rel(out, ref):.2e} dx {rel(xg.grad[:, :cin], xx.grad):.2e} "
              + " ".join(f"{k[-8:]} {rel(named[k].grad, ps[k].grad):.2e}" for k in named if not k.endswith("0.bias")))
        for k in named:
            assert named[k].grad.shape == named[k].shape, k
        if dtype == F32:            # everything is fp32-stored: the block as a whole meets the kernel gate
            assert rel(out, ref) <= 1e-5 and rel(xg.grad[:, :cin], xx.grad) <= 1e-5
            for k in named:
                if not k.endswith("0.bias"):
                    assert rel(named[k].grad, ps[k].grad) <= 1e-5, (k, rel(named[k].grad, ps[k].grad))


# ------------------------------------------------------------------ part 3: existing kernels at new shapes

@DTYPES
def test_same_block_2d_three_valid_channels(dtype):
    """SameBlock2D(3, 32) on [2, 3, 16, 16]: a 1x1 conv with 3 valid of 8 input channels."""
    torch.manual_seed(430)
    blk = fv.SameBlock2D(3, 32, False)
    perturb_bn(blk, 431)
    g = torch.Generator().manual_seed(432)
    x = torch.randn(2, 3, 16, 16, generator=g).to(dtype).float()
    gz = torch.randn(2, 32, 16, 16, generator=g).to(dtype).float()
    blk = blk.cuda().train().set_compute_dtype(dtype)
    xg = x.cuda().requires_grad_(True)

    def step():
        out = blk(xg)
        (out.float() * gz.cuda()).sum().backward()
        return out

    out, rows = run_captured(step)
    kinds = sorted(k for k, _ in rows)
    assert kinds == ["bn_bwd", "bn_fwd", "dgrad", "fwd", "wgrad"], kinds
    d = [r for k, r in rows if k == "fwd"][0]["d"]
    assert (d.cin, d.cin_valid, d.cout, d.ksize) == (8, 3, 32, 1)
    print(f"\nSameBlock2D(3, 32) on [2, 3, 16, 16] {'bf16' if dtype == BF16 else 'fp32'}, per launch:")
    for kind, row in rows:
        verify_launch(kind, row, dtype)
    assert tuple(out.shape) == (2, 32, 16, 16) and tuple(xg.grad.shape) == (2, 3, 16, 16)


@DTYPES
def test_down_block_256_to_32(dtype):
    """DownBlock2D(256, 32) on [1, 256, 8, 8]: the last block of `down`, wide in and narrow out."""
    torch.manual_seed(440)
    blk = fv.DownBlock2D(256, 32, False)
    perturb_bn(blk, 441)
    g = torch.Generator().manual_seed(442)
    x = torch.randn(1, 256, 8, 8, generator=g).to(dtype).float()
    gz = torch.randn(1, 32, 4, 4, generator=g).to(dtype).float()
    blk = blk.cuda().train().set_compute_dtype(dtype)
    xg = x.cuda().requires_grad_(True)

    def step():
        out = blk(xg)
        (out.float() * gz.cuda()).sum().backward()
        return out

    out, rows = run_captured(step)
    assert sorted(k for k, _ in rows) == ["bn_bwd", "bn_fwd", "dgrad", "fwd", "wgrad"]
    print(f"\nDownBlock2D(256, 32) on [1, 256, 8, 8] {'bf16' if dtype == BF16 else 'fp32'}, per launch:")
    for kind, row in rows:
        verify_launch(kind, row, dtype)
    assert tuple(out.shape) == (1, 32, 4, 4) and tuple(xg.grad.shape) == (1, 256, 8, 8)


@DTYPES
def test_mid_conv_16_to_4096(dtype):
    """Conv2d(16, 4096, 1) on [1, 16, 4, 4]: EFE_conv5.mid_conv at the default size."""
    torch.manual_seed(450)
    conv = fv.Conv2d(16, 4096, 1, 1, 0)
    g = torch.Generator().manual_seed(451)
    x = torch.randn(1, 16, 4, 4, generator=g).to(dtype).float()
    gy = torch.randn(1, 4096, 4, 4, generator=g).to(dtype).float()
    conv = conv.cuda().train()
    conv._dtype = dtype
    xg = x.cuda().requires_grad_(True)

    def step():
        y = conv(xg)
        (y.float() * gy.cuda()).sum().backward()
        return y

    y, rows = run_captured(step)
    assert sorted(k for k, _ in rows) == ["dgrad", "fwd", "wgrad"]
    print(f"\nConv2d(16, 4096, 1) on [1, 16, 4, 4] {'bf16' if dtype == BF16 else 'fp32'}, per launch:")
    for kind, row in rows:
        verify_launch(kind, row, dtype)
    w = conv.weight.detach().to(dtype).double().cpu()
    gate("module dx", xg.grad, F.conv_transpose2d(gy.double(), w), dtype == BF16)
    gate("module db", conv.bias.grad, gy.double().sum((0, 2, 3)), False)


# ------------------------------------------------------------------ part 4: the module

def _run_efe(mode, case, with_kl=True):
    gd = gold("efe")
    gc = gd[case]
    train_vae = True if case == "train_vae" else None
    torch.manual_seed(int(gd["seed"]))
    net = fv.EFE_conv5(False, **TOY)
    with torch.no_grad():
        dict(net.named_parameters())[MIX_OUT_BN].mul_(0.1)
    net = net.cuda().train().set_compute_dtype(mode)
    x, x_a = gd["x"].cuda().requires_grad_(True), gd["x_a"].cuda()
    kpc = gd["kpc"].cuda().requires_grad_(True)
    kp, x_c, x_a_c, (mu, ls), (x_vae, x_hat) = net(x, x_a, kpc, train_vae, gc["eps"].cuda())
    loss = (kp * gd["g"].cuda()).sum()
    if train_vae:
        kl = fv.KLDivergenceLoss()((mu, ls))
        loss = loss + kl
    loss.backward()
    torch.cuda.synchronize()
    assert x.grad is None                     # the image is data: no gradient
    assert kp.dtype == F32 and tuple(kp.shape) == (2, TOY["K"], 3)
    outs = dict(kp=kp, x_c=x_c, x_a_c=x_a_c, x_vae=x_vae, x_hat=x_hat)
    if train_vae:
        outs.update(mu=mu, logstd=ls)
        assert tuple(mu.shape) == (2, 256) and tuple(ls.shape) == (2, 256) and mu.dtype == F32
    else:
        assert mu is None and ls is None
    for k, v in outs.items():
        assert tuple(v.shape) == tuple(gc["out"][k].shape), (k, v.shape)
    return gd, gc, net, outs, kpc.grad


@pytest.mark.parametrize("case", ["no_vae", "train_vae"])
def test_efe_fp32_matches_reference(case):
    gd, gc, net, outs, dkpc = _run_efe(F32, case)
    print(f"\nEFE_conv5 fp32 [{case}] vs reference: " + "  ".join(f"{k} {rel(v, gc['out'][k]):.2e}" for k, v in outs.items())
          + f"  dkpc {rel(dkpc, gc['dkpc']):.2e}")
    for k, v in outs.items():
        assert rel(v, gc["out"][k]) < 1e-3, (k, rel(v, gc["out"][k]))
    assert rel(dkpc, gc["dkpc"]) < 1e-3
    _check_param_grads(net, gc["grads"], 1e-3, f"EFE_conv5 fp32 [{case}]", _dead_bias_module)
    _check_buffers(net, gc["buffers"], 1e-3)
    sd = net.state_dict()
    assert int(sd["down.0.layers.layers.1.num_batches_tracked"]) == 2           # `down` ran for x and for x_a
    assert int(sd["mix_out.layers.layers.1.num_batches_tracked"]) == 1
    net.eval()
    with torch.no_grad():
        ev = net(gd["x"].cuda(), None, gd["kpc"].cuda(), None)
    assert ev[1] is None and ev[2] is None and ev[3] == (None, None)
    ee = rel(ev[0], gc["kp_eval"])
    print(f"EFE_conv5 fp32 [{case}] eval-mode kp rel-L2 {ee:.2e}")
    assert ee < 1e-3


@pytest.mark.parametrize("case", ["no_vae", "train_vae"])
def test_efe_bf16_vs_fp32_reference(case):
    gd, gc, net, outs, dkpc = _run_efe(BF16, case)
    dev = gc["emu_dev"]
    print(f"\nEFE_conv5 bf16 [{case}] vs fp32 reference (gate = 3 x the bf16 emulation of the reference):")
    for k, v in outs.items():
        e, lim = rel(v, gc["out"][k]), 3 * dev["out"][k].item()
        print(f"  {k}: rel-L2 {e:.2e} (emulation {dev['out'][k].item():.2e}, gate {lim:.2e})")
        assert e <= lim, (k, e, lim)
    e, lim = rel(dkpc, gc["dkpc"]), 3 * dev["dkpc"].item()
    print(f"  dkpc: rel-L2 {e:.2e} (emulation {dev['dkpc'].item():.2e}, gate {lim:.2e})")
    assert e <= lim, (e, lim)
    _check_param_grads(net, gc["grads"], None, f"EFE_conv5 bf16 [{case}]", _dead_bias_module, per_key=dev["grads"])


def test_kl_reuses_the_reparameterisation_pass():
    """KLDivergenceLoss on the returned (x_mu, x_logstd) takes the value the VAE pass reduced, and
    equals the loss computed from the tensors themselves."""
    gd = gold("efe")
    torch.manual_seed(int(gd["seed"]))
    net = fv.EFE_conv5(False, **TOY).cuda().train().set_compute_dtype(F32)
    out = net(gd["x"].cuda(), None, gd["kpc"].cuda(), True, gd["train_vae"]["eps"].cuda())
    mu, ls = out[3]
    assert getattr(mu, "_fv_kl", None) is not None and mu._fv_kl[0] is ls
    kl = fv.KLDivergenceLoss()((mu, ls))
    ref = (-0.5 - ls.double() + 0.5 * mu.double() ** 2 + 0.5 * torch.exp(2 * ls.double())).mean()
    assert abs(kl.item() - ref.item()) <= 1e-5 * abs(ref.item()), (kl.item(), ref.item())
    assert out[1] is None and out[2] is None


def test_efe_fp8_mode_runs_in_bf16():
    gd = gold("efe")
    outs = []
    for mode in (BF16, torch.float8_e4m3fn):
        torch.manual_seed(int(gd["seed"]))
        net = fv.EFE_conv5(False, **TOY).cuda().train().set_compute_dtype(mode)
        kp = net(gd["x"].cuda(), None, gd["kpc"].cuda())[0]
        (kp * gd["g"].cuda()).sum().backward()
        outs.append((kp.detach(), net.out_conv.weight.grad.clone(), net.mix[0].conv1.weight.grad.clone()))
        assert net.compute_dtype() == mode and net.mid_conv._dtype == mode       # the mode is put back
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_default_efe_once_at_256():
    torch.manual_seed(21)
    net = fv.EFE_conv5().cuda().train().set_compute_dtype(BF16)
    g = torch.Generator().manual_seed(22)
    x, x_a = torch.rand(1, 3, 256, 256, generator=g).cuda(), torch.rand(1, 3, 256, 256, generator=g).cuda()
    kpc = ((torch.rand(1, 15, 3, generator=g) - 0.5) * 1.2).cuda().requires_grad_(True)
    gk = torch.randn(1, 15, 3, generator=g).cuda()
    eps = torch.randn(1, 16, 4, 4, generator=g).cuda()
    torch.cuda.reset_peak_memory_stats()
    runs = []
    for _ in range(2):
        for p in net.parameters():
            p.grad = None
        kpc.grad = None
        kp, x_c, x_a_c, (mu, ls), (x_vae, x_hat) = net(x, x_a, kpc, True, eps)
        ((kp * gk).sum() + fv.KLDivergenceLoss()((mu, ls))).backward()
        torch.cuda.synchronize()
        runs.append((kp.detach().clone(), kpc.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters()}))
    kp, dkpc, grads = runs[0]
    assert tuple(kp.shape) == (1, 15, 3) and kp.dtype == F32
    assert tuple(x_c.shape) == (1, 32, 4, 4) and tuple(x_a_c.shape) == (1, 32, 4, 4) and tuple(mu.shape) == (1, 256)
    assert torch.isfinite(kp).all() and kp.abs().max().item() <= 1.0 and torch.isfinite(dkpc).all()
    assert all(torch.isfinite(t.float()).all() for t in (x_c, x_a_c, mu, ls, x_vae, x_hat))
    bad = [k for k, v in grads.items() if not torch.isfinite(v).all()]
    assert not bad, bad
    assert len(grads) == len(list(net.parameters())) and grads["mid_conv.weight"].abs().sum().item() > 0
    assert grads["mix.0.layers.0.layers.2.weight"].shape == (30, 30, 3, 3, 3) and dkpc.abs().sum().item() > 0
    # a second forward + backward from the same parameters: bit-identical
    assert torch.equal(kp, runs[1][0]) and torch.equal(dkpc, runs[1][1])
    diff = [k for k in grads if not torch.equal(grads[k], runs[1][2][k])]
    assert not diff, diff
    print(f"\ndefault EFE_conv5 bf16 at 256 x 256 with x_a: kp range [{kp.min().item():.3f}, {kp.max().item():.3f}], "
          f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")


def test_ckd_transform_kp_efe_mfe_compose():
    """image -> CKD -> transform_kp (seeded pose) -> EFE_conv5 -> MFE: a loss on the MFE's outputs
    reaches CKD.out_conv through dkpc (trainer.py:290-308)."""
    torch.manual_seed(31)
    ckd = fv.CKD(False, **CKD_TOY).cuda().train()
    efe = fv.EFE_conv5(False, **TOY).cuda().train()
    mfe = fv.MFE(False, **MFE_TOY).cuda().train()
    g = torch.Generator().manual_seed(32)
    img = torch.rand(2, 3, 64, 64, generator=g).cuda()
    fs = torch.randn(2, 8, 4, 8, 8, generator=g).cuda()
    pose = lambda: [((torch.rand(2, generator=g) - 0.5) * 0.6).cuda() for _ in range(3)] + [   # noqa: E731
        (torch.randn(2, 3, generator=g) * 0.05).cuda(), (1 + 0.1 * torch.randn(2, 1, 1, 1, generator=g)).cuda()]
    kp_c = ckd(img)
    kp_s_old, Rs = fv.transform_kp(kp_c, *pose())
    kp_d_old, Rd = fv.transform_kp(kp_c, *pose())
    kp_s = efe(img, None, kp_s_old)[0]
    kp_d = efe(img, None, kp_d_old)[0]
    # the loss reads only what EFE_conv5 made of the posed keypoints: the one path to CKD is dkpc
    deformation, occlusion, mask = mfe(fs, kp_s, kp_d, Rs.detach(), Rd.detach())
    assert all(torch.isfinite(o).all() for o in (deformation, occlusion, mask, kp_s, kp_d))
    (deformation.sum() + occlusion.sum() + (mask * torch.randn(mask.shape, generator=g).cuda()).sum()).backward()
    torch.cuda.synchronize()
    gw = ckd.out_conv.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and gw.abs().sum().item() > 0
    ge = efe.mix[0].conv1.weight.grad
    assert ge is not None and torch.isfinite(ge).all() and ge.abs().sum().item() > 0


@pytest.mark.parametrize("mode", ["direction", "non-direction"])
def test_contrastive_loss_on_the_gpu(mode):
    gd = gold("contrastive")[mode.replace("-", "_")]
    seed = int(gd["seed"])
    torch.manual_seed(seed)
    crit = fv.ContrastiveLoss_linear(mode=mode).train()
    perturb_bn(crit, seed + 3)
    crit = crit.cuda()
    f1 = gd["f1"].cuda().contiguous(memory_format=CL).requires_grad_(True)
    f2 = gd["f2"].cuda().contiguous(memory_format=CL).requires_grad_(True)
    loss = crit(f1, f2)
    loss.backward()
    assert rel(loss, gd["loss"]) < 1e-4 and rel(f1.grad, gd["d_f1"]) < 1e-4 and rel(f2.grad, gd["d_f2"]) < 1e-4
    named = dict(crit.named_parameters())
    for k, ref in gd["grads"].items():
        got = named[k].grad[::16] if named[k].grad.dim() == 2 else named[k].grad
        assert rel(got, ref) < 1e-4, (k, rel(got, ref))
