"""GPU parity of the canonical keypoint detector.

Part 0: the EXISTING kernels at CKD's shapes, none of which another test covers -- DownBlock2D with
3 valid of 8 input channels and at 512 -> 1024 on a 4 x 4 plane, the 1024 -> 16384 1x1 `mid_conv` on
4 pixels, fv_depth_split at C = 1024 / D = 16 and C = 32 / D = 4, and the general 3-D conv with an
odd cout (15 and 3).  Every launch of a block (convolution forward, data and weight gradient, BN
statistics, BN apply and BN backward) is compared with torch in fp64 on the CPU on the operands
that launch read, captured at the block's real shapes through the ops.CHECK hook.

Kernel gates (tests/test_mfe_gpu.py, tests/test_hpe_gpu.py).  fp32-stored results (everything in
fp32 mode; dW, db, dgamma, dbeta, the BN statistics of fp32 data, and kp in both modes): rel-L2
<= 1e-5.  bf16-stored results with fp32 accumulation: rel-L2 <= 4e-3 and max |d| <= 1.6e-2
max|ref|.  In bf16 mode the BN statistics come from the conv's fp32 outputs before they are
rounded, while the test sees the rounded tensor: mean within 2^-9 max|y| and invstd within 4e-3
relative, the rounding of one bf16 element.

Part 1: the new kernels of csrc/ckd.hip.  Resize against the reference fixture (fp32, 1e-6; bf16 =
the rounded fp32 result, bit for bit); soft-argmax against the fixture and against torch fp64 on
the same rounded logits (kp 1e-5; dz 1e-5 fp32, 4e-3 bf16-stored).

Part 2: the toy CKD against the reference fixture (tests/golden/ckd.pt).  fp32 mode: < 1e-3
relative on kp, parameter gradients, running statistics and the eval-mode kp (the project's parity
bar).  The bias of a conv in front of a training-mode BatchNorm, and out_conv.bias in front of the
shift-invariant softmax, have mathematically zero gradients (the reference's values are round-off
noise), so they are gated in absolute terms against the scale of their conv's weight gradient, as
in tests/test_hpe_gpu.py (in bf16 mode with the factor 3 x max(the emulation's deviation of that
weight gradient, 2^-9)).  bf16 mode against the fp32 fixture: each gate is 3 x the deviation of
the bf16 EMULATION of the reference stored in the fixture for that quantity
(tests/golden/make_golden_ckd.py).  Then the default CKD() once at 256 x 256 and the CKD ->
transform_kp -> MFE chain.

Every test prints its measured errors (`pytest -s`); DESIGN.md section 13 has the tables.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L, ops, ops3d, ops_ckd  # noqa: E402
from golden_io import load_golden  # noqa: E402

CL, CL3 = torch.channels_last, torch.channels_last_3d
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
TOY = dict(down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3)
MFE_TOY = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)
GUARD, SENT = 4096, 0xA5
T = 0.1


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def maxd(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def gate(name, got, ref, stored_bf16, lim32=1e-5):
    """The kernel gates of the module docstring; prints the measured error."""
    assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
    e = rel(got, ref)
    lim = 4e-3 if stored_bf16 else lim32
    print(f"  {name}: rel-L2 {e:.2e} (gate {lim:.0e})", end="")
    assert e <= lim, (name, e, lim)
    if stored_bf16:
        m, top = maxd(got, ref), ref.abs().max().item()
        print(f"  max|d| {m:.2e} (gate {1.6e-2 * top:.2e})", end="")
        assert m <= 1.6e-2 * top, (name, m, top)
    print()


class Guarded:
    """Caller-sized buffers with a sentinel region behind them (tests/test_buffers_gpu.py)."""

    def __init__(self):
        self.bufs = []

    def __call__(self, n, dtype, device="cuda"):
        n = int(n)
        es = torch.empty(0, dtype=dtype).element_size()
        raw = torch.full((n * es + GUARD,), SENT, dtype=torch.uint8, device=device)
        self.bufs.append((raw, n * es))
        return raw[:n * es].view(dtype)

    def check(self):
        torch.cuda.synchronize()
        bad = [(i, nb) for i, (raw, nb) in enumerate(self.bufs) if not bool((raw[nb:] == SENT).all())]
        return len(self.bufs), bad


# ------------------------------------------------------------------ part 0: per-launch checks

def _c(t):
    return None if t is None else t.detach().clone()


class Launches:
    """ops.CHECK hook: keeps the operands and results of every conv / BN launch of a block."""

    def __init__(self):
        self.rows = []

    def __call__(self, kind, owner, **kw):
        row = {k: (_c(v) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        if kind.startswith("bn"):
            r = kw["r"]
            row["r"] = {n: _c(getattr(r, n)) for n in ("mean", "invstd", "scale", "shift")}
            row["count"] = r.count
            row["gamma"], row["beta"], row["eps"] = _c(owner.weight), _c(owner.bias), owner.eps
        else:
            row["w"], row["d"] = _c(owner.w), owner.d
        self.rows.append((kind, row))


def _nchw64(t, c=None):
    """NHWC (or any) device tensor -> NCHW fp64 on the CPU, first c channels."""
    t = t.detach().cpu().double().contiguous()
    return t if c is None else t[:, :c].contiguous()


def _act64(v, slope):
    return torch.maximum(v, v * slope)


def verify_launch(kind, row, dtype):
    """One captured launch against torch fp64 on the operands it read."""
    b16 = dtype == BF16
    if kind in ("fwd", "dgrad", "wgrad"):
        d = row["d"]
        w = row["w"].to(dtype).double().cpu()          # the weight image holds the weights in `dtype`
        k, pad = d.ksize, d.ksize // 2
        tag = f"{kind} {d.cin_valid}->{d.cout} k{k} {d.h}x{d.w}"
    if kind == "fwd":
        assert row["pro"] is None and row["res"] is None and not d.upsample
        x = _nchw64(row["x"], d.cin_valid)
        bias = row["bias"].double().cpu() if row["bias"] is not None else None
        gate(tag + " y", row["y"], F.conv2d(x, w, bias, 1, pad), b16 and row["y"].dtype == BF16)
    elif kind == "dgrad":
        dy = _nchw64(row["dy"], d.cout)
        dx = F.conv_transpose2d(dy, w, None, 1, pad)
        gate(tag + " dx", row["dx"][:, :d.cin_valid], dx, b16)
    elif kind == "wgrad":
        x, dy = _nchw64(row["x"], d.cin_valid), _nchw64(row["dy"], d.cout)
        dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, 1, pad)
        gate(tag + " dW", row["dw"], dw, False)
        if row["db"] is not None:
            # a sum that may cancel to zero (a conv in front of a BN): its error is measured against
            # the sum of the magnitudes, the scale a summation error is relative to
            e = (row["db"].double().cpu() - dy.sum((0, 2, 3))).norm().item() / dy.abs().sum((0, 2, 3)).norm().item()
            print(f"  {tag} db: |d| / sum|dy| {e:.2e} (gate 1e-05)")
            assert e <= 1e-5, (tag, e)
    elif kind == "bn_fwd":
        y, r = _nchw64(row["y"]), row["r"]
        C = y.shape[1]
        tag = f"bn {C}ch {y.shape[2]}x{y.shape[3]}"
        if row["count"]:                               # training mode: the statistics themselves
            mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
            invstd = (var + row["eps"]).rsqrt()
            if b16:
                dm, top = maxd(r["mean"], mean), y.abs().max().item()
                ei = ((r["invstd"].double().cpu() - invstd) / invstd).abs().max().item()
                print(f"  {tag} mean |d| {dm:.2e} (gate {2.0 ** -9 * top:.2e})  invstd {ei:.2e} (gate 4e-3)")
                assert dm <= 2.0 ** -9 * top and ei <= 4e-3
            else:
                gate(tag + " mean", r["mean"], mean, False)
                gate(tag + " invstd", r["invstd"], invstd, False)
            g, b = row["gamma"].double().cpu(), row["beta"].double().cpu()
            rm, ri = r["mean"].double().cpu(), r["invstd"].double().cpu()
            gate(tag + " scale", r["scale"], g * ri, False)
            gate(tag + " shift", r["shift"], b - rm * g * ri, False)
        sc, sh = r["scale"].double().cpu().view(1, C, 1, 1), r["shift"].double().cpu().view(1, C, 1, 1)
        out = _act64(y * sc + sh, row["slope"])
        if row["pool"]:
            out = F.avg_pool2d(out, 2)
        gate(tag + " out", row["out"], out, b16)
    elif kind == "bn_bwd":
        assert row["addend"] is None
        y, r = _nchw64(row["y"]), row["r"]
        C, n = y.shape[1], y.shape[0] * y.shape[2] * y.shape[3]
        assert row["count"] == n
        tag = f"bn-bwd {C}ch {y.shape[2]}x{y.shape[3]}"
        v = lambda t: t.double().cpu().view(1, C, 1, 1)       # noqa: E731
        xhat = (y - v(r["mean"])) * v(r["invstd"])
        z = xhat * v(row["gamma"]) + v(row["beta"])
        g = _nchw64(row["dout"])
        if row["pool"]:
            g = F.interpolate(g, scale_factor=2, mode="nearest") / 4
        da = g * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, row["slope"]))
        dbeta, dgamma = da.sum((0, 2, 3)), (da * xhat).sum((0, 2, 3))
        dx = v(row["gamma"]) * v(r["invstd"]) * (da - dbeta.view(1, C, 1, 1) / n - xhat * dgamma.view(1, C, 1, 1) / n)
        gate(tag + " dgamma", row["dg"], dgamma, False)
        gate(tag + " dbeta", row["dbt"], dbeta, False)
        gate(tag + " dx", row["dx"], dx, b16)
    else:
        raise AssertionError(f"unexpected launch kind {kind}")


def run_captured(fn):
    chk = Launches()
    ops.CHECK = chk
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.CHECK = None
    return out, chk.rows


DOWN_CASES = {"3to8_pad": (3, 8, (2, 3, 16, 24)), "512to1024_deep": (512, 1024, (1, 512, 4, 4))}


@DTYPES
@pytest.mark.parametrize("name", list(DOWN_CASES))
def test_down_block_at_ckd_shapes(name, dtype):
    cin, cout, shape = DOWN_CASES[name]
    torch.manual_seed(300 + cin)
    blk = fv.DownBlock2D(cin, cout, False)
    cb = blk.layers[0]
    with torch.no_grad():
        cb.bn.weight.uniform_(0.5, 1.5)
        cb.bn.bias.normal_(0, 0.5)
    g = torch.Generator().manual_seed(301 + cin)
    x = torch.randn(*shape, generator=g).to(dtype).float()
    gz = torch.randn(shape[0], cout, shape[2] // 2, shape[3] // 2, generator=g).to(dtype).float()
    # block-level fp64 reference on the same rounded x and weights
    ps = {k: v.detach().double().requires_grad_(True) for k, v in blk.named_parameters()}
    w64 = ps["layers.0.layers.0.weight"]
    wr = (w64 + (w64.detach().to(dtype).double() - w64).detach())
    xx = x.double().requires_grad_(True)
    yb = F.conv2d(xx, wr, ps["layers.0.layers.0.bias"], 1, 1)
    zb = F.batch_norm(yb, None, None, ps["layers.0.layers.1.weight"], ps["layers.0.layers.1.bias"], True, 0.1, 1e-5)
    ref = F.avg_pool2d(zb.relu(), 2)
    (ref * gz.double()).sum().backward()

    blk = blk.cuda().train().set_compute_dtype(dtype)
    xg = x.cuda().requires_grad_(True)

    def step():
        out = blk(xg)
        (out.float() * gz.cuda()).sum().backward()
        return out

    out, rows = run_captured(step)
    kinds = sorted(k for k, _ in rows)
    assert kinds == ["bn_bwd", "bn_fwd", "dgrad", "fwd", "wgrad"], kinds
    print(f"\nDownBlock2D({cin}, {cout}) on {list(shape)} {'bf16' if dtype == BF16 else 'fp32'}, per launch:")
    for kind, row in rows:
        verify_launch(kind, row, dtype)
    assert tuple(out.shape) == tuple(ref.shape) and xg.grad is not None and tuple(xg.grad.shape) == shape
    named = dict(blk.named_parameters())
    ends = {"out": (out, ref), "dx": (xg.grad, xx.grad)}
    ends.update({k: (named[k].grad, ps[k].grad) for k in named if not k.endswith("layers.0.bias")})
    print("  block against fp64 autograd: " + "  ".join(f"{k.replace('layers.0.layers.', 'L')} {rel(a, b):.2e}"
                                                         for k, (a, b) in ends.items()))
    if dtype == F32:            # everything is fp32-stored: the block as a whole meets the kernel gate
        for k, (a, b) in ends.items():
            assert rel(a, b) <= 1e-5, (k, rel(a, b))


@DTYPES
def test_mid_conv_1024_to_16384_on_four_pixels(dtype, monkeypatch):
    cin, cout = 1024, 16384
    torch.manual_seed(310)
    conv = fv.Conv2d(cin, cout, 1, 1, 0)
    g = torch.Generator().manual_seed(311)
    x = torch.randn(1, cin, 2, 2, generator=g).to(dtype).float()
    gy = torch.randn(1, cout, 2, 2, generator=g).to(dtype).float()
    guard = Guarded()
    monkeypatch.setattr(ops, "_empty", guard)
    # the weight images hold every row and column a tile may read: at least the dense matrix, and the
    # launches below pass the kernels' own extent guard (FV_E_BADARG otherwise)
    d = ops.desc(ops.storage(dtype), 1, 2, 2, cin, cin, cout, cout, 1)
    wk, wt = L.query("fv_conv_wk_elems", ctypes.byref(d)), L.query("fv_conv_wt_elems", ctypes.byref(d))
    assert wk >= cin * cout and wt >= cin * cout, (wk, wt)
    conv = conv.cuda().train()
    conv._dtype = dtype
    xg = x.cuda().requires_grad_(True)

    def step():
        y = conv(xg)
        (y.float() * gy.cuda()).sum().backward()
        return y

    y, rows = run_captured(step)
    assert sorted(k for k, _ in rows) == ["dgrad", "fwd", "wgrad"]
    assert tuple(y.shape) == (1, cout, 2, 2) and y.dtype == ops.storage(dtype)
    print(f"\nConv2d(1024, 16384, 1) on [1, 1024, 2, 2] {'bf16' if dtype == BF16 else 'fp32'} "
          f"(weight images {wk} / {wt} elements):")
    for kind, row in rows:
        verify_launch(kind, row, dtype)
    # the module's results are those launches' (every one of the 16384 channels was compared above)
    w = conv.weight.detach().to(dtype).double().cpu()
    gate("module dx", xg.grad, F.conv_transpose2d(gy.double(), w), dtype == BF16)
    gate("module dW", conv.weight.grad, torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double()), False)
    gate("module db", conv.bias.grad, gy.double().sum((0, 2, 3)), False)
    n, bad = guard.check()
    assert n >= 3 and not bad, f"{len(bad)} of {n} buffers written past their queried size: {bad[:8]}"


@DTYPES
@pytest.mark.parametrize("geo", [(1, 1024, 16, 2, 2), (2, 32, 4, 2, 3)], ids=["c1024_d16_2x2", "c32_d4_2x3"])
def test_depth_split_is_a_view(geo, dtype):
    N, C, D, H, W = geo
    g = torch.Generator().manual_seed(320)
    h = torch.randn(N, C * D, H, W, generator=g).to(dtype)
    gv = torch.randn(N, C, D, H, W, generator=g).to(dtype)
    hg = h.cuda().contiguous(memory_format=CL).requires_grad_(True)
    v = ops3d.depth_split(hg, C, D, dtype)
    assert tuple(v.shape) == (N, C, D, H, W) and v.dtype == dtype and v.is_contiguous(memory_format=CL3)
    assert torch.equal(v.detach().cpu(), h.view(N, C, D, H, W))
    v.backward(gv.cuda())
    torch.cuda.synchronize()
    assert torch.equal(hg.grad.cpu(), gv.view(N, C * D, H, W))
    m = ops3d.depth_merge(v.detach(), dtype)                   # the inverse direction as a forward
    assert torch.equal(m.cpu(), h)


# (N, cin, cout, D, H, W, ksize): an odd cout -> element stores, 30-byte bf16 rows, and a data
# gradient that gathers from a dy with 15 or 3 channels
C3_CASES = {"32to15": (1, 32, 15, 4, 8, 8, 3), "8to3": (2, 8, 3, 4, 8, 12, 3)}


@DTYPES
@pytest.mark.parametrize("name", list(C3_CASES))
def test_conv3dg_odd_cout(name, dtype):
    N, cin, cout, D, H, W, k = C3_CASES[name]
    g = torch.Generator().manual_seed(330 + cout)
    x = torch.randn(N, cin, D, H, W, generator=g).to(dtype).float()
    w = (torch.randn(cout, cin, k, k, k, generator=g) / math.sqrt(cin * k ** 3)).to(dtype).float()
    b = torch.randn(cout, generator=g)
    gy = torch.randn(N, cout, D, H, W, generator=g).to(dtype).float()
    xx, ww, bb = (t.double().requires_grad_(True) for t in (x, w, b))
    ry = F.conv3d(xx, ww, bb, 1, k // 2)
    (ry * gy.double()).sum().backward()
    d = ops3d.descg(dtype, N, D, H, W, cin, cout, k, False)
    cs = ops3d.Conv3dgState(w.cuda().contiguous(), d, "cuda", True)
    xb = x.cuda().to(dtype).contiguous(memory_format=CL3)
    gyb = gy.cuda().to(dtype).contiguous(memory_format=CL3)
    y = ops3d.conv3dg_forward(cs, xb, b.cuda())
    dx, dw, db = ops3d.conv3dg_backward(cs, xb, gyb)
    torch.cuda.synchronize()
    print(f"\nconv3dg {name} {'bf16' if dtype == BF16 else 'fp32'} (K fwd {27 * cin}, dgrad {27 * cout}):")
    gate("y", y, ry.detach(), dtype == BF16)
    gate("dx", dx, xx.grad, dtype == BF16)
    gate("dW", dw, ww.grad, False)
    gate("db", db, bb.grad, False)


# ------------------------------------------------------------------ part 1: the new kernels

_GOLD = {}


def gold(case):
    if not _GOLD:
        _GOLD.update(load_golden("ckd.pt"))
    return _GOLD[case]


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_resize_matches_reference(case):
    gd = gold("resize")[case]
    x, s = gd["x"].cuda(), float(gd["scale"])
    y32 = ops_ckd.ResizeFn.apply(x, s, F32)
    y16 = ops_ckd.ResizeFn.apply(x, s, BF16)
    torch.cuda.synchronize()
    N, _, Ho, Wo = gd["y"].shape
    for y, dt in ((y32, F32), (y16, BF16)):
        assert tuple(y.shape) == (N, 8, Ho, Wo) and y.dtype == dt and y.is_contiguous(memory_format=CL)
        assert not y.requires_grad
        assert bool((y[:, 3:] == 0).all())                         # the padded channels are exactly zero
    e = rel(y32[:, :3], gd["y"])
    print(f"\nresize {list(gd['x'].shape)} x {s}: fp32 rel-L2 {e:.2e} (gate 1e-6), max|d| {maxd(y32[:, :3], gd['y']):.2e}")
    assert e <= 1e-6
    assert torch.equal(y16, y32.to(BF16))                          # bf16 = the rounded fp32 result
    # to_nhwc passes the tensor through: no copy in front of the first conv
    for y, dt in ((y32, F32), (y16, BF16)):
        buf, cp = ops.to_nhwc(y, dt)
        assert cp == 8 and buf.data_ptr() == y.data_ptr()


def test_resize_default_is_the_centre_mean():
    """256 -> 64 at scale exactly 4: every output is the mean of the centre 2 x 2 of its 4 x 4 cell."""
    x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(340))
    y = ops_ckd.ResizeFn.apply(x.cuda(), 0.25, F32)[:, :3].cpu()
    c = x.view(1, 3, 64, 4, 64, 4)[:, :, :, 1:3, :, 1:3]
    want = 0.5 * (0.5 * c[:, :, :, 0, :, 0] + 0.5 * c[:, :, :, 0, :, 1]) + 0.5 * (0.5 * c[:, :, :, 1, :, 0] + 0.5 * c[:, :, :, 1, :, 1])
    assert torch.equal(y, want)


def sam_ref(z, G):
    """heatmap2kp(out2heatmap(z)) and dz in fp64 on the CPU; z [N, K, D, H, W], G [N, K, 3]."""
    z = z.detach().double().cpu().requires_grad_(True)
    N, K, D, H, W = z.shape
    p = torch.softmax(z.reshape(N, K, -1) / T, dim=2).view(N, K, D, H, W)
    lin = lambda n: 2 * (torch.arange(n, dtype=F64) / (n - 1)) - 1         # noqa: E731
    kp = torch.stack([(p * lin(W).view(1, 1, 1, 1, W)).sum((2, 3, 4)), (p * lin(H).view(1, 1, 1, H, 1)).sum((2, 3, 4)),
                      (p * lin(D).view(1, 1, D, 1, 1)).sum((2, 3, 4))], dim=2)
    (kp * G.double().cpu()).sum().backward()
    return kp.detach(), z.grad


def sam_run(z, G, dtype):
    """z logical [N, K, D, H, W] on the CPU -> (kp, dz) of the kernels with `dtype` storage."""
    zb = z.to(dtype).cuda().contiguous(memory_format=CL3).requires_grad_(True)
    kp = ops_ckd.SoftArgmaxFn.apply(zb, T)
    kp.backward(G.cuda())
    torch.cuda.synchronize()
    assert kp.dtype == F32 and zb.grad.dtype == dtype and zb.grad.shape == zb.shape
    return kp.detach(), zb.grad


def _sam_logits(name):
    g = torch.Generator().manual_seed(350)
    if name in ("fixture_a", "fixture_b"):
        gd = gold("softargmax")[name[-1]]
        return gd["z"], gd["G"]
    shape = {"k1": (2, 1, 3, 4, 5), "offset300": (1, 15, 2, 5, 7), "default_late_peak": (2, 15, 16, 64, 64)}[name]
    z = torch.randn(shape, generator=g)
    if name == "offset300":
        z = z + 300
    if name == "default_late_peak":
        # one voxel per keypoint raised by 8 in the last chunk: the running maximum changes after
        # most of the mass has been summed
        V = shape[2] * shape[3] * shape[4]
        zf = z.view(shape[0], shape[1], V)
        for n in range(shape[0]):
            for k in range(shape[1]):
                zf[n, k, V - 1 - 37 * k - n] += 8
    return z, torch.randn(shape[0], shape[1], 3, generator=g)


SAM_CASES = ["fixture_a", "fixture_b", "k1", "offset300", "default_late_peak"]
_SAM_REF = {}


def _sam_reference(name, dtype):
    key = (name, dtype)
    if key not in _SAM_REF:
        z, G = _sam_logits(name)
        _SAM_REF[key] = (z, G) + sam_ref(z.to(dtype).float(), G)
    return _SAM_REF[key]


@DTYPES
@pytest.mark.parametrize("name", SAM_CASES)
def test_softargmax_vs_fp64(name, dtype):
    z, G, rkp, rdz = _sam_reference(name, dtype)
    kp, dz = sam_run(z, G, dtype)
    print(f"\nsoft-argmax {name} {list(z.shape)} {'bf16' if dtype == BF16 else 'fp32'}:")
    assert torch.isfinite(kp).all() and torch.isfinite(dz).all()
    assert kp.abs().max().item() <= 1.0
    gate("kp", kp, rkp, False)
    gate("dz", dz, rdz, dtype == BF16)
    if name.startswith("fixture") and dtype == F32:           # the reference's own fp32 result
        gd = gold("softargmax")[name[-1]]
        gate("kp vs fixture", kp, gd["kp"], False)
        gate("dz vs fixture", dz, gd["dz"], False)
    # the softmax is invariant to a per-keypoint shift: the gradient sums to zero over the voxels
    # measured against (2 / T) sum_j |G_j|, the bound of sum_v |dz| (|grid - kp| <= 2, sum p = 1): fp32
    # 1e-5; bf16 2^-8, one rounding of 2^-9 per stored element, all aligned at worst, times 2
    s = (dz.double().cpu().sum((2, 3, 4)).abs() / (2 / T * G.double().abs().sum(2))).max().item()
    assert s <= (2.0 ** -8 if dtype == BF16 else 1e-5), s


@DTYPES
def test_softargmax_is_bit_reproducible(dtype):
    z, G = _sam_logits("default_late_peak")
    kp1, dz1 = sam_run(z, G, dtype)
    kp2, dz2 = sam_run(z, G, dtype)
    assert torch.equal(kp1, kp2) and torch.equal(dz1, dz2)


def test_softargmax_rejects_what_it_cannot_take():
    U = L.FV_E_UNSUPPORTED
    buf = torch.zeros(1 << 16, device="cuda")
    p, s = L.ptr(buf), L.stream()
    for dc in (L.FV_F32, L.FV_BF16):
        for (k, d, h, w) in ((3, 1, 8, 8), (3, 4, 1, 8), (3, 4, 8, 1), (257, 2, 2, 2), (0, 2, 2, 2)):
            assert L.query("fv_ckd_softargmax_ws_bytes", 1, k, d, h, w) == 0
            assert L.query("fv_ckd_softargmax_fwd", dc, p, 1, k, d, h, w, T, p, p, p, s) == U, (k, d, h, w)
            assert L.query("fv_ckd_softargmax_bwd", dc, p, p, p, 1, k, d, h, w, T, p, s) == U, (k, d, h, w)
        assert L.query("fv_ckd_softargmax_fwd", dc, p, 1, 3, 2, 2, 2, 0.0, p, p, p, s) == U
        assert L.query("fv_ckd_resize_fwd", dc, p, 1, 8, 8, 0, 2, p, s) == U
    assert L.query("fv_ckd_softargmax_fwd", L.FV_F64, p, 1, 3, 2, 2, 2, T, p, p, p, s) == U
    with pytest.raises(L.FaceVAELibError, match="at least 2"):
        ops_ckd.SoftArgmaxFn.apply(torch.zeros(1, 3, 1, 8, 8, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ part 2: the module

def _dead_bias(k):
    """Bias of a conv directly in front of a training-mode BN (layers.0 of every block), and
    out_conv.bias in front of the shift-invariant softmax: zero gradient in exact arithmetic."""
    return k.endswith("layers.0.bias") or k == "out_conv.bias"


def _check_param_grads(mod, gd, tol, label, per_key=None):
    worst = ("", 0.0)
    named = dict(mod.named_parameters())
    assert set(named) == set(gd)
    over = []
    for k, p in named.items():
        assert p.grad is not None, k
        if _dead_bias(k):
            wk = k[:-len("bias")] + "weight"
            # bf16 mode: the conv's output gradient is stored in bf16, 2^-9 relative rounding per element
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


def _run_ckd(mode):
    gd = gold("ckd")
    torch.manual_seed(int(gd["seed"]))
    net = fv.CKD(False, **TOY).cuda().train().set_compute_dtype(mode)
    x = gd["x"].cuda().requires_grad_(True)
    kp = net(x)
    (kp * gd["g"].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert x.grad is None                     # the image is data: no gradient
    assert tuple(kp.shape) == tuple(gd["out"].shape) and kp.dtype == F32
    return gd, net, kp


def test_ckd_fp32_matches_reference():
    gd, net, kp = _run_ckd(F32)
    e = rel(kp, gd["out"])
    print(f"\nCKD fp32 vs reference: kp rel-L2 {e:.2e}")
    assert e < 1e-3
    _check_param_grads(net, gd["grads"], 1e-3, "CKD fp32")
    sd = net.state_dict()
    for k, v in gd["buffers"].items():
        if v.is_floating_point():
            assert rel(sd[k], v) < 1e-3, (k, rel(sd[k], v))
        else:
            assert torch.equal(sd[k].cpu(), v), k
    net.eval()
    with torch.no_grad():
        ev = net(gd["x"].cuda())
    ee = rel(ev, gd["out_eval"])
    print(f"CKD fp32 eval-mode kp rel-L2 {ee:.2e}")
    assert ee < 1e-3


def test_ckd_bf16_vs_fp32_reference():
    gd, net, kp = _run_ckd(BF16)
    dev = gd["emu_dev"]
    e, lim = rel(kp, gd["out"]), 3 * dev["out"]["kp"].item()
    print(f"\nCKD bf16 vs fp32 reference (gate = 3 x the bf16 emulation of the reference):\n"
          f"  kp: rel-L2 {e:.2e} (emulation {dev['out']['kp'].item():.2e}, gate {lim:.2e})")
    assert e <= lim, (e, lim)
    _check_param_grads(net, gd["grads"], None, "CKD bf16", per_key=dev["grads"])


def test_ckd_fp8_mode_runs_in_bf16():
    gd = gold("ckd")
    outs = []
    for mode in (BF16, torch.float8_e4m3fn):
        torch.manual_seed(int(gd["seed"]))
        net = fv.CKD(False, **TOY).cuda().train().set_compute_dtype(mode)
        kp = net(gd["x"].cuda())
        (kp * gd["g"].cuda()).sum().backward()
        outs.append((kp.detach(), net.out_conv.weight.grad.clone(), net.down[0].layers[0].conv.weight.grad.clone()))
        assert net.compute_dtype() == mode and net.mid_conv._dtype == mode       # the mode is put back
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_ckd_workspaces_stay_in_bounds(monkeypatch):
    """Every caller-sized buffer on the module path: weight images, BN records, weight-gradient slabs
    and workspaces of the existing entries, and the soft-argmax partials."""
    guard = Guarded()
    monkeypatch.setattr(ops, "_empty", guard)
    gd = gold("ckd")
    for mode in (F32, BF16):
        torch.manual_seed(3)
        net = fv.CKD(False, **TOY).cuda().train().set_compute_dtype(mode)
        net(gd["x"].cuda()).sum().backward()
    z, G = _sam_logits("fixture_b")
    sam_run(z, G, BF16)
    n, bad = guard.check()
    assert n > 20, n
    assert not bad, f"{len(bad)} of {n} buffers written past their queried size: {bad[:8]}"


def test_default_ckd_once_at_256():
    torch.manual_seed(11)
    net = fv.CKD().cuda().train().set_compute_dtype(BF16)
    x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(12)).cuda()
    g = torch.randn(1, 15, 3, generator=torch.Generator().manual_seed(13)).cuda()
    runs = []
    for _ in range(2):
        for p in net.parameters():
            p.grad = None
        kp = net(x)
        (kp * g).sum().backward()
        torch.cuda.synchronize()
        runs.append((kp.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()}))
    kp, grads = runs[0]
    assert tuple(kp.shape) == (1, 15, 3) and kp.dtype == F32
    assert torch.isfinite(kp).all() and kp.abs().max().item() <= 1.0
    bad = [k for k, v in grads.items() if not torch.isfinite(v).all()]
    assert not bad, bad
    assert len(grads) == len(list(net.parameters())) and grads["mid_conv.weight"].abs().sum().item() > 0
    # a second forward + backward from the same parameters: bit-identical
    assert torch.equal(kp, runs[1][0])
    diff = [k for k in grads if not torch.equal(grads[k], runs[1][1][k])]
    assert not diff, diff
    print(f"\ndefault CKD bf16 at 256 x 256: kp range [{kp.min().item():.3f}, {kp.max().item():.3f}], "
          f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")


def test_ckd_transform_kp_mfe_compose():
    """image -> CKD -> transform_kp (seeded pose) -> MFE: a loss on the MFE's outputs reaches CKD.out_conv."""
    torch.manual_seed(7)
    ckd = fv.CKD(False, **TOY).cuda().train()
    mfe = fv.MFE(False, **MFE_TOY).cuda().train()
    g = torch.Generator().manual_seed(8)
    img = torch.rand(2, 3, 64, 96, generator=g).cuda()
    fs = torch.randn(2, 8, 4, 8, 8, generator=g).cuda()
    pose = lambda: [((torch.rand(2, generator=g) - 0.5) * 0.6).cuda() for _ in range(3)] + [   # noqa: E731
        (torch.randn(2, 3, generator=g) * 0.05).cuda(), (1 + 0.1 * torch.randn(2, 1, 1, 1, generator=g)).cuda()]
    kp_c = ckd(img)
    assert tuple(kp_c.shape) == (2, 3, 3) and kp_c.dtype == F32
    kp_s, Rs = fv.transform_kp(kp_c, *pose())
    kp_d, Rd = fv.transform_kp(kp_c, *pose())
    deformation, occlusion, mask = mfe(fs, kp_s, kp_d, Rs, Rd)
    assert all(torch.isfinite(o).all() for o in (deformation, occlusion, mask, kp_s, kp_d))
    (deformation.sum() + occlusion.sum() + (mask * torch.randn(mask.shape, generator=g).cuda()).sum()).backward()
    torch.cuda.synchronize()
    gw = ckd.out_conv.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and gw.abs().sum().item() > 0
    gd0 = ckd.down[0].layers[0].conv.weight.grad
    assert gd0 is not None and torch.isfinite(gd0).all()
