"""GPU parity of the head pose estimator: the kernels of csrc/pose.hip (7x7 stride-2 stem, 3x3
stride-2 max pool, subsample, bottleneck join, pose head) against torch in fp64 on the CPU on the
same dtype-rounded operands, the stem / ResBottleneck / HPE_EDE modules against the reference
fixtures (tests/golden/hpe.pt), and the HPE_EDE -> transform_kp -> MFE composition.

Kernel gates.  fp32-stored results (everything in fp32 mode; dW, db, the BN records and the pose
head's fp32 outputs in both modes, the bf16 operands being exact in fp32): rel-L2 <= 1e-5.
bf16-stored outputs with fp32 accumulation: rel-L2 <= 4e-3 and max |d| <= 1.6e-2 max|ref| (the
gates of tests/test_mfe_gpu.py).  The max pool is bit-equal to torch's (values and argmax).

Modules and model in fp32 mode: < 1e-3 relative on outputs, input gradients, parameter gradients
and running statistics (the project's parity bar); the three angles are centre-subtracted and can
sit near zero, so they are gated by absolute error <= 1e-3 x the angle range n_bins * 3 pi / 180.
The bias of a conv in front of a training-mode BatchNorm has a mathematically zero gradient (the
reference's value is round-off noise), so it is gated in absolute terms against the scale of its
conv's weight gradient, as in tests/test_mfe_gpu.py (in bf16 mode with the factor 3 x max(the
emulation's deviation of that weight gradient, 2^-9): its summands are bf16-stored gradients).

bf16 mode against the fp32 fixture: each gate is 3 x the deviation of the bf16 EMULATION of the
reference stored in the fixture for that key (tests/golden/make_golden_hpe.py; the emulation
covers forward rounding only, the factor allows for bf16-stored gradients and differing rounding
points).  Every test prints its measured errors (`pytest -s`); DESIGN.md section 12 has the tables.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L, ops, ops_pose  # noqa: E402
from golden_io import load_golden  # noqa: E402

CL = torch.channels_last
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
TOY = dict(n_filters=[16, 32, 64], n_blocks=[1, 1], n_bins=6, K=3)
MFE_TOY = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)
GUARD, SENT = 4096, 0xA5


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def maxd(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def gate(name, got, ref, dtype, stored_bf16):
    """The kernel gates of the module docstring; prints the measured error."""
    e = rel(got, ref)
    lim = 4e-3 if (dtype == BF16 and stored_bf16) else 1e-5
    print(f"  {name}: rel-L2 {e:.2e} (gate {lim:.0e})", end="")
    assert e <= lim, (name, e, lim)
    if dtype == BF16 and stored_bf16:
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


def nhwc(t, dtype):
    return t.cuda().to(dtype).contiguous(memory_format=CL)


# ------------------------------------------------------------------ stem

STEM_CASES = {"2x32x48_c16": (2, 32, 48, 16), "1x64x64_c64": (1, 64, 64, 64), "3x20x36_c24_ragged": (3, 20, 36, 24)}


def _stem_operands(name, dtype):
    N, H, W, cout = STEM_CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(STEM_CASES).index(name))
    x = torch.randn(N, 3, H, W, generator=g).to(dtype).float()
    w = (torch.randn(cout, 3, 7, 7, generator=g) / math.sqrt(147)).to(dtype).float()
    b = torch.randn(cout, generator=g)
    gy = torch.randn(N, cout, H // 2, W // 2, generator=g).to(dtype).float()
    return x, w, b, gy


_STEM_REF = {}


def _stem_ref(name, dtype):
    if (name, dtype) not in _STEM_REF:
        x, w, b, gy = _stem_operands(name, dtype)
        ww, bb = w.double().requires_grad_(True), b.double().requires_grad_(True)
        y = F.conv2d(x.double(), ww, bb, 2, 3)
        (y * gy.double()).sum().backward()
        _STEM_REF[(name, dtype)] = (y.detach(), ww.grad, bb.grad)
    return _STEM_REF[(name, dtype)]


def _stem_run(name, dtype, alloc):
    N, H, W, cout = STEM_CASES[name]
    x, w, b, gy = _stem_operands(name, dtype)
    dc = L.dtype_code(dtype)
    xd, wd, bd = x.cuda().contiguous(), w.cuda().contiguous(), b.cuda()
    wk = alloc(L.query("fv_stem7s2_wk_elems", cout), dtype)
    L.call("fv_stem7s2_weight_prep", dc, L.ptr(wd), cout, L.ptr(wk), L.stream())
    nb, bp = L.query("fv_stem7s2_stats_blocks", N, H, W), L.query("fv_stem7s2_stats_block_pixels")
    assert nb * bp >= N * (H // 2) * (W // 2) > (nb - 1) * bp
    stats = alloc(nb * 2 * cout, F32)
    y = torch.empty((N, cout, H // 2, W // 2), dtype=dtype, device="cuda", memory_format=CL)
    L.call("fv_stem7s2_fwd", dc, L.ptr(xd), N, H, W, cout, L.ptr(wk), L.ptr(bd), L.ptr(y), L.ptr(stats), L.stream())
    gyb = nhwc(gy, dtype)
    ws = alloc(L.query("fv_stem7s2_wgrad_ws_bytes", N, H, W, cout) // 4, F32)
    dw = torch.empty(cout, 3, 7, 7, device="cuda")
    db = torch.empty(cout, device="cuda")

    def wgrad():
        L.call("fv_stem7s2_bwd_weight", dc, L.ptr(xd), L.ptr(gyb), N, H, W, cout, L.ptr(dw), L.ptr(db), L.ptr(ws),
               L.stream())
        torch.cuda.synchronize()
        return dw.clone(), db.clone()

    dw1, db1 = wgrad()
    return y, stats.view(nb, 2, cout), dw1, db1, wgrad


@DTYPES
@pytest.mark.parametrize("name", list(STEM_CASES))
def test_stem_kernels_vs_torch_fp64(name, dtype):
    g = Guarded()
    ry, rdw, rdb = _stem_ref(name, dtype)
    y, stats, dw, db, wgrad = _stem_run(name, dtype, g)
    print(f"\nstem {name} {'bf16' if dtype == BF16 else 'fp32'}:")
    assert y.shape == ry.shape
    gate("y", y.float(), ry, dtype, True)
    gate("dw", dw, rdw, dtype, False)
    gate("db", db, rdb, dtype, False)
    # the BN records hold the fp32 outputs before the rounding to the storage dtype
    gate("record sums", stats[:, 0].double().sum(0), ry.sum((0, 2, 3)), dtype, False)
    gate("record squares", stats[:, 1].double().sum(0), ry.square().sum((0, 2, 3)), dtype, False)
    dw2, db2 = wgrad()
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "weight gradient reruns differ"
    n, bad = g.check()
    assert n == 3 and not bad, bad


def test_unsupported_descriptors_return_unsupported():
    U = L.FV_E_UNSUPPORTED
    for dc in (L.FV_F32, L.FV_BF16):
        for (h, w, cout) in ((31, 48, 16), (32, 47, 16), (32, 48, 12), (32, 48, 20)):
            assert L.query("fv_stem7s2_fwd", dc, None, 1, h, w, cout, None, None, None, None, None) == U
            assert L.query("fv_stem7s2_bwd_weight", dc, None, None, 1, h, w, cout, None, None, None, None) == U
        assert L.query("fv_stem7s2_weight_prep", dc, None, 12, None, None) == U
        for (h, w, c) in ((7, 8, 16), (8, 9, 16), (8, 8, 12)):
            assert L.query("fv_maxpool3s2_fwd", dc, None, 1, h, w, c, None, None, 0.0, None, None, None) == U
            assert L.query("fv_maxpool3s2_bwd", dc, None, None, 1, h, w, c, None, None) == U
            assert L.query("fv_subsample2_fwd", dc, None, 1, h, w, c, None, None) == U
            assert L.query("fv_subsample2_bwd", dc, None, 1, h, w, c, None, None) == U
        assert L.query("fv_bn2_add_relu_fwd", dc, None, None, None, None, None, None, 10, 12, None, None) == U
        assert L.query("fv_pose_pool_fwd", dc, None, 2, 6, 12, None, None) == U
        assert L.query("fv_pose_head_bwd", dc, None, None, None, 2, 6, 12, 6, None, None, None, None, None, None) == U
    assert L.query("fv_pose_head_fwd", None, 2, 12, 6, None, None, None, None, None) == U
    assert b"multiple of 8" in L.load().fv_last_error()
    assert L.query("fv_stem7s2_wk_elems", 12) == 0 and L.query("fv_stem7s2_stats_blocks", 1, 31, 48) == 0
    assert L.query("fv_stem7s2_wgrad_ws_bytes", 1, 32, 48, 12) == 0


# ------------------------------------------------------------------ max pool, subsample

POOL_SHAPES = {"2x8x12_c16": (2, 8, 12, 16), "1x6x10_c24": (1, 6, 10, 24)}


def _pool_input(kind, shape, dtype):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(31)
    if kind == "relu":
        x = torch.randn(N, C, H, W, generator=g).relu()       # half the elements are 0: tied windows
    elif kind == "negative":
        x = -torch.rand(N, C, H, W, generator=g) - 0.1        # padding must behave as -inf, not 0
    else:
        x = torch.full((N, C, H, W), 1.5)                     # every window is a tie
    return x.to(dtype).float()


def _tap_to_flat(am, H, W):
    """uint8 taps [N, Ho, Wo, C] -> torch's flat input-plane indices [N, C, Ho, Wo]."""
    N, Ho, Wo, C = am.shape
    t = am.long()
    oy = torch.arange(Ho, device=am.device).view(1, Ho, 1, 1)
    ox = torch.arange(Wo, device=am.device).view(1, 1, Wo, 1)
    iy, ix = 2 * oy - 1 + t // 3, 2 * ox - 1 + t % 3
    assert (t <= 8).all() and (iy >= 0).all() and (iy < H).all() and (ix >= 0).all() and (ix < W).all()
    return (iy * W + ix).permute(0, 3, 1, 2)


def _pool_run(xb, pro=None, slope=0.0, alloc=None):
    N, C, H, W = xb.shape
    y = torch.empty((N, C, H // 2, W // 2), dtype=xb.dtype, device="cuda", memory_format=CL)
    am = (alloc or Guarded())(N * (H // 2) * (W // 2) * C, torch.uint8)
    sc, sh = pro if pro is not None else (None, None)
    L.call("fv_maxpool3s2_fwd", L.dtype_code(xb.dtype), L.ptr(xb), N, H, W, C, L.ptr(sc), L.ptr(sh), float(slope),
           L.ptr(y), L.ptr(am), L.stream())
    torch.cuda.synchronize()
    return y, am.view(N, H // 2, W // 2, C)


@DTYPES
@pytest.mark.parametrize("kind", ["relu", "negative", "constant"])
@pytest.mark.parametrize("shape", list(POOL_SHAPES))
def test_maxpool_bit_equal_to_torch(shape, kind, dtype):
    N, H, W, C = POOL_SHAPES[shape]
    x = _pool_input(kind, POOL_SHAPES[shape], dtype)
    ry, ridx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    g = Guarded()
    y, am = _pool_run(nhwc(x, dtype), alloc=g)
    assert torch.equal(y.float().cpu(), ry), "values differ from torch"
    assert torch.equal(_tap_to_flat(am, H, W).cpu(), ridx), "argmax differs from torch (tie rule)"
    n, bad = g.check()
    assert n == 1 and not bad
    # backward: a gather, against an fp64 scatter of the output gradient to torch's indices
    gy = torch.randn(ry.shape, generator=torch.Generator().manual_seed(32)).to(dtype).float()
    ref = torch.zeros(N, C, H * W, dtype=torch.float64)
    ref.scatter_add_(2, ridx.view(N, C, -1), gy.double().view(N, C, -1))
    dx = torch.full((N, C, H, W), float("nan"), device="cuda").to(dtype).contiguous(memory_format=CL)
    L.call("fv_maxpool3s2_bwd", L.dtype_code(dtype), L.ptr(nhwc(gy, dtype)), L.ptr(am), N, H, W, C, L.ptr(dx),
           L.stream())
    torch.cuda.synchronize()
    assert not torch.isnan(dx).any(), "an element of dx was not written"
    print(f"\nmax pool {shape} {kind} {'bf16' if dtype == BF16 else 'fp32'}:")
    gate("dx", dx.float(), ref.view(N, C, H, W), dtype, True)


@DTYPES
def test_maxpool_propagates_nan(dtype):
    x = _pool_input("relu", (1, 8, 12, 16), dtype)
    x[0, 3, 2, 5] = float("nan")
    x[0, 7, 7, 11] = float("nan")
    ry, ridx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    y, am = _pool_run(nhwc(x, dtype))
    yc = y.float().cpu()
    assert torch.equal(torch.isnan(yc), torch.isnan(ry)) and torch.isnan(ry).sum() >= 2
    assert torch.equal(torch.nan_to_num(yc, 7.0), torch.nan_to_num(ry, 7.0))
    assert torch.equal(_tap_to_flat(am, 8, 12).cpu(), ridx)


class _Affine:
    def __init__(self, scale, shift):
        self.scale, self.shift = scale, shift


@DTYPES
@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_maxpool_prologue_equals_bn_act_then_pool(dtype, slope):
    N, H, W, C = 2, 8, 12, 16
    g = torch.Generator().manual_seed(33)
    xb = nhwc(torch.randn(N, C, H, W, generator=g), dtype)
    r = _Affine((torch.randn(C, generator=g)).cuda(), torch.randn(C, generator=g).cuda())   # both signs of scale
    act = ops.bn_act_forward(xb, r, slope, False)
    y2, am2 = _pool_run(act)
    y1, am1 = _pool_run(xb, (r.scale, r.shift), slope)
    assert torch.equal(y1, y2), "prologue values differ from fv_bn_act_fwd + pool"
    assert torch.equal(am1, am2)
    flat = _tap_to_flat(am1, H, W)                                      # [N, C, Ho, Wo]
    at = act.float().reshape(N, C, H * W).gather(2, flat.reshape(N, C, -1)).view_as(y1)
    assert torch.equal(at, y1.float()), "the element at the recorded argmax is not the stored maximum"


@DTYPES
def test_subsample_round_trip(dtype):
    N, H, W, C = 2, 6, 10, 24
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(34)).to(dtype)
    xb = nhwc(x, dtype)
    y = ops_pose.subsample_forward(xb)
    assert torch.equal(y.cpu(), x[:, :, ::2, ::2])
    dx = torch.full((N, C, H, W), float("nan"), device="cuda").to(dtype).contiguous(memory_format=CL)
    L.call("fv_subsample2_bwd", L.dtype_code(dtype), L.ptr(y), N, H, W, C, L.ptr(dx), L.stream())
    want = torch.zeros_like(x)
    want[:, :, ::2, ::2] = x[:, :, ::2, ::2]
    assert torch.equal(dx.cpu(), want)


# ------------------------------------------------------------------ join

@DTYPES
@pytest.mark.parametrize("second_affine", [True, False])
def test_join_vs_fp64(dtype, second_affine):
    N, H, W, C = 2, 8, 12, 24
    g = torch.Generator().manual_seed(35)
    ya, yb = (torch.randn(N, C, H, W, generator=g).to(dtype).float() for _ in range(2))
    sa, ha, sb, hb = (torch.randn(C, generator=g) for _ in range(4))
    v = lambda t: t.double().view(1, C, 1, 1)     # noqa: E731
    ref = (ya.double() * v(sa) + v(ha) + (yb.double() * v(sb) + v(hb) if second_affine else yb.double())).relu()
    out = ops_pose.join_forward(nhwc(ya, dtype), _Affine(sa.cuda(), ha.cuda()), nhwc(yb, dtype),
                                _Affine(sb.cuda(), hb.cuda()) if second_affine else None)
    torch.cuda.synchronize()
    print(f"\njoin {'bf16' if dtype == BF16 else 'fp32'} second_affine={second_affine}:")
    gate("out", out.float(), ref, dtype, True)
    # the backward's ReLU mask comes from `out` itself (fv_relu_bwd) and the sum of the branch gradients from fv_add2
    gy = nhwc(torch.randn(N, C, H, W, generator=g), dtype)
    d = ops_pose.relu_backward(gy, out)
    assert torch.equal(d, torch.where(out > 0, gy, torch.zeros_like(gy)))
    s = ops_pose.add2(d, gy)
    assert torch.equal(s, (d.float() + gy.float()).to(dtype))


# ------------------------------------------------------------------ pose head

def _head_operands(n_bins, dtype):
    n, hw, c = 3, 6, 64
    g = torch.Generator().manual_seed(36 + n_bins)
    x = torch.randn(n, c, 2, 3, generator=g).to(dtype).float()
    rows = (n_bins, n_bins, n_bins, 3, 1)
    ws = [torch.randn(r, c, generator=g) / math.sqrt(c) * 3 for r in rows]     # logits spread over a few units
    bs = [torch.randn(r, generator=g) for r in rows]
    g_out = torch.randn(n, 7, generator=g)
    return x, ws, bs, g_out


def _head_ref(n_bins, dtype):
    x, ws, bs, g_out = _head_operands(n_bins, dtype)
    xx = x.double().requires_grad_(True)
    ww = [w.double().requires_grad_(True) for w in ws]
    bb = [b.double().requires_grad_(True) for b in bs]
    feat = xx.mean((2, 3))
    idx = torch.arange(n_bins, dtype=torch.float64)
    cols = []
    for i in range(3):
        p = torch.softmax(feat @ ww[i].t() + bb[i], 1)
        cols.append((((p * idx).sum(1) - n_bins // 2) * 3 * math.pi / 180)[:, None])
    cols += [feat @ ww[3].t() + bb[3], feat @ ww[4].t() + bb[4]]
    out = torch.cat(cols, 1)
    (out * g_out.double()).sum().backward()
    return out.detach(), xx.grad, [w.grad for w in ww], [b.grad for b in bb]


@DTYPES
@pytest.mark.parametrize("n_bins", [6, 66])
def test_pose_head_vs_fp64(n_bins, dtype):
    x, ws, bs, g_out = _head_operands(n_bins, dtype)
    rout, rdx, rdw, rdb = _head_ref(n_bins, dtype)
    g = Guarded()
    old, ops._empty = ops._empty, g
    try:
        h = nhwc(x, dtype).requires_grad_(True)
        wb = [t.cuda().requires_grad_(True) for pair in zip(ws, bs) for t in pair]
        out = ops_pose.PoseHeadFn.apply(h, n_bins, dtype, *wb)
        out.backward(g_out.cuda())
        torch.cuda.synchronize()
        grads1, dx1 = [t.grad.clone() for t in wb], h.grad.clone()
        for t in wb + [h]:
            t.grad = None
        ops_pose.PoseHeadFn.apply(h, n_bins, dtype, *wb).backward(g_out.cuda())
        torch.cuda.synchronize()
    finally:
        ops._empty = old
    print(f"\npose head n_bins={n_bins} {'bf16' if dtype == BF16 else 'fp32'}:")
    assert out.dtype == F32 and tuple(out.shape) == (3, 7)
    gate("out", out, rout, dtype, False)
    gate("dx", dx1.float(), rdx, dtype, True)
    assert torch.equal(dx1, h.grad)
    for i, name in enumerate(("yaw", "pitch", "roll", "t", "scale")):
        gate(f"dW {name}", grads1[2 * i], rdw[i], dtype, False)
        gate(f"db {name}", grads1[2 * i + 1], rdb[i], dtype, False)
    assert all(torch.equal(a, t.grad) for a, t in zip(grads1, wb)), "head gradient reruns differ"
    n, bad = g.check()
    assert n == 2 and not bad, (n, bad)


# ------------------------------------------------------------------ the default's widths on the 1x1 kernels

def _bn_ref(y, gamma, beta, eps=1e-5):
    m = y.mean((0, 2, 3), keepdim=True)
    v = y.var((0, 2, 3), unbiased=False, keepdim=True)
    return (y - m) / torch.sqrt(v + eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


@pytest.mark.parametrize("form", [("CNA", 2048, 512), ("CN", 512, 2048)], ids=["CNA_2048to512", "CN_512to2048"])
def test_default_widths_pass_the_1x1_kernels(form):
    pattern, cin, cout = form
    torch.manual_seed(41)
    blk = fv.ConvBlock2D(pattern, cin, cout, 1, 1, 0, False)
    with torch.no_grad():
        blk.bn.weight.uniform_(0.5, 1.5)
        blk.bn.bias.normal_()
    g = torch.Generator().manual_seed(42)
    x = torch.randn(2, cin, 4, 4, generator=g)
    gy = torch.randn(2, cout, 4, 4, generator=g)
    xx = x.double().requires_grad_(True)
    ps = {k: v.detach().double().requires_grad_(True) for k, v in blk.named_parameters()}
    z = _bn_ref(F.conv2d(xx, ps["layers.0.weight"], ps["layers.0.bias"]), ps["layers.1.weight"], ps["layers.1.bias"])
    z = z.relu() if pattern == "CNA" else z
    (z * gy.double()).sum().backward()
    for mode, tol in ((F32, 1e-3), (BF16, 1e-2)):
        blk = blk.cuda().train().set_compute_dtype(mode)
        for p in blk.parameters():
            p.grad = None
        xg = x.cuda().requires_grad_(True)
        out = blk(xg)
        (out.float() * gy.cuda()).sum().backward()
        torch.cuda.synchronize()
        eo, ex, ew = rel(out, z), rel(xg.grad, xx.grad), rel(blk.conv.weight.grad, ps["layers.0.weight"].grad)
        eg = rel(blk.bn.weight.grad, ps["layers.1.weight"].grad)
        print(f"\n{pattern} 1x1 {cin}->{cout} {'bf16' if mode == BF16 else 'fp32'}: out {eo:.2e} dx {ex:.2e} "
              f"dW {ew:.2e} dgamma {eg:.2e}")
        assert tuple(out.shape) == (2, cout, 4, 4)
        assert eo < tol, eo
        if mode == F32:
            assert ex < tol and ew < tol and eg < tol, (ex, ew, eg)
        else:
            assert all(torch.isfinite(t).all() for t in (xg.grad, blk.conv.weight.grad, blk.bn.weight.grad))


# ------------------------------------------------------------------ modules and model vs the reference

_GOLD = {}


def gold(case):
    if not _GOLD:
        _GOLD.update(load_golden("hpe.pt"))
    return _GOLD[case]


CTORS = {
    "stem": lambda: torch.nn.Sequential(fv.ConvBlock2D("CNA", 3, 16, 7, 2, 3, False), fv.MaxPool2d(3, 2, 1)),
    "bneck_id": lambda: fv.ResBottleneck(32, 32, 1, False),
    "bneck_proj": lambda: fv.ResBottleneck(16, 32, 1, False),
    "bneck_s2": lambda: fv.ResBottleneck(32, 64, 2, False),
}


def _dead_bias(k):
    """Bias of a conv directly in front of a training-mode BN (every ConvBlock2D conv here, layers.0
    of its block): zero gradient in exact arithmetic."""
    return k.endswith("layers.0.bias")


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
            if per_key is not None:
                print(f"    {k}: |d| {d:.2e} (zero-gradient bias, gate {lim:.2e})")
            assert d <= lim, (k, d, lim)
            continue
        e = rel(p.grad, gd[k])
        lim = tol if per_key is None else 3 * per_key[k].item()
        if per_key is not None:
            print(f"    {k}: {e:.2e} (emulation {per_key[k].item():.2e}, gate {lim:.2e})")
        if e > worst[1]:
            worst = (k, e)
        if e > lim:
            over.append((k, e, lim))
    print(f"{label}: worst parameter gradient {worst[0]} {worst[1]:.2e}")
    assert not over, over


def _check_buffers(mod, gd, tol):
    sd = mod.state_dict()
    for k, v in gd.items():
        if v.is_floating_point():
            assert rel(sd[k], v) < tol, (k, rel(sd[k], v))
        else:
            assert torch.equal(sd[k].cpu(), v), k


@pytest.mark.parametrize("case", list(CTORS))
def test_blocks_fp32_match_reference(case):
    gd = gold(case)
    torch.manual_seed(int(gd["seed"]))
    blk = CTORS[case]().cuda().train()
    for m in blk.modules():
        if hasattr(m, "_dtype"):
            m._dtype = F32
    has_dx = "dx" in gd
    x = gd["x"].cuda().requires_grad_(has_dx)
    y = blk(x)
    assert y.shape == gd["out"].shape
    (y.float() * gd["g"].cuda()).sum().backward()
    torch.cuda.synchronize()
    ey = rel(y, gd["out"])
    edx = rel(x.grad, gd["dx"]) if has_dx else 0.0
    print(f"\n{case} fp32 vs reference: out {ey:.2e} dx {edx:.2e}")
    assert ey < 1e-3 and edx < 1e-3
    assert has_dx or x.grad is None
    _check_param_grads(blk, gd["grads"], 1e-3, case)
    _check_buffers(blk, gd["buffers"], 1e-3)
    blk.eval()
    with torch.no_grad():
        ye = blk(gd["x"].cuda())
    assert rel(ye, gd["out_eval"]) < 1e-3


OUT_NAMES = ("yaw", "pitch", "roll", "t", "scale")


def _run_hpe(mode):
    gd = gold("hpe")
    torch.manual_seed(int(gd["seed"]))
    net = fv.HPE_EDE(False, **TOY).cuda().train().set_compute_dtype(mode)
    x = gd["x"].cuda().requires_grad_(True)
    outs = net(x)
    sum((o * gd["g"][n].cuda()).sum() for n, o in zip(OUT_NAMES, outs)).backward()
    torch.cuda.synchronize()
    assert x.grad is None                     # the image is data: no gradient
    return gd, net, dict(zip(OUT_NAMES, outs))


def test_hpe_fp32_matches_reference():
    gd, net, outs = _run_hpe(F32)
    rng = TOY["n_bins"] * 3 * math.pi / 180
    print("\nHPE_EDE fp32 vs reference:")
    for n in OUT_NAMES:
        assert outs[n].shape == gd["out"][n].shape and outs[n].dtype == F32, n
        if n in ("yaw", "pitch", "roll"):
            e = maxd(outs[n], gd["out"][n])
            print(f"  {n}: max |d| {e:.2e} (gate {1e-3 * rng:.2e})")
            assert e <= 1e-3 * rng, (n, e)
        else:
            e = rel(outs[n], gd["out"][n])
            print(f"  {n}: rel-L2 {e:.2e}")
            assert e < 1e-3, (n, e)
    _check_param_grads(net, gd["grads"], 1e-3, "HPE_EDE fp32")
    _check_buffers(net, gd["buffers"], 1e-3)
    net.eval()
    with torch.no_grad():
        ev = dict(zip(OUT_NAMES, net(gd["x"].cuda())))
    for n in OUT_NAMES:
        if n in ("yaw", "pitch", "roll"):
            assert maxd(ev[n], gd["out_eval"][n]) <= 1e-3 * rng, n
        else:
            assert rel(ev[n], gd["out_eval"][n]) < 1e-3, n


def test_hpe_bf16_vs_fp32_reference():
    gd, net, outs = _run_hpe(BF16)
    dev = gd["emu_dev"]
    print("\nHPE_EDE bf16 vs fp32 reference (gate = 3 x the bf16 emulation of the reference):")
    over = []
    for n in OUT_NAMES:
        e, lim = rel(outs[n], gd["out"][n]), 3 * dev["out"][n].item()
        print(f"  {n}: rel-L2 {e:.2e} (emulation {dev['out'][n].item():.2e}, gate {lim:.2e})")
        if e > lim:
            over.append((n, e, lim))
    assert not over, over
    _check_param_grads(net, gd["grads"], None, "HPE_EDE bf16", per_key=dev["grads"])


def test_hpe_workspaces_stay_in_bounds(monkeypatch):
    """Every caller-sized buffer of the new entries on the module path (weight image, BN records,
    argmax, weight-gradient slabs, head workspace) and of the existing entries they drive."""
    g = Guarded()
    monkeypatch.setattr(ops, "_empty", g)
    gd = gold("hpe")
    for mode in (F32, BF16):
        torch.manual_seed(3)
        net = fv.HPE_EDE(False, **TOY).cuda().train().set_compute_dtype(mode)
        outs = net(gd["x"].cuda())
        sum(o.sum() for o in outs).backward()
        seq = CTORS["stem"]().cuda().train()
        seq(gd["x"].cuda()).float().sum().backward()
    n, bad = g.check()
    assert n > 40, n
    assert not bad, f"{len(bad)} of {n} buffers written past their queried size: {bad[:8]}"


def test_hpe_transform_kp_mfe_compose():
    """image -> HPE_EDE -> transform_kp -> MFE: a loss on the deformation reaches every HPE_EDE parameter."""
    torch.manual_seed(7)
    hpe = fv.HPE_EDE(False, **TOY).cuda().train()
    mfe = fv.MFE(False, **MFE_TOY).cuda().train()
    g = torch.Generator().manual_seed(8)
    img = torch.rand(4, 3, 32, 48, generator=g).cuda()                  # two source and two driving images
    kp_c = ((torch.rand(2, 3, 3, generator=g) - 0.5) * 1.2).cuda()
    fs = torch.randn(2, 8, 4, 8, 8, generator=g).cuda()
    yaw, pitch, roll, t, scale = hpe(img)
    assert all(o.dtype == F32 for o in (yaw, pitch, roll, t, scale)) and tuple(scale.shape) == (4, 1, 1, 1)
    kp_s, Rs = fv.transform_kp(kp_c, yaw[:2], pitch[:2], roll[:2], t[:2], scale[:2])
    kp_d, Rd = fv.transform_kp(kp_c, yaw[2:], pitch[2:], roll[2:], t[2:], scale[2:])
    deformation, occlusion, mask = mfe(fs, kp_s, kp_d, Rs, Rd)
    assert all(torch.isfinite(o).all() for o in (deformation, occlusion, mask, kp_s, kp_d, Rs, Rd))
    gd = torch.randn(deformation.shape, generator=g).cuda()
    (deformation * gd).sum().backward()
    torch.cuda.synchronize()
    dead = [k for k, p in hpe.named_parameters()
            if p.grad is None or not torch.isfinite(p.grad).all() or p.grad.abs().sum().item() == 0]
    assert not dead, dead
