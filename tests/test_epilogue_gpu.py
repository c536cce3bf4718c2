"""GPU checks of the 3x3 halo kernels' epilogues (conv3_halo_fwd2 / fwd3: the bounds-free store
pass of conv_epilogue) and of the sliding-row weight gradient's slab write (conv3_halo_wgrad2),
through the public conv entry points, against torch float64 on the host CPU.

Every case runs bf16 at the smallest shape that reaches its tile: one 256-pixel tile per co tile
and more than one block.  The reference is computed once per case, on the bf16-rounded operands
the kernels read, so what is left is the fp32 accumulation and the bf16 rounding of the output
(2^-9 relative per element; bound 1e-2 relative L2 as for test_conv3x3_64ch_with_residual).
Record sums are compared with the float64 sums of the reference (1e-2 of the absolute sums, the
bound of test_conv_fwd's statistics) and, for the store-pass records, with the float64 sums of
the very tensor the launch stored (fp32 sums of <= 64 terms per record: 1e-5).  Each launch runs
twice and must repeat bit for bit."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
from facevae_amd import _lib as L  # noqa: E402
from facevae_amd import ops  # noqa: E402

CL = torch.channels_last
BF = torch.bfloat16
TOL_Y = 1e-2          # relative L2 of a bf16 output against float64 on the same bf16 operands
TOL_SUM = 1e-2        # record-derived sums against the float64 reference's
TOL_REC = 1e-5        # store-pass records against float64 sums of the stored tensor itself


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bfr(t):
    """t rounded to bf16, as float64."""
    return t.to(BF).double()


# name -> (cin, cout, N, H, W)
FWD_CASES = {
    "a_256co": (128, 256, 1, 8, 64),       # 256-co tile
    "b_128co": (256, 256, 1, 8, 64),       # 128-co tile (fewer 256-co tiles than CUs)
    "c_64co": (128, 64, 1, 8, 64),         # 64-co tile on 8-row tiles
    "d_res": (256, 256, 2, 64, 64),        # the res convs' shape at minimal batch
}
# (bias, fp32 statistics records, residual + store-pass records through fv_conv2d_fwd_sr)
VARIANTS = {
    "plain": (False, False, False),
    "bias": (True, False, False),
    "stats": (False, True, False),
    "bias_stats": (True, True, False),
    "res_sr": (False, False, True),
    "bias_res_sr": (True, False, True),
}


@functools.lru_cache(maxsize=None)
def fwd_case(name):
    """Inputs and the float64 reference of a forward case (shared by its variants, not modified)."""
    cin, cout, N, H, W = FWD_CASES[name]
    g = torch.Generator().manual_seed(4100 + cin + cout + H)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=g)
    r = torch.randn(N, cout, H, W, generator=g)
    conv = F.conv2d(bfr(x), bfr(w), None, padding=1)
    return x, w, b, r, conv


def run_fwd(name, bias, stats, sr):
    """One launch of a forward case -> (y, fp32 statistics partials or None, store-pass records or None)."""
    cin, cout, N, H, W = FWD_CASES[name]
    x, w, b, r, _ = fwd_case(name)
    xb, cp = ops.to_nhwc(x.cuda(), BF)
    d = ops.desc(BF, N, H, W, cp, cin, cout, cout, 3)
    wk = torch.empty(L.query("fv_conv_wk_elems", ctypes.byref(d)), dtype=BF, device="cuda")
    L.call("fv_conv_weight_prep", ctypes.byref(d), w.cuda().float().contiguous().data_ptr(), None, wk.data_ptr(), None,
           L.stream())
    bd = b.cuda() if bias else None
    y = torch.full((N, cout, H, W), float("nan"), dtype=BF, device="cuda").contiguous(memory_format=CL)
    part = rec = None
    if sr:
        bp = ctypes.c_int(0)
        nrec = L.query("fv_conv2d_sr_records", ctypes.byref(d), 0, ctypes.byref(bp))
        assert nrec == N * H * W // bp.value and bp.value in (32, 64), (nrec, bp.value)
        rec = torch.full((nrec * 2 * cout,), float("nan"), device="cuda")
        rb = r.cuda().to(BF).contiguous(memory_format=CL)
        s = L.StoreReduce(1, rec.data_ptr(), None, None, None, None, None, 0.0)
        L.call("fv_conv2d_fwd_sr", ctypes.byref(d), xb.data_ptr(), wk.data_ptr(), L.ptr(bd), rb.data_ptr(), y.data_ptr(),
               ctypes.byref(s), L.stream())
        rec = rec.view(nrec, 2, cout)
    else:
        if stats:
            nb = L.query("fv_conv2d_stats_blocks", ctypes.byref(d))
            part = torch.full((nb * 2 * cout,), float("nan"), device="cuda")
        L.call("fv_conv2d_fwd", ctypes.byref(d), xb.data_ptr(), wk.data_ptr(), L.ptr(bd), None, None, None, y.data_ptr(),
               L.ptr(part), L.stream())
    torch.cuda.synchronize()
    return d, y, part, rec


def check_fwd(name, variant, monkeypatch, pers=False):
    bias, stats, sr = VARIANTS[variant]
    cin, cout, N, H, W = FWD_CASES[name]
    x, w, b, r, conv = fwd_case(name)
    ref = conv + (b.double()[None, :, None, None] if bias else 0)       # the fp32 accumulator + bias
    out = bfr(ref) + bfr(r) if sr else ref                               # the residual joins the rounded tile
    d, y, part, rec = run_fwd(name, bias, stats, sr)
    d2, y2, part2, rec2 = run_fwd(name, bias, stats, sr)
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), "two launches differ"
    assert not torch.isnan(y.float()).any(), "output not fully written"
    e = rel(y, out)
    print(f"{name} {variant}: y rel {e:.2e}")
    assert e < TOL_Y
    P = N * H * W
    if stats:
        assert torch.equal(part, part2), "two launches' statistics records differ"
        st = torch.empty(3 * cout, dtype=torch.float64, device="cuda")
        ws = torch.empty(L.query("fv_bn_ws_bytes", cout) // 8, dtype=torch.float64, device="cuda")
        nb = L.query("fv_conv2d_stats_blocks", ctypes.byref(d))
        L.call("fv_bn_stats_from_partials", part.data_ptr(), nb, L.query("fv_conv2d_stats_block_pixels", ctypes.byref(d)),
               P, cout, st.data_ptr(), ws.data_ptr(), L.stream())
        torch.cuda.synchronize()
        s = st.cpu().view(3, cout)
        yr = ref.permute(1, 0, 2, 3).reshape(cout, -1)
        assert torch.allclose(s[0], torch.full((cout,), float(P), dtype=torch.float64))
        e1 = ((s[1] - yr.sum(1)).abs() / yr.abs().sum(1)).max().item()
        e2 = rel(s[2], (yr * yr).sum(1))
        print(f"{name} {variant}: statistics sum {e1:.2e} sumsq {e2:.2e}")
        assert e1 < TOL_SUM and e2 < TOL_SUM
    if sr:
        assert torch.equal(rec, rec2), "two launches' store-pass records differ"
        got = rec.double().sum(0).cpu()                                  # [2][cout]
        ys = y.double().cpu().permute(1, 0, 2, 3).reshape(cout, -1)      # what the launch stored
        yr = out.permute(1, 0, 2, 3).reshape(cout, -1)
        e0 = ((got[0] - ys.sum(1)).abs() / ys.abs().sum(1)).max().item()
        e0q = rel(got[1], (ys * ys).sum(1))
        e1 = ((got[0] - yr.sum(1)).abs() / yr.abs().sum(1)).max().item()
        e2 = rel(got[1], (yr * yr).sum(1))
        print(f"{name} {variant}: records vs stored {e0:.2e} {e0q:.2e}, vs float64 {e1:.2e} {e2:.2e}")
        assert e0 < TOL_REC and e0q < TOL_REC
        assert e1 < TOL_SUM and e2 < TOL_SUM
    return y, part, rec


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_halo_fwd_epilogue(name, variant, monkeypatch):
    check_fwd(name, variant, monkeypatch)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_halo_fwd_epilogue_persistent(variant, monkeypatch):
    """Case b on a persistent grid of one block: the block walks every tile, the next tile's
    prologue issued between the epilogue's LDS read-back and its stores (the `mid` hook).  Same
    results bit for bit as one tile per block."""
    y0, part0, rec0 = check_fwd("b_128co", variant, monkeypatch)
    monkeypatch.setenv("FV_PERS_GRID", "1")
    y1, part1, rec1 = check_fwd("b_128co", variant, monkeypatch)
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    if part0 is not None:
        assert torch.equal(part0, part1)
    if rec0 is not None:
        assert torch.equal(rec0, rec1)


@functools.lru_cache(maxsize=None)
def dgrad_case():
    """The data gradient of a 64 -> 128 conv (AFE.down1's shape: a 128 -> 64 conv over dy, the 64-co
    tile) at N=1, H=8, W=64, and its float64 reference."""
    cin, cout, N, H, W = 64, 128, 1, 8, 64
    g = torch.Generator().manual_seed(4242)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    gy = torch.randn(N, cout, H, W, generator=g)
    ybn = torch.randn(N, cin, H, W, generator=g)                        # the BN input of the layer below
    mean = torch.randn(cin, generator=g) * 0.1
    invstd = torch.rand(cin, generator=g) + 0.5
    gamma = torch.randn(cin, generator=g)
    beta = torch.randn(cin, generator=g) * 0.3
    dx = F.conv_transpose2d(bfr(gy), bfr(w), None, padding=1)
    return w, gy, ybn, mean, invstd, gamma, beta, dx


def run_dgrad(sr, slope=0.2):
    cin, cout, N, H, W = 64, 128, 1, 8, 64
    w, gy, ybn, mean, invstd, gamma, beta, _ = dgrad_case()
    d = ops.desc(BF, N, H, W, cin, cin, cout, cout, 3)
    wk = torch.empty(L.query("fv_conv_wk_elems", ctypes.byref(d)), dtype=BF, device="cuda")
    wt = torch.empty(L.query("fv_conv_wt_elems", ctypes.byref(d)), dtype=BF, device="cuda")
    L.call("fv_conv_weight_prep", ctypes.byref(d), w.cuda().float().contiguous().data_ptr(), None, wk.data_ptr(),
           wt.data_ptr(), L.stream())
    gyb = gy.cuda().to(BF).contiguous(memory_format=CL)
    dx = torch.full((N, cin, H, W), float("nan"), dtype=BF, device="cuda").contiguous(memory_format=CL)
    rec = None
    if sr:
        bp = ctypes.c_int(0)
        nrec = L.query("fv_conv2d_sr_records", ctypes.byref(d), 1, ctypes.byref(bp))
        assert nrec == N * H * W // 64 and bp.value == 64, (nrec, bp.value)
        rec = torch.full((nrec * 2 * cin,), float("nan"), device="cuda")
        yb = ybn.cuda().to(BF).contiguous(memory_format=CL)
        keep = [mean.cuda(), invstd.cuda(), gamma.cuda(), beta.cuda()]
        s = L.StoreReduce(2, rec.data_ptr(), yb.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                          keep[3].data_ptr(), float(slope))
        L.call("fv_conv2d_bwd_data_sr", ctypes.byref(d), gyb.data_ptr(), cout, wt.data_ptr(), dx.data_ptr(), ctypes.byref(s),
               L.stream())
        rec = rec.view(nrec, 2, cin)
    else:
        L.call("fv_conv2d_bwd_data", ctypes.byref(d), gyb.data_ptr(), cout, wt.data_ptr(), dx.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return dx, rec


@pytest.mark.parametrize("sr", [False, True])
def test_halo_dgrad_epilogue(sr):
    """Case c as the workload runs it: the 64-co tile of AFE.down1's data gradient, plain and with
    the BN-backward sums (store-pass records, mode 2) of the stored gradient."""
    cin = 64
    w, gy, ybn, mean, invstd, gamma, beta, ref = dgrad_case()
    slope = 0.2
    dx, rec = run_dgrad(sr, slope)
    dx2, rec2 = run_dgrad(sr, slope)
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16)), "two launches differ"
    assert not torch.isnan(dx.float()).any(), "gradient not fully written"
    e = rel(dx, ref)
    print(f"dgrad sr={sr}: dx rel {e:.2e}")
    assert e < TOL_Y
    plain, _ = (dx, None) if not sr else run_dgrad(False, slope)
    assert torch.equal(dx.view(torch.int16), plain.view(torch.int16)), "records change the stored gradient"
    if sr:
        assert torch.equal(rec, rec2), "two launches' records differ"
        got = rec.double().sum(0).cpu()                                  # [2][cin]: sum g, sum g * yhat

        def sums(v):                                                     # v: the gradient, float64 NCHW
            yhat = (bfr(ybn) - mean.double()[None, :, None, None]) * invstd.double()[None, :, None, None]
            pre = gamma.double()[None, :, None, None] * yhat + beta.double()[None, :, None, None]
            gg = torch.where(pre > 0, v, v * slope)
            f = lambda t: t.permute(1, 0, 2, 3).reshape(cin, -1)
            return f(gg).sum(1), f(gg * yhat).sum(1), f(gg).abs().sum(1), f(gg * yhat).abs().sum(1)

        s0, q0, sa, qa = sums(dx.double().cpu())                         # of the stored gradient itself
        e0 = ((got[0] - s0).abs() / sa).max().item()
        e0q = ((got[1] - q0).abs() / qa).max().item()
        s1, q1, sa1, qa1 = sums(ref)
        e1 = ((got[0] - s1).abs() / sa1).max().item()
        e1q = ((got[1] - q1).abs() / qa1).max().item()
        print(f"dgrad records vs stored {e0:.2e} {e0q:.2e}, vs float64 {e1:.2e} {e1q:.2e}")
        assert e0 < TOL_REC and e0q < TOL_REC
        assert e1 < TOL_SUM and e1q < TOL_SUM


# (cin, cout, N, H, W): one strip, two strips, the res convs' 4 ci tiles x 2 co tiles
WGRAD_CASES = [(64, 128, 1, 8, 64), (64, 128, 1, 8, 128), (256, 256, 2, 8, 64)]


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_halo_wgrad_slab(case):
    """dW and db of the sliding-row weight gradient through its slab and the slab reduce."""
    cin, cout, N, H, W = case
    g = torch.Generator().manual_seed(4300 + cin + W)
    x = torch.randn(N, cin, H, W, generator=g)
    gy = torch.randn(N, cout, H, W, generator=g)
    wr = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    (F.conv2d(bfr(x), wr, br, padding=1) * bfr(gy)).sum().backward()
    xb, cp = ops.to_nhwc(x.cuda(), BF)
    d = ops.desc(BF, N, H, W, cp, cin, cout, cout, 3)
    gyb = gy.cuda().to(BF).contiguous(memory_format=CL)

    def run():
        slab = torch.full((L.query("fv_conv2d_wgrad_slab_elems", ctypes.byref(d)),), float("nan"), device="cuda")
        bslab = torch.full((L.query("fv_conv2d_wgrad_bias_slab_elems", ctypes.byref(d)),), float("nan"), device="cuda")
        L.call("fv_conv2d_bwd_weight", ctypes.byref(d), xb.data_ptr(), None, None, gyb.data_ptr(), cout, slab.data_ptr(),
               bslab.data_ptr(), L.stream())
        dw = torch.empty(cout, cin, 3, 3, device="cuda")
        db = torch.empty(cout, device="cuda")
        L.call("fv_conv2d_wgrad_reduce", ctypes.byref(d), slab.data_ptr(), bslab.data_ptr(), dw.data_ptr(), db.data_ptr(),
               L.stream())
        torch.cuda.synchronize()
        return slab, bslab, dw, db

    slab, bslab, dw, db = run()
    slab2, bslab2, dw2, db2 = run()
    assert torch.equal(slab.view(torch.int32), slab2.view(torch.int32)) and torch.equal(dw, dw2) and torch.equal(db, db2)
    assert not torch.isnan(slab).any() and not torch.isnan(bslab).any(), "slab not fully written"
    # fp32 sums of exact bf16 products over N * H * W pixels, split over the slab's partial sums:
    # far inside the harness's bf16 bound
    ew, eb = rel(dw, wr.grad), rel(db, br.grad)
    print(f"wgrad {case}: dW rel {ew:.2e} db rel {eb:.2e}")
    assert ew < 1e-4 and eb < 1e-4
