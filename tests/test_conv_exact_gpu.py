"""Exact-operand parity of the 2-D conv kernel families on the GPU: every output of every launch
must equal the float64 reference BIT FOR BIT after one rounding to the output type.

The operands are small integers (tests/exact_operands.py), so every product and every partial
sum is exact in fp32 whatever the tile shape, split count or summation order: there is no
tolerance to hide behind, and a mismatch comes with its coordinates and bounding box (one tile,
one column, one channel group, one tap).  Outputs are pre-filled with NaN between two canary
regions, so an element never written and a write outside the buffer both fail.  Every launch
runs twice and must repeat bit for bit.

Through the public entry points only, called as tests/test_kernels_gpu.py, test_disc_gpu.py and
test_epilogue_gpu.py call them, in bf16 (the fast kernels: conv_fwd_v2, the halo 3x3 / 7x7,
sub-pixel and band upsample kernels, conv1x1_stream, conv7c4, conv7_n3, the weight-gradient
families) and in fp32 (the exact fp32 MFMA path):
  forward          fv_conv2d_fwd: y, and the statistics records folded by fv_bn_stats_from_partials
                   (count and sum exact; the sum of squares is a fp32 sum of up to
                   block_pixels non-negative terms, each a rounded square: relative error at most
                   (block_pixels + 1) * 2^-23 -- derived, the only bound in this file)
  data gradient    fv_conv2d_bwd_data, then fv_upsample2x_bwd unless fv_conv2d_dgrad_lowres
  weight gradient  fv_conv2d_bwd_weight + fv_conv2d_wgrad_reduce: dw and db as exact integers
  stride 2         the fv_conv2d_s2_* set
  store pass       fv_conv2d_fwd_sr (bias + residual; records against the stored tensor and the
                   reference) and the dx of fv_conv2d_bwd_data_sr -- bf16 only: the store pass
                   exists only on the bf16 halo kernels (fv_conv2d_sr_records is 0 in fp32)

Not covered here, because their arithmetic is not exact on any operands: epi_sigmoid, the
demodulated ConvTranspose path, and the mode-2 records of fv_conv2d_bwd_data_sr (transcendental
or invstd arithmetic).  fp8 has its own elementwise gates in test_fp8_gpu.py.  The 3-D convs
are held to the same equality in tests/test_conv3d_exact_gpu.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
from facevae_amd import _lib as L  # noqa: E402
from facevae_amd import ops  # noqa: E402

import exact_operands as X  # noqa: E402
from exact_operands import Guarded, assert_exact  # noqa: E402

CL = torch.channels_last
DTYPES = [torch.float32, torch.bfloat16]


def same_bits(a, b):
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def twice(run, what):
    """run() -> tuple of tensors, launched twice into fresh buffers: the results repeat bit for bit"""
    a, b = run(), run()
    for i, (u, v) in enumerate(zip(a, b)):
        assert same_bits(u, v), f"{what}: output {i} differs between two launches"
    return a


def dev(t, dtype=torch.float32):
    return t.to(dtype).cuda().contiguous()


def nhwc_padded(t, dtype, ld):
    """float64 NCHW on the CPU -> NHWC on the GPU with channel stride ld, padding channels 0"""
    N, C, H, W = t.shape
    buf = torch.zeros((N, ld, H, W), dtype=dtype, device="cuda").contiguous(memory_format=CL)
    buf[:, :C] = t.to(dtype).cuda()
    return buf


def prep(c, dtype, need_wt=False, slope=0.0):
    """descriptor, NHWC input and prepared weights of a stride-1 case (test_kernels_gpu.conv_setup)"""
    xb, cp = ops.to_nhwc(c.x.float().cuda(), dtype)
    N, cout, H, W = c.out_shape
    d = ops.desc(dtype, N, H, W, cp, c.cin, cout, cout, c.k, c.ups, c.pro, slope, False, 0)
    wk = torch.empty(L.query("fv_conv_wk_elems", ctypes.byref(d)), dtype=dtype, device="cuda")
    wt = torch.empty(L.query("fv_conv_wt_elems", ctypes.byref(d)), dtype=dtype, device="cuda") if need_wt else None
    wc = dev(c.w)
    L.call("fv_conv_weight_prep", ctypes.byref(d), wc.data_ptr(), None, wk.data_ptr(), L.ptr(wt), L.stream())
    return d, xb, cp, wk, wt


def check_stats(d, part, nb, c, dtype, what):
    """the statistics records against the float64 reference (the fp32 accumulator, before y's rounding)"""
    N, cout, H, W = c.out_shape
    P = N * H * W
    bp = L.query("fv_conv2d_stats_block_pixels", ctypes.byref(d))
    stats = torch.empty(3 * cout, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.query("fv_bn_ws_bytes", cout) // 8, dtype=torch.float64, device="cuda")
    L.call("fv_bn_stats_from_partials", part.data_ptr(), nb, bp, P, cout, stats.data_ptr(), ws.data_ptr(), L.stream())
    torch.cuda.synchronize()
    s = stats.cpu().view(3, cout)
    yr = c.y.permute(1, 0, 2, 3).reshape(cout, -1)
    assert torch.equal(s[0], torch.full((cout,), float(P), dtype=torch.float64)), f"{what}: statistics count"
    assert_exact(s[1], yr.sum(1), f"{what}: statistics sum per channel")
    q = (yr * yr).sum(1)
    e = ((s[2] - q).abs() / q).max().item()
    bound = (bp + 1) * 2.0 ** -23
    print(f"{what}: {nb} records of {bp} pixels, sum of squares rel {e:.3e} (bound {bound:.3e})")
    assert e <= bound, f"{what}: statistics sum of squares off by {e:.3e} relative, bound {bound:.3e}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cn", X.FWD_LIST, ids=X.case_id)
def test_conv_fwd_exact(cn, dtype, monkeypatch):
    case, N = cn
    if case == X.C7_BAND_CASE:
        monkeypatch.setenv("FV_C7_BAND", "64")     # conv7_n3_fwd2: 16 row groups per block
    c = X.conv_case(case, N)
    what = f"fwd {X.case_id(cn)} {dtype}"
    d, xb, cp, wk, _ = prep(c, dtype, slope=X.FWD_SLOPE if c.pro else 0.0)
    cout = c.cout
    nchw = cout % 4 != 0
    if nchw:
        d.out_nchw_f32 = 1
    bias, scd, shd = dev(c.b), dev(c.sc), dev(c.sh)
    nb = L.query("fv_conv2d_stats_blocks", ctypes.byref(d))
    assert L.conv_kernel(d, stats=True) == X.conv_kinds(case, dtype)[0], what + ": kernel kind"

    def run():
        y = Guarded(c.out_shape, torch.float32 if nchw else dtype, nhwc=not nchw)
        part = Guarded((nb * 2 * cout,), torch.float32)
        L.call("fv_conv2d_fwd", ctypes.byref(d), xb.data_ptr(), wk.data_ptr(), bias.data_ptr(),
               L.ptr(scd if c.pro else None), L.ptr(shd if c.pro else None), None, y.data_ptr(), part.data_ptr(),
               L.stream())
        torch.cuda.synchronize()
        y.check_canary(what + " y")
        part.check_canary(what + " statistics records")
        return y.t, part.flat

    y, part = twice(run, what)
    assert_exact(y, c.y, what + " y")
    if cout % 8 == 0:
        check_stats(d, part, nb, c, dtype, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cn", X.DGRAD_LIST, ids=X.case_id)
def test_conv_dgrad_exact(cn, dtype):
    case, N = cn
    c = X.conv_case(case, N)
    what = f"dgrad {X.case_id(cn)} {dtype}"
    d, xb, cp, _, wt = prep(c, dtype, need_wt=True)
    _, cout, H, W = c.out_shape
    ldd = ops.pad_pow2(cout)
    gyb = nhwc_padded(c.gy_d, dtype, ldd)
    lowres = bool(c.ups and L.query("fv_conv2d_dgrad_lowres", ctypes.byref(d)))
    assert L.conv_kernel(d, dgrad=True) == X.conv_kinds(case, dtype)[1], what + ": kernel kind"

    def run():
        shape = (N, cp, c.H, c.W) if lowres else (N, cp, H, W)
        dx = Guarded(shape, dtype, nhwc=True)
        L.call("fv_conv2d_bwd_data", ctypes.byref(d), gyb.data_ptr(), ldd, wt.data_ptr(), dx.data_ptr(), L.stream())
        outs = [dx]
        if c.ups and not lowres:
            src = Guarded((N, cp, c.H, c.W), dtype, nhwc=True)
            L.call("fv_upsample2x_bwd", L.dtype_code(dtype), dx.data_ptr(), N, c.H, c.W, cp, src.data_ptr(), L.stream())
            outs.append(src)
        torch.cuda.synchronize()
        for o in outs:
            o.check_canary(what + " dx")
        return tuple(o.t for o in outs)

    outs = twice(run, what)
    hi = c.dx_conv                                          # at the conv's resolution
    if lowres:
        assert_exact(outs[0][:, :c.cin], X.pool2_sum(hi), what + " dx (low-res path)")
    else:
        assert_exact(outs[0][:, :c.cin], hi, what + " dx")
        if c.ups:
            # fv_upsample2x_bwd sums the four stored (already rounded) gradients and rounds again
            assert_exact(outs[1][:, :c.cin], X.pool2_sum(hi.to(dtype).double()), what + " dx after fv_upsample2x_bwd")
    if cp > c.cin:      # the header promises nothing about the padded channels of the generic conv
        print(f"{what}: padded channels of dx: max |.| {outs[-1][:, c.cin:].float().abs().max().item()}")


def wgrad_run(d, c, dtype, xb, gyb, ldd, what, fam=""):
    """weight + bias gradient through the slabs and their reduce, into NaN-filled guarded dw / db"""
    pro = bool(c.pro)
    scd, shd = dev(c.sc), dev(c.sh)
    nslab = L.query(f"fv_conv2d{fam}_wgrad_slab_elems", ctypes.byref(d))
    nbslab = L.query(f"fv_conv2d{fam}_wgrad_bias_slab_elems", ctypes.byref(d))

    def run():
        slab = torch.full((nslab,), float("nan"), device="cuda")
        bslab = torch.full((nbslab,), float("nan"), device="cuda")
        if fam:
            L.call("fv_conv2d_s2_bwd_weight", ctypes.byref(d), 2 * c.H, 2 * c.W, xb.data_ptr(), gyb.data_ptr(), ldd,
                   slab.data_ptr(), bslab.data_ptr(), L.stream())
        else:
            L.call("fv_conv2d_bwd_weight", ctypes.byref(d), xb.data_ptr(), L.ptr(scd if pro else None),
                   L.ptr(shd if pro else None), gyb.data_ptr(), ldd, slab.data_ptr(), bslab.data_ptr(), L.stream())
        dw = Guarded((c.cout, c.cin, c.k, c.k), torch.float32)
        db = Guarded((c.cout,), torch.float32)
        L.call(f"fv_conv2d{fam}_wgrad_reduce", ctypes.byref(d), slab.data_ptr(), bslab.data_ptr(), dw.data_ptr(),
               db.data_ptr(), L.stream())
        torch.cuda.synchronize()
        dw.check_canary(what + " dw")
        db.check_canary(what + " db")
        return dw.t, db.t

    dw, db = twice(run, what)
    dw_ref, db_ref = c.dw_db
    assert_exact(dw, dw_ref, what + " dw (co, ci, r, s)")
    assert_exact(db, db_ref, what + " db")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("cn", X.WGRAD_LIST, ids=X.case_id)
def test_conv_wgrad_exact(cn, dtype):
    case, N = cn
    c = X.conv_case(case, N)
    what = f"wgrad {X.case_id(cn)} {dtype}"
    xb, cp = ops.to_nhwc(c.x.float().cuda(), dtype)
    _, cout, H, W = c.out_shape
    d = ops.desc(dtype, N, H, W, cp, c.cin, cout, cout, c.k, c.ups, c.pro, 0.0, False, 0)
    ldd = ops.pad_pow2(cout)
    wgrad_run(d, c, dtype, xb, nhwc_padded(c.gy_w, dtype, ldd), ldd, what)


# ------------------------------------------------------------------------ stride-2 conv
def s2_prep(c, dtype, need_wt=False):
    xb, cp = ops.to_nhwc(c.x.float().cuda(), dtype)
    ldy = ops.pad_pow2(c.cout)
    d = ops.desc(dtype, c.N, c.H, c.W, cp, c.cin, c.cout, ldy, 3)
    wk = torch.empty(L.query("fv_conv2d_s2_wk_elems", ctypes.byref(d)), dtype=dtype, device="cuda")
    wt = torch.empty(L.query("fv_conv2d_s2_wt_elems", ctypes.byref(d)), dtype=dtype, device="cuda") if need_wt else None
    wc = dev(c.w)
    L.call("fv_conv2d_s2_weight_prep", ctypes.byref(d), wc.data_ptr(), None, wk.data_ptr(), L.ptr(wt), L.stream())
    return d, xb, cp, ldy, wk, wt


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", X.S2_CASES, ids=X.case_id)
def test_conv_s2_fwd_exact(case, dtype):
    c = X.s2_case(case)
    what = f"s2 fwd {case} {dtype}"
    d, xb, cp, ldy, wk, _ = s2_prep(c, dtype)
    bias = dev(c.b)

    def run():
        y = Guarded((c.N, ldy, c.H, c.W), dtype, nhwc=True)
        L.call("fv_conv2d_s2_fwd", ctypes.byref(d), 2 * c.H, 2 * c.W, xb.data_ptr(), wk.data_ptr(), bias.data_ptr(),
               y.data_ptr(), L.stream())
        torch.cuda.synchronize()
        y.check_canary(what + " y")
        return (y.t,)

    (y,) = twice(run, what)
    assert_exact(y[:, :c.cout], c.y, what + " y")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", X.S2_CASES, ids=X.case_id)
def test_conv_s2_dgrad_exact(case, dtype):
    c = X.s2_case(case)
    what = f"s2 dgrad {case} {dtype}"
    d, xb, cp, ldy, _, wt = s2_prep(c, dtype, need_wt=True)
    dyb, ldd = ops.to_nhwc(c.gy_d.float().cuda(), dtype)    # channel stride pad_pow2(cout), padding 0

    def run():
        dx = Guarded((c.N, cp, 2 * c.H, 2 * c.W), dtype, nhwc=True)
        L.call("fv_conv2d_s2_bwd_data", ctypes.byref(d), 2 * c.H, 2 * c.W, dyb.data_ptr(), ldd, wt.data_ptr(),
               dx.data_ptr(), L.stream())
        torch.cuda.synchronize()
        dx.check_canary(what + " dx")
        return (dx.t,)

    (dx,) = twice(run, what)
    assert_exact(dx[:, :c.cin], c.dx_conv, what + " dx")
    if cp > c.cin:
        assert bool((dx[:, c.cin:] == 0).all()), f"{what}: padded input channels of dx must be 0"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", X.S2_CASES, ids=X.case_id)
def test_conv_s2_wgrad_exact(case, dtype):
    c = X.s2_case(case)
    what = f"s2 wgrad {case} {dtype}"
    d, xb, cp, ldy, _, _ = s2_prep(c, dtype)
    dyb, ldd = ops.to_nhwc(c.gy_w.float().cuda(), dtype)
    wgrad_run(d, c, dtype, xb, dyb, ldd, what, fam="_s2")


# ------------------------------------------------------------------------ store pass (bf16 halo kernels)
@pytest.mark.parametrize("name", list(X.SR_CASES))
def test_conv_fwd_store_pass_exact(name):
    """fv_conv2d_fwd_sr with bias and residual: the residual joins the bf16-rounded tile; with
    |conv + bias| + |res| <= 256 both are exact integers wherever the kernel rounds.  The records
    (at most 64 pixels each, |y| <= 256: sums <= 2^14, sums of squares <= 2^22) are exact too."""
    dtype = torch.bfloat16
    c = X.sr_case(name)
    what = f"fwd_sr {name}"
    d, xb, cp, wk, _ = prep(c, dtype)
    N, cout, H, W = c.out_shape
    bias = dev(c.b)
    rb = c.r.to(dtype).cuda().contiguous(memory_format=CL)
    bp = ctypes.c_int(0)
    nrec = L.query("fv_conv2d_sr_records", ctypes.byref(d), 0, ctypes.byref(bp))
    assert nrec == N * H * W // bp.value and bp.value in (32, 64), (nrec, bp.value)
    assert L.conv_kernel(d, res=True, sr_mode=1) == X.SR_KINDS[name], what + ": kernel kind"

    def run():
        y = Guarded(c.out_shape, dtype, nhwc=True)
        rec = Guarded((nrec, 2, cout), torch.float32)
        s = L.StoreReduce(1, rec.data_ptr(), None, None, None, None, None, 0.0)
        L.call("fv_conv2d_fwd_sr", ctypes.byref(d), xb.data_ptr(), wk.data_ptr(), bias.data_ptr(), rb.data_ptr(),
               y.data_ptr(), ctypes.byref(s), L.stream())
        torch.cuda.synchronize()
        y.check_canary(what + " y")
        rec.check_canary(what + " records")
        return y.t, rec.t

    y, rec = twice(run, what)
    out = c.y + c.r
    assert_exact(y, out, what + " y")
    got = rec.double().sum(0).cpu()                          # [2][cout]
    for v, src in ((y.double().cpu(), "the stored tensor"), (out, "the reference")):
        f = v.permute(1, 0, 2, 3).reshape(cout, -1)
        assert_exact(got[0], f.sum(1), f"{what}: record sums against {src}")
        assert_exact(got[1], (f * f).sum(1), f"{what}: record sums of squares against {src}")


def test_conv_dgrad_store_pass_dx_exact():
    """The dx of fv_conv2d_bwd_data_sr (AFE.down1's data gradient on the 64-co halo tile): its
    mode-2 records carry invstd arithmetic and are not compared, the stored gradient is."""
    dtype = torch.bfloat16
    c = X.conv_case(X.SR_DGRAD_CASE, 1)
    what = "bwd_data_sr"
    d, xb, cp, _, wt = prep(c, dtype, need_wt=True)
    N, cout, H, W = c.out_shape
    cin = c.cin
    gyb = nhwc_padded(c.gy_d, dtype, cout)
    bp = ctypes.c_int(0)
    nrec = L.query("fv_conv2d_sr_records", ctypes.byref(d), 1, ctypes.byref(bp))
    assert nrec == N * H * W // 64 and bp.value == 64, (nrec, bp.value)
    assert L.conv_kernel(d, dgrad=True, res=True, sr_mode=2) == X.SR_DGRAD_KIND, what + ": kernel kind"
    g = torch.Generator().manual_seed(4242)
    yb = torch.randn(N, cin, H, W, generator=g).cuda().to(dtype).contiguous(memory_format=CL)
    keep = [t.cuda() for t in (torch.randn(cin, generator=g) * 0.1, torch.rand(cin, generator=g) + 0.5,
                               torch.randn(cin, generator=g), torch.randn(cin, generator=g) * 0.3)]

    def run():
        dx = Guarded((N, cin, H, W), dtype, nhwc=True)
        rec = Guarded((nrec, 2, cin), torch.float32)
        s = L.StoreReduce(2, rec.data_ptr(), yb.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                          keep[3].data_ptr(), 0.2)
        L.call("fv_conv2d_bwd_data_sr", ctypes.byref(d), gyb.data_ptr(), cout, wt.data_ptr(), dx.data_ptr(),
               ctypes.byref(s), L.stream())
        torch.cuda.synchronize()
        dx.check_canary(what + " dx")
        rec.check_canary(what + " records")
        assert not torch.isnan(rec.t).any(), what + ": records not fully written"
        return dx.t, rec.t

    dx, _ = twice(run, what)
    assert_exact(dx, c.dx_conv, what + " dx")
