"""Exact-operand parity of the 3-D conv kernels on the GPU: every output of every launch must
equal the float64 reference BIT FOR BIT after one rounding to the output type (DESIGN.md
section 20; the idea, conditions and comparator are those of section 19 and
tests/exact_operands.py, the cases and references those of tests/exact_operands3d.py).

Outputs are pre-filled with NaN between two canary regions (an element never written and a
write outside the buffer both fail), the weight-gradient workspaces are pre-filled with NaN,
and every launch runs twice into fresh buffers and must repeat bit for bit.  Through the public
entry points only, called as facevae_amd/ops3d.py calls them:

  C = 32 fast path   fv_conv3d_weight_prep + fv_conv3d_fwd in its four epilogue variants (plain,
                     bias + residual, statistics, statistics + residual), fv_conv3d_bwd_data,
                     fv_conv3d_bwd_weight; before a launch the case's plan (forward kernel and
                     depth chunks, weight-gradient blocks) is asserted through the public queries,
                     so a case cannot silently stop reaching its branch
  direct kernels     the same entry points in fp32 and off the fast shape (plain, bias + residual)
  weight prep        fv_conv3d_weight_prep_multi with 17 weights against fv_conv3d_weight_prep
  general GEMM       fv_conv3dg_weight_prep, _fwd, _bwd_data (+ _upsample_bwd), _bwd_weight

Every comparison is an equality.  The one bound is that of section 19 on a statistics record's
sum of squares, a fp32 sum of block_pixels non-negative terms: (block_pixels + 1) * 2^-23
relative (with |y| <= 256 the squares themselves are exact; measured values are printed)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
from facevae_amd import _lib as L  # noqa: E402
from facevae_amd import ops3d  # noqa: E402

import exact_operands3d as X3  # noqa: E402
from exact_operands import Guarded, assert_exact  # noqa: E402

CL3 = torch.channels_last_3d
BF16, F32 = torch.bfloat16, torch.float32
C3W_NS, C3W_SLAB = 16, 32 * 864 + 32          # csrc/conv3d.hip: reduce partials, floats per block slab


def tname(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def twice(run, what):
    """run() -> tuple of tensors, launched twice into fresh buffers: the results repeat bit for bit"""
    a, b = run(), run()
    for i, (u, v) in enumerate(zip(a, b)):
        assert same_bits(u, v), f"{what}: output {i} differs between two launches"
    return a


def dev(t, dtype=F32):
    return t.to(dtype).cuda().contiguous()


def ndhwc(t, dtype):
    """float64 NCDHW on the CPU -> NDHWC on the GPU"""
    return t.to(dtype).cuda().contiguous(memory_format=CL3)


def nan_ws(nbytes):
    assert nbytes % 4 == 0
    return torch.full((max(nbytes // 4, 1),), float("nan"), dtype=F32, device="cuda")


# ------------------------------------------------------------------------ fv_conv3d_* (conv3d.hip)
def prep3(c, dtype):
    d = ops3d.desc3(dtype, c.N, c.D, c.H, c.W, c.cin, c.cout)
    nbytes = L.query("fv_conv3d_wk_bytes", ctypes.byref(d))
    assert nbytes > 0
    wk = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    wt = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    wc = dev(c.w)
    L.call("fv_conv3d_weight_prep", ctypes.byref(d), wc.data_ptr(), wk.data_ptr(), wt.data_ptr(), L.stream())
    return d, wk, wt


def check_records(part, nb, bp, want, what):
    """records [nb][2][cout], summed in float64 on the host, against the reference `want`"""
    cout = want.shape[1]
    got = part.view(nb, 2, cout).double().sum(0).cpu()
    f = want.permute(1, 0, 2, 3, 4).reshape(cout, -1)
    assert_exact(got[0], f.sum(1), f"{what}: record sums per channel")
    q = (f * f).sum(1)
    e = ((got[1] - q).abs() / q).max().item()
    bound = (bp + 1) * 2.0 ** -23
    print(f"{what}: {nb} records of {bp} voxels, sum of squares rel {e:.3e} (bound {bound:.3e})")
    assert e <= bound, f"{what}: record sum of squares off by {e:.3e} relative, bound {bound:.3e}"


def fwd3_variants(c, d, wk, dtype, what, nb, bp):
    """fv_conv3d_fwd per epilogue variant: (bias, residual, records) -> reference"""
    xb = ndhwc(c.x, dtype)
    rb = ndhwc(c.r, dtype)
    bias = dev(c.b)
    variants = [("plain", False, False, False, c.conv), ("bias + residual", True, True, False, c.y + c.r)]
    if nb:
        variants += [("statistics", True, False, True, c.y), ("statistics + residual", True, True, True, c.y + c.r)]
    for name, use_b, use_r, use_s, want in variants:
        w2 = f"{what} [{name}]"

        def run():
            y = Guarded(c.out_shape, dtype, ndhwc=True)
            part = Guarded((nb * 2 * c.cout,), F32) if use_s else None
            L.call("fv_conv3d_fwd", ctypes.byref(d), xb.data_ptr(), wk.data_ptr(), L.ptr(bias if use_b else None),
                   L.ptr(rb if use_r else None), y.data_ptr(), L.ptr(part), L.stream())
            torch.cuda.synchronize()
            y.check_canary(w2 + " y")
            if use_s:
                part.check_canary(w2 + " records")
                return y.t, part.flat
            return (y.t,)

        outs = twice(run, w2)
        assert_exact(outs[0], want, w2 + " y")
        if use_s:
            check_records(outs[1], nb, bp, want, w2)


def dgrad3(c, d, wt, dtype, what):
    gyb = ndhwc(c.gy_d, dtype)

    def run():
        dx = Guarded(c.in_shape, dtype, ndhwc=True)
        L.call("fv_conv3d_bwd_data", ctypes.byref(d), gyb.data_ptr(), wt.data_ptr(), dx.data_ptr(), L.stream())
        torch.cuda.synchronize()
        dx.check_canary(what + " dx")
        return (dx.t,)

    (dx,) = twice(run, what)
    assert_exact(dx, c.dx_conv, what + " dx")


def wgrad3(c, d, dtype, what):
    xb, gyb = ndhwc(c.x, dtype), ndhwc(c.gy_w, dtype)
    nws = L.query("fv_conv3d_wgrad_ws_bytes", ctypes.byref(d))

    def run():
        ws = nan_ws(nws) if nws else None
        dw = Guarded(c.w_shape, F32)
        db = Guarded((c.cout,), F32)
        L.call("fv_conv3d_bwd_weight", ctypes.byref(d), xb.data_ptr(), gyb.data_ptr(), dw.data_ptr(), db.data_ptr(),
               L.ptr(ws), L.stream())
        torch.cuda.synchronize()
        dw.check_canary(what + " dw")
        db.check_canary(what + " db")
        return dw.t, db.t

    dw, db = twice(run, what)
    dw_ref, db_ref = c.dw_db
    assert_exact(dw, dw_ref, what + " dw (co, ci, kd, kh, kw)")
    assert_exact(db, db_ref, what + " db")


def c32_plan(case):
    """the descriptor of a C = 32 case, its plan asserted through the public queries"""
    N, D, H, kern, ndc, dchunk, nper, ndcw = case
    d = ops3d.desc3(BF16, N, D, H, 64, 32, 32)
    bp = L.query("fv_conv3d_stats_block_pixels", ctypes.byref(d))
    nb = L.query("fv_conv3d_stats_blocks", ctypes.byref(d))
    assert bp == dchunk * 64, f"{X3.c32_id(case)}: depth chunk of {bp // 64}, the case is there for {dchunk}"
    assert nb == N * H * ndc, f"{X3.c32_id(case)}: {nb} records, the case is there for {ndc} depth chunks"
    assert ndc * dchunk == D and (kern == "dr") == (dchunk >= 4 and (dchunk + 2) % 3 == 0)
    nblk = (N // nper) * (H // 4) * ndcw
    nws = L.query("fv_conv3d_wgrad_ws_bytes", ctypes.byref(d))
    assert nws == (nblk + C3W_NS) * C3W_SLAB * 4, (
        f"{X3.c32_id(case)}: weight-gradient workspace of {nws} bytes, the case is there for {nblk} blocks "
        f"({nper} images per block, {ndcw} depth chunks)")
    return d, nb, bp


@pytest.mark.parametrize("case", X3.C32_CASES, ids=X3.c32_id)
def test_c32_fwd_exact(case):
    c = X3.c32_case(*case[:3])
    what = f"c32 fwd {X3.c32_id(case)} ({case[3]}, {case[4]} x {case[5]})"
    _, nb, bp = c32_plan(case)
    d, wk, _ = prep3(c, BF16)
    fwd3_variants(c, d, wk, BF16, what, nb, bp)


@pytest.mark.parametrize("case", X3.C32_CASES, ids=X3.c32_id)
def test_c32_dgrad_exact(case):
    c = X3.c32_case(*case[:3])
    c32_plan(case)
    d, _, wt = prep3(c, BF16)
    dgrad3(c, d, wt, BF16, f"c32 dgrad {X3.c32_id(case)} ({case[3]}, {case[4]} x {case[5]})")


@pytest.mark.parametrize("case", X3.C32_CASES, ids=X3.c32_id)
def test_c32_wgrad_exact(case):
    c = X3.c32_case(*case[:3])
    d, _, _ = c32_plan(case)
    wgrad3(c, d, BF16, f"c32 wgrad {X3.c32_id(case)} ({case[6]} images per block, {case[7]} depth chunks)")


DIRECT = [(shape, dt, ops) for shape, dts, ops in X3.DIRECT_CASES for dt in dts]


@pytest.mark.parametrize("shape,dtype,ops", DIRECT, ids=[f"{X3.direct_id(s)}_{tname(dt)}" for s, dt, _ in DIRECT])
def test_direct_exact(shape, dtype, ops):
    c = X3.direct_case(shape)
    what = f"direct {X3.direct_id(shape)} {tname(dtype)}"
    d, wk, wt = prep3(c, dtype)
    # off the fast path: no records, no weight-gradient workspace
    assert L.query("fv_conv3d_stats_blocks", ctypes.byref(d)) == 0, what
    assert L.query("fv_conv3d_wgrad_ws_bytes", ctypes.byref(d)) == 0, what
    assert L.query("fv_conv3d_wk_bytes", ctypes.byref(d)) == 27 * c.cin * c.cout * 4, what
    fwd3_variants(c, d, wk, dtype, what + " fwd", 0, 0)
    if "dgrad" in ops:
        dgrad3(c, d, wt, dtype, what + " dgrad")
    wgrad3(c, d, dtype, what + " wgrad")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=tname)
def test_weight_prep_multi_matches_single(dtype):
    """17 weights, one more than a launch of fv_conv3d_weight_prep_multi takes (W3P_MAX = 16): the
    second launch of its loop runs.  bf16 at the fast shape: the MFMA layouts; fp32: the direct
    kernels' layouts."""
    n = 17
    d = ops3d.desc3(dtype, 1, 2, 4, 64, 32, 32)
    nbytes = L.query("fv_conv3d_wk_bytes", ctypes.byref(d))
    assert nbytes == 27 * 32 * 32 * (2 if dtype == BF16 else 4)
    ne = 27 * 32 * 32
    g = torch.Generator().manual_seed(1717)
    ws = [torch.randn(32, 32, 3, 3, 3, generator=g).cuda().contiguous() for _ in range(n)]
    single = []
    for w in ws:
        wk, wt = Guarded((ne,), dtype), Guarded((ne,), dtype)
        L.call("fv_conv3d_weight_prep", ctypes.byref(d), w.data_ptr(), wk.data_ptr(), wt.data_ptr(), L.stream())
        single.append((wk, wt))
    multi = [(Guarded((ne,), dtype), Guarded((ne,), dtype)) for _ in ws]
    P = ctypes.c_void_p * n
    L.call("fv_conv3d_weight_prep_multi", ctypes.byref(d), n, P(*[w.data_ptr() for w in ws]),
           P(*[a.data_ptr() for a, _ in multi]), P(*[b.data_ptr() for _, b in multi]), L.stream())
    torch.cuda.synchronize()
    for i, ((sk, st), (mk, mt)) in enumerate(zip(single, multi)):
        for s, m, nm in ((sk, mk, "wk"), (st, mt, "wt")):
            s.check_canary(f"weight_prep {nm}[{i}]")
            m.check_canary(f"weight_prep_multi {nm}[{i}]")
            assert not torch.isnan(s.flat).any(), f"weight_prep {nm}[{i}] not fully written"
            assert same_bits(s.flat, m.flat), f"weight_prep_multi {nm}[{i}] differs from fv_conv3d_weight_prep"
    # the forward layout holds the weights themselves: [t][co][ci] (fast) or [t][ci][co] (direct)
    w0 = ws[0].permute(2, 3, 4, 0, 1).reshape(27, 32, 32)
    want = w0 if dtype == BF16 else w0.transpose(1, 2)
    assert_exact(multi[0][0].flat.view(27, 32, 32), want.double(), "weight_prep_multi wk[0]")


# ------------------------------------------------------------------------ fv_conv3dg_* (conv3d_gemm.hip)
def test_gemm_table_holds_the_mfe_cases():
    import test_mfe_gpu
    assert {k: X3.GEMM_CASES[k] for k in X3.MFE_CASE_NAMES} == test_mfe_gpu.CASES


@pytest.mark.parametrize("dtype", [BF16, F32], ids=tname)
@pytest.mark.parametrize("name", list(X3.GEMM_CASES))
def test_conv3dg_exact(name, dtype):
    c = X3.gemm_case(name)
    what = f"conv3dg {name} {tname(dtype)}"
    d = ops3d.descg(dtype, c.N, c.D, c.H, c.W, c.cin, c.cout, c.k, c.ups)
    L.call("fv_conv3dg_check", ctypes.byref(d))
    wk = torch.empty(L.query("fv_conv3dg_wk_bytes", ctypes.byref(d)), dtype=torch.uint8, device="cuda")
    wt = torch.empty(L.query("fv_conv3dg_wt_bytes", ctypes.byref(d)), dtype=torch.uint8, device="cuda")
    wc = dev(c.w)
    L.call("fv_conv3dg_weight_prep", ctypes.byref(d), wc.data_ptr(), wk.data_ptr(), wt.data_ptr(), L.stream())
    xb, bias = ndhwc(c.x, dtype), dev(c.b)
    gyd, gyw = ndhwc(c.gy_d, dtype), ndhwc(c.gy_w, dtype)
    nws = L.query("fv_conv3dg_wgrad_ws_bytes", ctypes.byref(d))
    hi_shape = (c.N, c.cin, c.D, c.H, c.W)

    def run_fwd():
        y = Guarded(c.out_shape, dtype, ndhwc=True)
        L.call("fv_conv3dg_fwd", ctypes.byref(d), xb.data_ptr(), wk.data_ptr(), bias.data_ptr(), y.data_ptr(), L.stream())
        torch.cuda.synchronize()
        y.check_canary(what + " y")
        return (y.t,)

    def run_dgrad():
        dx = Guarded(hi_shape, dtype, ndhwc=True)
        L.call("fv_conv3dg_bwd_data", ctypes.byref(d), gyd.data_ptr(), wt.data_ptr(), dx.data_ptr(), L.stream())
        outs = [dx]
        if c.ups:
            lo = Guarded(c.in_shape, dtype, ndhwc=True)
            L.call("fv_conv3dg_upsample_bwd", ctypes.byref(d), dx.data_ptr(), lo.data_ptr(), L.stream())
            outs.append(lo)
        torch.cuda.synchronize()
        for o in outs:
            o.check_canary(what + " dx")
        return tuple(o.t for o in outs)

    def run_wgrad():
        ws = nan_ws(nws)
        dw, db = Guarded(c.w_shape, F32), Guarded((c.cout,), F32)
        L.call("fv_conv3dg_bwd_weight", ctypes.byref(d), xb.data_ptr(), gyw.data_ptr(), dw.data_ptr(), db.data_ptr(),
               ws.data_ptr(), L.stream())
        torch.cuda.synchronize()
        dw.check_canary(what + " dw")
        db.check_canary(what + " db")
        return dw.t, db.t

    (y,) = twice(run_fwd, what + " fwd")
    assert_exact(y, c.y, what + " y")
    outs = twice(run_dgrad, what + " dgrad")
    assert_exact(outs[0], c.dx_conv, what + " dx")
    if c.ups:
        assert_exact(outs[1], c.dx_low(dtype), what + " dx after fv_conv3dg_upsample_bwd")
    dw, db = twice(run_wgrad, what + " wgrad")
    assert_exact(dw, c.dw_db[0], what + " dw (co, ci, kd, kh, kw)")
    assert_exact(db, c.dw_db[1], what + " db")
