"""Every case of tests/test_conv3d_exact_gpu.py meets the conditions under which bit equality is
owed, the comparator flags what a 3-D kernel gets wrong at its 5-D coordinates, and the float64
references equal the same convolutions in fp32 bit for bit (no GPU).

The corruptions are made on the CPU the way the kernels of csrc/conv3d.hip go wrong: one voxel
off by one, one depth slice of one channel taken from the neighbouring slice (a wrong ring slot),
one (kd, kh, kw) tap of one (co, ci) pair missing, one element never written (NaN), a write past
either end of an NDHWC buffer."""
import pytest
import torch
import torch.nn.functional as F

import exact_operands as X
import exact_operands3d as X3

DTYPES = [torch.float32, torch.bfloat16]
SMALL = (1, 5, 4)            # a C = 32 case: [1, 32, 5, 4, 64]


@pytest.fixture(scope="module")
def small():
    c = X3.c32_case(*SMALL)
    assert (c.y.abs() + c.r.abs()).max() <= 256     # every corruption below stays visible after a bf16 rounding
    return c


# ---------------------------------------------------------------------------- case tables
def test_case_tables():
    assert len(X3.C32_CASES) == len({c[:3] for c in X3.C32_CASES}) == 18
    assert all(c in [k[:3] for k in X3.C32_CASES] for c in X3.C32_LARGE)
    for N, D, H, kern, ndc, dchunk, nper, ndcw in X3.C32_CASES:
        assert H % 4 == 0 and ndc * dchunk == D and N % nper == 0
        assert (kern == "dr") == (dchunk >= 4 and (dchunk + 2) % 3 == 0), (N, D, H)
        assert N * D * H * 64 * 32 * 2 < 2 ** 31            # c32_fast's byte-offset limit
    assert len(X3.DIRECT_CASES) == 6 and X3.C32_EDGE in [c[0] for c in X3.DIRECT_CASES]
    assert len(X3.GEMM_CASES) == 14 and len(X3.MFE_CASE_NAMES) == 8
    for N, cin, cout, D, H, W, k, ups in X3.GEMM_CASES.values():
        assert cin % 8 == 0 and k in (1, 3, 7) and (not ups or (H % 2 == 0 and W % 2 == 0))
    # the branches the new GEMM cases are there for (planners of csrc/conv3d_gemm.hip)
    P = lambda n: (lambda N, cin, cout, D, H, W, k, ups: N * D * H * W)(*X3.GEMM_CASES[n])   # noqa: E731
    assert X3.GEMM_CASES["16to6_k3"][2] % 4 != 0 and X3.GEMM_CASES["24to20_ups"][2] % 8 != 0
    assert -(-72 // 64) * -(-P("72to72_k3") // 128) < 256                     # 32 x 64 tiles
    assert -(-72 // 64) * -(-P("8to72_bigtile_ragged") // 128) >= 256         # 64 x 128 tiles
    assert P("8to72_bigtile_ragged") % 128 == 41
    assert P("8to8_k1_dbcap") > 262144 and -(-P("8to8_k1_dbcap") // 1024) == 264


def test_operand_values():
    c = X3.gemm_case("24to20_ups")
    for t, vals in ((c.x, {-2, -1, 0, 1, 2}), (c.w, {-1, 0, 1}), (c.gy_w, {-1, 0, 1}), (c.gy_d, {-2, -1, 0, 1, 2}),
                    (c.r, set(range(-3, 4)))):
        assert set(t.unique().tolist()) == vals
    assert set(c.b.tolist()) <= set(range(-3, 4)) and len(set(c.b.tolist())) > 3      # 20 draws
    assert c.x.shape == (1, 24, 2, 3, 5) and c.y.shape == (1, 20, 2, 6, 10) and c.dx_conv.shape == (1, 24, 2, 6, 10)
    assert torch.equal(c.x, X3.ExactCase3("24to20_ups", *X3.GEMM_CASES["24to20_ups"]).x)      # seeded per case
    assert not torch.equal(X3.gemm_case("16to8_ups").x, X3.gemm_case("16to6_k3").x[:, :, :2, :2, :2])


# ---------------------------------------------------------------------------- conditions
_WORST = {}


def _note(family, fig):
    w = _WORST.setdefault(family, {})
    for k, v in fig.items():
        w[k] = max(w.get(k, v), v)
    print(family, "worst so far:", {k: w[k] for k in sorted(w)})


@pytest.mark.parametrize("case", X3.C32_CASES, ids=X3.c32_id)
def test_c32_case_conditions(case):
    c = X3.c32_case(*case[:3])
    fig = c.check_conditions()
    print(X3.c32_id(case), fig)
    assert fig["sr_max"] <= 256 and fig["fwd_A"] <= 2 ** X.CAP_LOG2
    # the stored values and the records: integers bf16 holds; a record sums <= 33 * 64 of them
    dchunk = case[5]
    assert dchunk * 64 * 256 <= 2 ** 24
    _note("c32", fig)


@pytest.mark.parametrize("shape,ops", [(s, o) for s, _, o in X3.DIRECT_CASES], ids=[X3.direct_id(s) for s, _, _ in X3.DIRECT_CASES])
def test_direct_case_conditions(shape, ops):
    fig = X3.direct_case(shape).check_conditions(ops)
    print(X3.direct_id(shape), fig)
    assert fig["sr_max"] <= 256
    _note("direct", fig)


@pytest.mark.parametrize("name", list(X3.GEMM_CASES))
def test_gemm_case_conditions(name):
    c = X3.gemm_case(name)
    fig = c.check_conditions()
    print(name, fig)
    if c.ups:            # the second rounding of the upsample backward: four stored values, exact sum
        lo = c.dx_low(torch.bfloat16)
        assert lo.abs().max() <= 4 * c.dx_conv.abs().max() and bool((lo == torch.round(lo)).all())
    _note("gemm", fig)


def test_thinning_covers_the_store_condition():
    """a cap the dense weights miss thins them, and the sr bound is part of the same loop"""
    a = X3.ExactCase3("thin", 1, 32, 32, 3, 4, 64, sr=True)
    t = X3.ExactCase3("thin", 1, 32, 32, 3, 4, 64, sr=True, cap_log2=9)
    assert a.w_zero_share == X.ZERO_SHARE and t.w_zero_share > X.ZERO_SHARE
    assert bool(((t.w == a.w) | (t.w == 0)).all())
    assert t.check_conditions()["fwd_A"] <= 2 ** 9 < a.check_conditions()["fwd_A"]
    a.r = a.r * 100                                      # a residual the bound cannot hold
    a._fig.clear()
    with pytest.raises(AssertionError):
        a.check_conditions(("fwd",))


# ---------------------------------------------------------------------------- the comparator in 5-D
@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_copy_passes(small, dtype):
    got = small.y.to(dtype)
    assert X.mismatch_report(got, small.y) is None
    X.assert_exact(got.contiguous(memory_format=torch.channels_last_3d), small.y, "clean, NDHWC memory")
    dw, db = small.dw_db
    X.assert_exact(dw.float(), dw, "clean dw")
    X.assert_exact(db.float(), db, "clean db")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_voxel_off_by_one(small, dtype):
    at = (0, 17, 4, 3, 16)                               # the voxel right of a fragment boundary (15 | 16)
    got = small.y.to(dtype)
    got[at] += 1
    rep = X.mismatch_report(got, small.y)
    assert rep["count"] == 1 and rep["lo"] == at and rep["hi"] == at
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got, small.y, "y")
    msg = str(e.value)
    assert "(n, c, d, h, w)" in msg and str(at) in msg and "bounding box: 0..0, 17..17, 4..4, 3..3, 16..16" in msg


@pytest.mark.parametrize("dtype", DTYPES)
def test_depth_slice_of_one_channel_shifted(small, dtype):
    n, ch, d = 0, 31, 2
    got = small.y.to(dtype)
    got[n, ch, d] = got[n, ch, d + 1]                    # the slice of the wrong ring slot
    differ = (small.y[n, ch, d] != small.y[n, ch, d + 1]).nonzero()
    assert len(differ) > 64
    rep = X.mismatch_report(got, small.y)
    assert rep["count"] == len(differ)
    assert rep["lo"][:3] == rep["hi"][:3] == (n, ch, d)
    assert rep["lo"][3:] == tuple(differ.min(0).values.tolist()) and rep["hi"][3:] == tuple(differ.max(0).values.tolist())
    with pytest.raises(AssertionError, match=r"bounding box: 0\.\.0, 31\.\.31, 2\.\.2, "):
        X.assert_exact(got, small.y, "y")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropped_tap_of_one_weight_pair(small, dtype):
    co, ci = 9, 21
    w2, (kd, kh, kw) = X3.drop_tap(small.w, co, ci)
    y2 = F.conv3d(small.x, w2, small.b, 1, 1)
    want_bad = y2 != small.y
    assert want_bad.any() and not want_bad[:, :co].any() and not want_bad[:, co + 1:].any()
    rep = X.mismatch_report(y2.to(dtype), small.y)
    assert rep["count"] == int(want_bad.sum())           # a missing tap moves an output by 1 or 2: none hides
    idx = want_bad.nonzero()
    assert rep["lo"] == tuple(idx.min(0).values.tolist()) and rep["hi"] == tuple(idx.max(0).values.tolist())
    assert rep["lo"][1] == rep["hi"][1] == co
    with pytest.raises(AssertionError, match=r"\(n, c, d, h, w\)"):
        X.assert_exact(y2.to(dtype), small.y, "y")
    # ... and the data gradient through the same weights: only input channel ci moves
    xi = torch.zeros(small.in_shape, dtype=torch.float64, requires_grad=True)
    dx2 = torch.autograd.grad(F.conv3d(xi, w2, None, 1, 1), xi, small.gy_d)[0]
    rep = X.mismatch_report(dx2.to(dtype), small.dx_conv)
    assert rep is not None and rep["lo"][1] == rep["hi"][1] == ci


def test_dropped_tap_of_a_weight_gradient(small):
    dw, db = small.dw_db
    at = (9, 21, 2, 0, 1)
    assert dw[at] != 0
    got = dw.float()
    got[at] = 0
    rep = X.mismatch_report(got, dw)
    assert rep["count"] == 1 and rep["lo"] == at and rep["hi"] == at
    with pytest.raises(AssertionError, match=r"bounding box: 9\.\.9, 21\.\.21, 2\.\.2, 0\.\.0, 1\.\.1"):
        X.assert_exact(got, dw, "dw (co, ci, kd, kh, kw)")
    # one depth slice missing from the sum (a chunk's slab never added) moves nearly every element
    miss = torch.nn.grad.conv3d_weight(small.x[:, :, :4], dw.shape, small.gy_w[:, :, :4], 1, 1)
    assert X.mismatch_report(miss.float(), dw)["count"] > dw.numel() // 2
    got = db.float()
    got[5] += 1
    assert X.mismatch_report(got, db)["lo"] == (5,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_is_never_equal(small, dtype):
    at = (0, 3, 0, 3, 63)
    got = small.y.to(dtype)
    got[at] = float("nan")
    rep = X.mismatch_report(got, small.y)
    assert rep["count"] == 1 and rep["lo"] == at
    with pytest.raises(AssertionError, match=r"\(0, 3, 0, 3, 63\)"):
        X.assert_exact(got, small.y, "y")


@pytest.mark.parametrize("dtype", DTYPES)
def test_guarded_ndhwc_buffer(dtype):
    shape = (2, 6, 3, 4, 5)
    g = X.Guarded(shape, dtype, device="cpu", ndhwc=True)
    assert g.t.shape == shape and g.t.stride() == (360, 1, 120, 30, 6)
    assert torch.isnan(g.t).all()
    ref = torch.arange(720, dtype=torch.float64).view(shape) % 200
    g.t.copy_(ref)
    assert torch.equal(g.flat.double().view(2, 3, 4, 5, 6), ref.permute(0, 2, 3, 4, 1))      # NDHWC memory
    X.assert_exact(g.t, ref, "through the NCDHW view")
    g.check_canary("intact")
    n = g.flat.numel()
    for off in (X.GUARD + n, X.GUARD + n + 77, len(g.buf) - 1, X.GUARD - 1, 0):
        g = X.Guarded(shape, dtype, device="cpu", ndhwc=True)
        g.buf[off] = 0
        with pytest.raises(AssertionError, match="written outside"):
            g.check_canary("overwritten")


# ---------------------------------------------------------------------------- the premise on the CPU
@pytest.mark.parametrize("make", [lambda: X3.c32_case(1, 7, 4), lambda: X3.direct_case((1, 64, 8, 2, 3, 5)),
                                  lambda: X3.gemm_case("24to20_ups")], ids=["c32", "direct", "gemm"])
def test_fp32_convolution_equals_the_float64_reference(make):
    """The conditions, not the precision, make the result unique: the same convolutions in fp32
    (another summation order, 24-bit accumulation) give the float64 references bit for bit."""
    c = make()
    c.check_conditions()
    p = c.k // 2
    xi = X3.upsample(c.x.float()) if c.ups else c.x.float()
    y32 = F.conv3d(xi, c.w.float(), c.b.float(), 1, p)
    assert y32.dtype == torch.float32
    X.assert_exact(y32, c.y, "fp32 forward")
    z = torch.zeros_like(xi, requires_grad=True)
    dx32 = torch.autograd.grad(F.conv3d(z, c.w.float(), None, 1, p), z, c.gy_d.float())[0]
    X.assert_exact(dx32, c.dx_conv, "fp32 data gradient")
    dw32 = torch.nn.grad.conv3d_weight(xi, c.w_shape, c.gy_w.float(), 1, p)
    X.assert_exact(dw32, c.dw_db[0], "fp32 weight gradient")
    X.assert_exact(c.gy_w.float().sum((0, 2, 3, 4)), c.dw_db[1], "fp32 bias gradient")
