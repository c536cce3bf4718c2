"""The exact-operand comparator cannot pass a wrong result, and every case of
tests/test_conv_exact_gpu.py meets the conditions under which equality is owed (no GPU).

The comparator is run on a float64 reference output and on copies corrupted on the CPU the way
a kernel goes wrong: one element off by one, one border column of one channel shifted, one tap
of one (co, ci) pair missing, one element never written, a write past the end."""
import pytest
import torch
import torch.nn.functional as F

import exact_operands as X

DTYPES = [torch.float32, torch.bfloat16]
SMALL = ((3, 32, 64, 12, 10, False, False), 2)


@pytest.fixture(scope="module")
def small():
    c = X.conv_case(*SMALL)
    assert c.y.abs().max() < 128          # every corruption below stays visible after a bf16 rounding
    return c


@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_copy_passes(small, dtype):
    got = small.y.to(dtype)
    assert X.mismatch_report(got, small.y) is None
    X.assert_exact(got, small.y, "clean")
    X.assert_exact(got.contiguous(memory_format=torch.channels_last), small.y, "clean, NHWC memory")


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_element_off_by_one(small, dtype):
    at = (1, 37, 5, 9)
    got = small.y.to(dtype)
    got[at] += 1
    rep = X.mismatch_report(got, small.y)
    assert rep["count"] == 1 and rep["lo"] == at and rep["hi"] == at
    assert rep["first"] == [(at, small.y[at].item() + 1, small.y[at].item())]
    with pytest.raises(AssertionError) as e:
        X.assert_exact(got, small.y, "y")
    msg = str(e.value)
    assert "1 of " in msg and str(at) in msg and "bounding box: 1..1, 37..37, 5..5, 9..9" in msg


@pytest.mark.parametrize("dtype", DTYPES)
def test_border_column_of_one_channel_shifted(small, dtype):
    n, c = 0, 63
    W = small.y.shape[3]
    got = small.y.to(dtype)
    got[n, c, :, W - 1] = got[n, c, :, W - 2]
    differ = (small.y[n, c, :, W - 1] != small.y[n, c, :, W - 2]).nonzero().flatten().tolist()
    assert len(differ) > 1
    rep = X.mismatch_report(got, small.y)
    assert rep["count"] == len(differ)
    assert rep["lo"] == (n, c, differ[0], W - 1) and rep["hi"] == (n, c, differ[-1], W - 1)
    assert [f[0] for f in rep["first"]] == [(n, c, h, W - 1) for h in differ[:10]]
    with pytest.raises(AssertionError):
        X.assert_exact(got, small.y, "y")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropped_tap_of_one_weight_pair(small, dtype):
    co, ci = 17, 5
    r, s = [int(i) for i in small.w[co, ci].nonzero()[0]]
    w2 = small.w.clone()
    w2[co, ci, r, s] = 0
    y2 = F.conv2d(small.x, w2, small.b, padding=1)
    want_bad = (y2 != small.y)
    assert want_bad.any() and not want_bad[:, :co].any() and not want_bad[:, co + 1:].any()
    rep = X.mismatch_report(y2.to(dtype), small.y)
    assert rep["count"] == int(want_bad.sum())          # a missing tap moves an output by 1 or 2: none hides
    idx = want_bad.nonzero()
    assert rep["lo"] == tuple(idx.min(0).values.tolist()) and rep["hi"] == tuple(idx.max(0).values.tolist())
    assert rep["lo"][1] == rep["hi"][1] == co
    # ... and the same for the weight gradient: one tap of one pair left at zero
    dw, _ = small.dw_db
    got = dw.float()
    assert dw[co, ci, r, s] != 0
    got[co, ci, r, s] = 0
    rep = X.mismatch_report(got, dw)
    assert rep["count"] == 1 and rep["lo"] == (co, ci, r, s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_is_never_equal(small, dtype):
    at = (0, 0, 11, 0)
    got = small.y.to(dtype)
    got[at] = float("nan")
    rep = X.mismatch_report(got, small.y)
    assert rep["count"] == 1 and rep["lo"] == at
    want = small.y.clone()
    want[at] = float("nan")                               # the same NaN on both sides is still a mismatch
    assert X.mismatch_report(got, want)["count"] == 1
    with pytest.raises(AssertionError):
        X.assert_exact(got, small.y, "y")


def test_rounding_is_to_nearest_even():
    want = torch.tensor([257.0, 259.0, 258.0, 1.0 + 2.0 ** -8, 3.0], dtype=torch.float64)
    assert X.mismatch_report(torch.tensor([256.0, 260.0, 258.0, 1.0, 3.0], dtype=torch.bfloat16), want) is None
    rep = X.mismatch_report(torch.tensor([258.0, 260.0, 258.0, 1.0, 3.0], dtype=torch.bfloat16), want)   # 257 rounded up
    assert rep["count"] == 1 and rep["lo"] == (0,)
    assert X.mismatch_report(want.float(), want) is None


@pytest.mark.parametrize("dtype", DTYPES)
def test_guarded_buffer(dtype):
    shape = (2, 8, 3, 5)
    g = X.Guarded(shape, dtype, device="cpu", nhwc=True)
    assert g.t.shape == shape and g.t.is_contiguous(memory_format=torch.channels_last)
    assert torch.isnan(g.t).all()
    g.t.copy_(torch.ones(shape))
    assert bool((g.flat == 1).all())
    g.check_canary("intact")
    for off in (X.GUARD + g.flat.numel(), X.GUARD + g.flat.numel() + 77, len(g.buf) - 1, X.GUARD - 1, 0):
        g = X.Guarded(shape, dtype, device="cpu")
        g.buf[off] = 0
        with pytest.raises(AssertionError, match="written outside"):
            g.check_canary("overwritten")
    g = X.Guarded(shape, dtype, device="cpu")
    g.buf[X.GUARD + g.flat.numel()] = float("nan")
    with pytest.raises(AssertionError, match="written outside"):
        g.check_canary("NaN in the canary")


def test_operand_values():
    c = X.conv_case((3, 64, 128, 16, 16, False, True), 2)
    for t, vals in ((c.x, {-2, -1, 0, 1, 2}), (c.w, {-1, 0, 1}), (c.gy_w, {-1, 0, 1}), (c.gy_d, {-2, -1, 0, 1, 2}),
                    (c.b, set(range(-3, 4))), (c.sc, {0.5, 1, 2}), (c.sh, {-1, 0, 1})):
        assert set(t.unique().tolist()) == vals
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    xi = X.conv_input(c.x, False, c.pro_fwd)
    assert torch.equal(xi.to(torch.bfloat16).double(), xi) and xi.abs().max() == 5
    assert torch.equal(X.conv_case((3, 64, 128, 16, 16, False, True), 2).x, X.ExactCase(c.case, 2).x)   # seeded per case
    assert not torch.equal(c.x[0], X.conv_case(c.case, 3).x[0])


def test_a_lower_cap_thins_the_operands():
    case = (3, 64, 24, 8, 16, False, False)
    c, t = X.ExactCase(case, 2), X.ExactCase(case, 2, cap_log2=9)
    assert c.w_zero_share == X.ZERO_SHARE and t.w_zero_share > X.ZERO_SHARE
    assert bool(((t.w == c.w) | (t.w == 0)).all())       # thinning only clears entries
    assert t.check_conditions()["fwd_A"] <= 2 ** 9 < c.check_conditions()["fwd_A"]


def test_a_case_that_breaks_a_condition_fails():
    c = X.ExactCase((3, 16, 32, 7, 9, False, False), 2)
    c.w, c.gy_w                                           # drawn for 2^22 ...
    c.cap = 2.0 ** 5                                      # ... and held to a cap they do not meet
    with pytest.raises(AssertionError):
        c.check_conditions(("fwd",))
    with pytest.raises(AssertionError):
        c.check_conditions(("wgrad",))


def _ops(cn):
    return tuple(op for op, lst in (("fwd", X.FWD_LIST), ("dgrad", X.DGRAD_LIST), ("wgrad", X.WGRAD_LIST)) if cn in lst)


ALL_CONV = sorted(set(X.FWD_LIST) | set(X.WGRAD_LIST), key=lambda cn: (X.CONV_CASES.index(cn[0]), cn[1]))


def test_case_lists():
    assert len(X.CONV_CASES) == len(set(X.CONV_CASES)) == 34
    assert len(X.FWD_LIST) == 32 + 12 and len(X.WGRAD_LIST) == 31 + 12 + 2
    assert all(c in X.CONV_CASES for c in X.N13_CASES + X.FULL_SIZE_UP + [X.C7_BAND_CASE, X.SR_DGRAD_CASE])
    assert all(_ops((c, 2)) == ("wgrad",) for c in X.FULL_SIZE_UP) and _ops((X.C7_BAND_CASE, 2)) == ("fwd",)


@pytest.mark.parametrize("cn", ALL_CONV, ids=X.case_id)
def test_conv_case_conditions(cn):
    fig = X.conv_case(*cn).check_conditions(_ops(cn))
    print(X.case_id(cn), fig)


# ---------------------------------------------------------------- kernel kinds (library queries, no GPU)
def _desc(case, N, dtype, fwd):
    """the descriptor tests/test_conv_exact_gpu.py launches a case with (prep; the forward stores NCHW
    fp32 when cout % 4 != 0)"""
    import fvamd  # noqa: F401
    from facevae_amd import ops
    k, cin, cout, H, W, ups, pro = case
    ho, wo = (2 * H, 2 * W) if ups else (H, W)
    return ops.desc(dtype, N, ho, wo, ops.pad_pow2(cin), cin, cout, cout, k, ups, pro, X.FWD_SLOPE if pro and fwd else 0.0,
                    False, int(fwd and cout % 4 != 0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cn", ALL_CONV, ids=X.case_id)
def test_conv_case_kinds(cn, dtype):
    """every case's forward and data gradient take the kernel kind the table names"""
    from facevae_amd import _lib as L
    case, N = cn
    if cn in X.FWD_LIST:
        assert L.conv_kernel(_desc(case, N, dtype, True), stats=True) == X.conv_kinds(case, dtype)[0]
    else:
        assert X.CONV_KINDS[case][0] is None
    if cn in X.DGRAD_LIST:
        assert L.conv_kernel(_desc(case, N, dtype, False), dgrad=True) == X.conv_kinds(case, dtype)[1]
    else:
        assert X.CONV_KINDS[case][1] is None


def test_store_pass_kinds():
    import fvamd  # noqa: F401
    from facevae_amd import _lib as L, ops
    assert set(X.SR_KINDS) == set(X.SR_CASES)
    for name, (cin, cout, N, H, W) in X.SR_CASES.items():
        d = ops.desc(torch.bfloat16, N, H, W, cin, cin, cout, cout, 3)
        assert L.conv_kernel(d, res=True, sr_mode=1) == X.SR_KINDS[name], name
    assert L.conv_kernel(_desc(X.SR_DGRAD_CASE, 1, torch.bfloat16, False), dgrad=True, res=True, sr_mode=2) == X.SR_DGRAD_KIND


def test_every_kernel_kind_has_a_case():
    """a condition, not a measurement: each FV_CONVK_* kind is the expected kind of some case"""
    from facevae_amd import _lib as L
    have = {k for cn in ALL_CONV for k in X.CONV_KINDS[cn[0]]} | set(X.SR_KINDS.values()) | {X.SR_DGRAD_KIND}
    assert have - {None} == set(L.CONV_KERNELS)


@pytest.mark.parametrize("case", X.S2_CASES, ids=X.case_id)
def test_s2_case_conditions(case):
    print(case, X.s2_case(case).check_conditions())


@pytest.mark.parametrize("name", list(X.SR_CASES))
def test_sr_case_conditions(name):
    c = X.sr_case(name)
    fig = c.check_conditions(("fwd",))
    print(name, "weight zero share", c.w_zero_share, fig)
    assert fig["sr_max"] <= 256
    out = c.y + c.r                                       # what the launch stores: exact in bf16
    assert torch.equal(out.to(torch.bfloat16).double(), out)
    # the record totals of <= 64 pixels each are exact in fp32
    assert 64 * 256 <= 2 ** 24 and 64 * 256 ** 2 <= 2 ** 24
