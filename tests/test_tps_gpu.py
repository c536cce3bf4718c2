"""GPU parity of the equivariance transform (csrc/tps.hip, ops_tps, Transform).

Frame warp: against tests/tps_reference.py in fp64 on the same inputs, rel-L2 <= max(1e-5, 3 *
`ref_dev`): 1e-5 is the project's gate for fp32-stored kernel results, `ref_dev` is the deviation
of the REFERENCE's fp32 result from the same fp64 evaluation (tests/golden/make_golden_tps.py),
and 3 x is the margin DESIGN.md section 13 gives a quantity gated by the reference's own deviation.
Against the reference's stored fp32 output: that gate plus ref_dev (both sides deviate from fp64).
Coordinate warp, its gradient and the EquivarianceLoss chain: 1e-5 against fp64 autograd of the
restatement and against the fixture.

Every test prints its measured errors (`pytest -s`); DESIGN.md section 15 has the tables.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
import tps_reference as R  # noqa: E402
from facevae_amd import _lib as L, ops, ops_tps  # noqa: E402
from golden_io import load_golden  # noqa: E402

F32, F64 = torch.float32, torch.float64
TOY = dict(down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3)      # tests/test_ckd_gpu.py
GUARD, SENT = 4096, 0xA5
_GOLD, _REF = {}, {}


def gold(case):
    if not _GOLD:
        _GOLD.update(load_golden("tps.pt"))
    return _GOLD[case]


def maxd(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


class Guarded:
    """Caller-sized buffers with a sentinel region behind them (tests/test_ckd_gpu.py)."""

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


def transform_of(gd, bs):
    """A Transform carrying the fixture's parameters (its own draws are overwritten)."""
    pts = int(gd["points_tps"]) if "points_tps" in gd else 5
    t = fv.Transform(bs, points_tps=pts)
    t.theta, t.control_params = gd["theta"].clone(), gd["control_params"].clone()
    return t, pts


def frame_ref64(name):
    """fp64 restatement of a frame case, computed once."""
    if name not in _REF:
        gd = gold("frame")[name]
        _REF[name] = R.transform_frame(gd["x"], gd["theta"], gd["control_params"], int(gd["points_tps"]))
    return _REF[name]


def frame_gate(label, y, ref64, ref_dev, stored=None):
    lim = max(1e-5, 3 * ref_dev)
    e = R.rel_l2(y, ref64)
    print(f"\n{label}: vs fp64 rel-L2 {e:.2e} (gate {lim:.2e}; reference's own deviation {ref_dev:.2e}), "
          f"max|d| {maxd(y, ref64):.2e}", end="")
    assert torch.isfinite(y).all()
    assert e <= lim, (label, e, lim)
    if stored is not None:
        es = R.rel_l2(y, stored)
        print(f"; vs reference fp32 {es:.2e} (gate {lim + ref_dev:.2e})", end="")
        assert es <= lim + ref_dev, (label, es, lim + ref_dev)
    print()


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_frame_matches_reference(name):
    gd = gold("frame")[name]
    t, _ = transform_of(gd, gd["x"].shape[0])
    y = t.transform_frame(gd["x"].cuda())
    torch.cuda.synchronize()
    assert y.dtype == F32 and tuple(y.shape) == tuple(gd["y"].shape) and y.is_contiguous() and not y.requires_grad
    frame_gate(f"frame {name} {list(gd['x'].shape)} outside {float(gd['outside']):.2f}", y, frame_ref64(name),
               float(gd["ref_dev"]), gd["y"])
    if name == "a":                                    # any float dtype in, fp32 out
        y16 = t.transform_frame(gd["x"].cuda().bfloat16())
        assert y16.dtype == F32 and torch.equal(y16, t.transform_frame(gd["x"].bfloat16().float().cuda()))


def test_frame_at_the_workload_shape():
    gd = gold("workload")
    shape = tuple(int(v) for v in gd["shape"])
    x = torch.rand(shape, generator=torch.Generator().manual_seed(int(gd["frame_seed"])))
    t, pts = transform_of(gd, shape[0])
    y = t.transform_frame(x.cuda())
    torch.cuda.synchronize()
    frame_gate(f"frame workload {list(shape)}", y, R.transform_frame(x, gd["theta"], gd["control_params"], pts),
               float(gd["ref_dev"]))


def test_identity_transform_returns_the_frame():
    x = torch.rand(1, 3, 9, 13, generator=torch.Generator().manual_seed(720)).cuda()
    t = fv.Transform(1)
    t.theta, t.control_params = torch.eye(2, 3).view(1, 2, 3), torch.zeros(1, 1, 25)
    y = t.transform_frame(x)
    d = maxd(y, x)
    print(f"\nidentity [1, 3, 9, 13]: max|d| {d:.2e} (gate 1e-5)")
    assert d <= 1e-5


def test_parameters_are_per_sample():
    """Case c with the parameters of samples 0 and 2 swapped (and the frames with them) gives the
    outputs swapped, bit for bit."""
    gd = gold("frame")["c"]
    t, _ = transform_of(gd, 3)
    x = gd["x"].cuda()
    y = t.transform_frame(x)
    perm = [2, 1, 0]
    t.theta, t.control_params = gd["theta"][perm].clone(), gd["control_params"][perm].clone()
    ys = t.transform_frame(x[perm].contiguous())
    assert torch.equal(ys, y[perm])
    assert not torch.equal(y[0], t.transform_frame(x)[0])     # and the parameters do matter


def coords_run(gd, coords=None):
    coords = gd["coords"] if coords is None else coords
    bs = gd["theta"].shape[0]
    t, _ = transform_of(gd, bs)
    c = coords.cuda().requires_grad_(True)
    out = t.warp_coordinates(c)
    out.backward(gd["g"].cuda())
    torch.cuda.synchronize()
    assert out.dtype == F32 and tuple(out.shape) == (bs, coords.shape[1], 2) and c.grad.shape == c.shape
    return out.detach(), c.grad


def gate5(name, got, ref):
    e = R.rel_l2(got, ref)
    print(f"  {name}: rel-L2 {e:.2e} (gate 1e-05)")
    assert tuple(got.shape) == tuple(ref.shape) and torch.isfinite(got).all()
    assert e <= 1e-5, (name, e)


@pytest.mark.parametrize("name", ["a", "b", "lattice"])
def test_coordinates_match_reference(name):
    gd = gold("coords")[name]
    out, d = coords_run(gd)
    o64, d64 = R.coords_with_grad(gd["coords"], gd["g"], gd["theta"], gd["control_params"], int(gd["points_tps"]))
    print(f"\ncoords {name} {list(gd['coords'].shape)}:")
    gate5("out vs fp64", out, o64)
    gate5("d_coords vs fp64", d, d64)
    gate5("out vs fixture", out, gd["out"])
    gate5("d_coords vs fixture", d, gd["d_coords"])


def test_broadcast_coordinates_sum_their_gradient():
    """[1, M, 2] coordinates warp under every sample's parameters; their gradient is the sum over bs."""
    gd = gold("coords")["b"]
    c1 = gd["coords"][:1]
    out, d = coords_run(gd, c1)
    o64, d64 = R.coords_with_grad(c1, gd["g"], gd["theta"], gd["control_params"], 5)
    assert tuple(d.shape) == (1, 15, 2) and tuple(d64.shape) == (1, 15, 2)
    print("\ncoords broadcast [1, 15, 2] -> [3, 15, 2]:")
    gate5("out vs fp64", out, o64)
    gate5("d_coords vs fp64", d, d64)


def test_equivariance_chain_matches_reference():
    gd = gold("chain")
    t, _ = transform_of(gd, 3)
    a, b = gd["kp_d"].cuda().requires_grad_(True), gd["transformed_kp"].cuda().requires_grad_(True)
    loss = fv.EquivarianceLoss()(a, t.warp_coordinates(b[:, :, :2]))
    loss.backward()
    torch.cuda.synchronize()
    print("\nequivariance chain [3, 5, 3]:")
    gate5("loss", loss, gd["loss"])
    gate5("d_kp_d", a.grad, gd["d_kp_d"])
    gate5("d_transformed_kp", b.grad, gd["d_transformed_kp"])


def test_reruns_are_bit_identical():
    gd = gold("frame")["c"]
    t, _ = transform_of(gd, 3)
    x = gd["x"].cuda()
    assert torch.equal(t.transform_frame(x), t.transform_frame(x))
    gc = gold("coords")["b"]
    (o1, d1), (o2, d2) = coords_run(gc), coords_run(gc)
    assert torch.equal(o1, o2) and torch.equal(d1, d2)


def test_outputs_stay_in_bounds(monkeypatch):
    guard = Guarded()
    monkeypatch.setattr(ops, "_empty", guard)
    for name in ("a", "c", "d"):
        gd = gold("frame")[name]
        t, _ = transform_of(gd, gd["x"].shape[0])
        y = t.transform_frame(gd["x"].cuda())
        assert R.rel_l2(y, frame_ref64(name)) <= max(1e-5, 3 * float(gd["ref_dev"]))     # the guarded buffer was used
    gc = gold("coords")["b"]
    out, d = coords_run(gc)
    assert R.rel_l2(out, gc["out"]) <= 1e-5 and R.rel_l2(d, gc["d_coords"]) <= 1e-5
    n, bad = guard.check()
    assert n == 5, n                                    # three frames, out and d_coords
    assert not bad, f"{len(bad)} of {n} buffers written past their size: {bad}"


def test_entries_reject_what_they_cannot_take():
    U = L.FV_E_UNSUPPORTED
    buf = torch.zeros(1 << 12, device="cuda")
    p, s = L.ptr(buf), L.stream()
    #                                                  n  c  h  w  pts
    for (n, c, h, w, pts) in ((1, 1, 1, 8, 5), (1, 1, 8, 1, 5), (1, 1, 8, 8, 1), (0, 1, 8, 8, 5), (1, 0, 8, 8, 5),
                              (1, 1, 8, 8, 17), (65536, 1, 8, 8, 5)):
        assert L.query("fv_tps_warp_frame_fwd", p, p, p, n, c, h, w, pts, p, s) == U, (n, c, h, w, pts)
    for (n, m, pts) in ((0, 4, 5), (1, 0, 5), (1, 4, 1), (1, 4, 17)):
        assert L.query("fv_tps_warp_coords_fwd", p, p, p, n, m, pts, p, s) == U, (n, m, pts)
        assert L.query("fv_tps_warp_coords_bwd", p, p, p, p, n, m, pts, p, s) == U, (n, m, pts)
    th, cp = torch.eye(2, 3).view(1, 2, 3).cuda(), torch.zeros(1, 1, 25).cuda()
    with pytest.raises(L.FaceVAELibError, match="at least 2"):
        ops_tps.warp_frame(torch.zeros(1, 3, 1, 8, device="cuda"), th, cp, 5)
    with pytest.raises(L.FaceVAELibError, match="at least 2"):
        ops_tps.warp_frame(torch.zeros(1, 3, 8, 1, device="cuda"), th, cp, 5)
    with pytest.raises(L.FaceVAELibError, match="points_tps"):
        ops_tps.warp_frame(torch.zeros(1, 3, 8, 8, device="cuda"), th, torch.zeros(1, 1, 1).cuda(), 1)
    with pytest.raises(L.FaceVAELibError, match="N must be"):
        ops_tps.warp_frame(torch.zeros(0, 3, 8, 8, device="cuda"), th[:0], cp[:0], 5)
    with pytest.raises(L.FaceVAELibError, match="M must be"):
        ops_tps.WarpCoordsFn.apply(torch.zeros(1, 0, 2, device="cuda"), th, cp, 5)
    torch.cuda.synchronize()


def test_transform_wires_into_the_equivariance_term():
    """transform_frame(d) -> CKD -> warp_coordinates(kp[:, :, :2]) -> EquivarianceLoss against a
    second CKD output (trainer.py:271-272, 289, 310-312): the loss reaches CKD.out_conv."""
    torch.manual_seed(7)
    ckd = fv.CKD(False, **TOY).cuda().train()
    d = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(8)).cuda()
    t = fv.Transform(2, 0.3, 0.05)
    td = t.transform_frame(d)
    assert tuple(td.shape) == (2, 3, 64, 96) and td.dtype == F32 and not td.requires_grad
    kp_d = ckd(d)
    transformed_kp = ckd(td)
    reverse_kp = t.warp_coordinates(transformed_kp[:, :, :2])
    loss = fv.EquivarianceLoss()(kp_d, reverse_kp)
    loss.backward()
    torch.cuda.synchronize()
    gw = ckd.out_conv.weight.grad
    assert torch.isfinite(loss) and gw is not None and torch.isfinite(gw).all() and gw.abs().sum().item() > 0
    print(f"\nequivariance term on the toy CKD: loss {loss.item():.4f}, |d out_conv.weight| {gw.abs().sum().item():.3e}")
