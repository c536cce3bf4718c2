"""CPU checks of the equivariance transform: the constructor's random draws and control lattice
against the reference (tests/golden/tps.pt, bit for bit), the forms that must raise, and the
restatement tests/tps_reference.py, which the GPU tests compare the kernels with in fp64, pinned
in fp32 against every reference result of the fixture.

The restatement's gate.  Run in fp32 it repeats the reference's operations on the same inputs, so
it differs from the reference's fp32 result by less than either differs from exact arithmetic:
rel-L2 <= 2 * `ref_dev` (the fixture's deviation of the reference from fp64), floored at 1e-6, a few
fp32 roundings, where ref_dev itself is only a handful of ulps."""
import pytest
import torch

import fvamd  # noqa: F401
import facevae_amd as fv
import tps_reference as R
from golden_io import load_golden

F32 = torch.float32
_GOLD = {}


def gold(case):
    if not _GOLD:
        _GOLD.update(load_golden("tps.pt"))
    return _GOLD[case]


def pin(got, want, ref_dev):
    e, lim = R.rel_l2(got, want), max(1e-6, 2 * float(ref_dev))
    assert e <= lim, (e, lim)


@pytest.mark.parametrize("name", ["s7", "s11"])
def test_constructor_draws_match_reference(name):
    gd = gold("ctor")[name]
    bs, pts = int(gd["bs"]), int(gd["points_tps"])
    torch.manual_seed(int(gd["seed"]))
    t = fv.Transform(bs) if pts == 5 else fv.Transform(bs, points_tps=pts)
    assert t.bs == bs
    for k in ("theta", "control_params", "control_points"):
        v = getattr(t, k)
        assert v.dtype == F32 and v.device.type == "cpu" and tuple(v.shape) == tuple(gd[k].shape), k
        assert torch.equal(v, gd[k]), k
    assert tuple(t.theta.shape) == (bs, 2, 3) and tuple(t.control_params.shape) == (bs, 1, pts * pts)
    assert tuple(t.control_points.shape) == (1, pts, pts, 2)


def test_constructor_takes_the_reference_sigmas():
    torch.manual_seed(3)
    a = fv.Transform(4, 0.8, 0.05, 3)
    torch.manual_seed(3)
    noise = torch.normal(mean=0, std=0.8 * torch.ones([4, 2, 3]))
    cp = torch.normal(mean=0, std=0.05 * torch.ones([4, 1, 9]))
    assert torch.equal(a.theta, noise + torch.eye(2, 3).view(1, 2, 3)) and torch.equal(a.control_params, cp)


def test_coordinate_grid_2d():
    from facevae_amd import warp
    for name in ("s7", "s11"):
        gd = gold("ctor")[name]
        pts = int(gd["points_tps"])
        assert torch.equal(warp.make_coordinate_grid_2d((pts, pts)).unsqueeze(0), gd["control_points"])
    g = warp.make_coordinate_grid_2d((3, 5))
    assert tuple(g.shape) == (3, 5, 2) and g.dtype == F32
    assert g[0, 0].tolist() == [-1.0, -1.0] and g[0, 4].tolist() == [1.0, -1.0] and g[2, 0].tolist() == [-1.0, 1.0]
    assert torch.equal(g, R.grid_2d(3, 5, F32))            # x along W first, as the 3-D grid


def test_cpu_tensors_are_rejected():
    t = fv.Transform(2)
    with pytest.raises(RuntimeError, match="GPU only"):
        t.transform_frame(torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        t.warp_coordinates(torch.zeros(2, 5, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        t.warp_coordinates(torch.zeros(1, 5, 2))
    from facevae_amd import ops_tps
    with pytest.raises(RuntimeError, match="GPU only"):
        ops_tps.warp_frame(torch.zeros(2, 3, 8, 8), t.theta, t.control_params, 5)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops_tps.WarpCoordsFn.apply(torch.zeros(2, 5, 2), t.theta, t.control_params, 5)


def test_wrong_arguments_raise_value_errors():
    t = fv.Transform(2)
    with pytest.raises(ValueError, match="requires grad"):
        t.transform_frame(torch.zeros(2, 3, 8, 8, requires_grad=True))
    with pytest.raises(ValueError, match=r"\[2, C, H, W\]"):
        t.transform_frame(torch.zeros(3, 3, 8, 8))
    with pytest.raises(ValueError, match=r"\[2, C, H, W\]"):
        t.transform_frame(torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match=r"\[1, M, 2\]"):
        t.warp_coordinates(torch.zeros(3, 5, 2))
    with pytest.raises(ValueError, match=r"\[1, M, 2\]"):
        t.warp_coordinates(torch.zeros(2, 5, 3))
    t.control_params = torch.zeros(2, 1, 9)                # no longer the 5 x 5 lattice's
    with pytest.raises(ValueError, match="control lattice"):
        t.warp_coordinates(torch.zeros(2, 5, 2))


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_restatement_reproduces_the_reference_frames(case):
    gd = gold("frame")[case]
    pts = int(gd["points_tps"])
    y = R.transform_frame(gd["x"], gd["theta"], gd["control_params"], pts, F32)
    assert y.dtype == F32 and tuple(y.shape) == tuple(gd["y"].shape)
    pin(y, gd["y"], gd["ref_dev"])
    h, w = gd["x"].shape[2:]
    outside = R.outside_share(h, w, gd["theta"], gd["control_params"], pts)
    assert outside == pytest.approx(float(gd["outside"]), abs=1e-6)         # stored as fp32


def test_fixture_covers_the_reflection_branch():
    fr = gold("frame")
    assert float(fr["a"]["outside"]) >= 0.05 and float(fr["b"]["outside"]) >= 0.5 and float(fr["c"]["outside"]) >= 0.5
    # case d: every other column of the 5 x 9 frame lies on the control lattice
    g = R.grid_2d(5, 9, F32)
    on = (g.view(-1, 1, 2) == R.grid_2d(5, 5, F32).view(1, -1, 2)).all(dim=2).any(dim=1)
    assert int(on.sum()) == 25


@pytest.mark.parametrize("case", ["a", "b", "lattice"])
def test_restatement_reproduces_the_reference_coordinates(case):
    gd = gold("coords")[case]
    out, d = R.coords_with_grad(gd["coords"], gd["g"], gd["theta"], gd["control_params"], int(gd["points_tps"]), F32)
    pin(out, gd["out"], gd["ref_dev"]["out"])
    pin(d, gd["d_coords"], gd["ref_dev"]["d_coords"])
    assert torch.isfinite(gd["out"]).all() and torch.isfinite(gd["d_coords"]).all()


def test_restatement_reproduces_the_reference_chain():
    gd = gold("chain")
    a, b = gd["kp_d"].clone().requires_grad_(True), gd["transformed_kp"].clone().requires_grad_(True)
    loss = fv.EquivarianceLoss()(a, R.warp_coordinates(b[:, :, :2], gd["theta"], gd["control_params"], 5, F32))
    loss.backward()
    pin(loss, gd["loss"], 0)
    pin(a.grad, gd["d_kp_d"], 0)
    pin(b.grad, gd["d_transformed_kp"], 0)
