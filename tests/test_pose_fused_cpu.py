"""CPU-side checks of the fused pose step: the fp64 restatement (pose_reference.py) that the GPU tests
of fv_pose_kp_fwd / fv_pose_kp_new_fwd use as their yardstick is held to the two reference fixtures
and to torch.inverse first, the restated u8 -> float conversion to data.u8_to_float on every byte, and
the new entry points raise the usual error on CPU tensors (no GPU calls)."""
import numpy as np
import pytest
import torch

import fvamd  # noqa: F401
import facevae_amd as fv
import pose_reference as P
from facevae_amd.data import u8_to_float
from golden_io import load_golden
from pose_reference import rel


def test_restatement_reproduces_transform_kp_fixture():
    gd = load_golden("hpe.pt")["pose"]
    a = gd["inputs"]
    kp, R, J = P.transform_kp_fp64(a["kp"], a["yaw"], a["pitch"], a["roll"], a["t"], a["scale"])
    assert J is None and kp.dtype == torch.float64 and kp.shape == gd["kp_out"].shape and R.shape == gd["R"].shape
    assert rel(kp, gd["kp_out"]) < 1e-6 and rel(R, gd["R"]) < 1e-6


def test_restatement_reproduces_new_pose_fixture():
    g = load_golden("animate.pt")["new_pose"]
    kp, R, _ = P.transform_kp_new_fp64(g["kp_c"], g["yaw"], g["pitch"], g["roll"], g["t"], g["delta"], g["new_yaw"],
                                       g["new_pitch"], g["new_roll"])
    assert kp.shape == g["kp"].shape and R.shape == g["rot"].shape
    assert rel(kp, g["kp"]) < 1e-6 and rel(R, g["rot"]) < 1e-6
    assert abs(kp[:, :, 2].mean().item() - 0.33) < 1e-12


@pytest.mark.parametrize("name", list(P.CASES))
def test_adjugate_jacobian_agrees_with_torch_inverse(name):
    N, Nc, Ns, K = P.CASES[name]
    a = P.pose_inputs(name)
    assert tuple(a["kp_c"].shape) == (Nc, K, 3) and tuple(a["Rs"].shape) == (Ns, 3, 3) and a["yaw"].numel() == N
    for angles in (("yaw", "pitch", "roll"), ("new_yaw", "new_pitch", "new_roll")):
        R = P.rotation(*(a[k] for k in angles))
        want = a["Rs"].double() @ torch.inverse(R)
        assert rel(P.jacobian(a["Rs"], R), want) < 1e-12
        assert rel(P.inverse_adjugate(R), R.transpose(1, 2)) < 1e-12        # a rotation, so also its transpose
    # and on a matrix that is no rotation, where the transpose would be wrong
    gen = torch.Generator().manual_seed(5)
    m = torch.randn(4, 3, 3, generator=gen, dtype=torch.float64) + 2 * torch.eye(3, dtype=torch.float64)
    assert rel(P.inverse_adjugate(m), torch.inverse(m)) < 1e-12


def test_u8_restatement_is_u8_to_float():
    x = np.arange(256, dtype=np.uint8)
    assert np.array_equal(P.u8_to_float_exact(x), u8_to_float(x))
    assert P.u8_to_float_exact(x).dtype == np.float32


def test_fused_pose_entry_points_raise_on_cpu_tensors():
    a = P.pose_inputs("b")
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.pose.pose_kp(a["kp_c"], a["yaw"], a["pitch"], a["roll"], a["t"], a["scale"])
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.pose.pose_kp(a["kp_c"], a["yaw"], a["pitch"], a["roll"], a["t"], a["scale"], a["Rs"])
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.pose.pose_kp_new(a["kp_c"], a["yaw"], a["pitch"], a["roll"], a["t"], a["delta"], a["new_yaw"],
                            a["new_pitch"], a["new_roll"])
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.warp.frames_from_u8(torch.zeros(1, 2, 2, 3, dtype=torch.uint8))
    assert fv.CapturedDrive is fv.animate.CapturedDrive
