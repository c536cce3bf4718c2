"""CPU-side checks of the reenactment inference path: transform_kp_with_new_pose against the
reference fixture (tests/golden/animate.pt), the numpy restatement of evaluate.py's frame
conversion that the GPU test uses as its yardstick, the strict loader of reference checkpoints,
and the argument checks of Animator / MFE.infer / Generator.infer (no GPU calls)."""
import numpy as np
import pytest
import torch

import fvamd  # noqa: F401
import facevae_amd as fv
from animate_reference import frames_u8_numpy
from golden_io import load_golden

TOY_MFE = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_transform_kp_with_new_pose_matches_reference():
    g = load_golden("animate.pt")["new_pose"]
    kp, rot = fv.transform_kp_with_new_pose(g["kp_c"], g["yaw"], g["pitch"], g["roll"], g["t"], g["delta"],
                                            g["new_yaw"], g["new_pitch"], g["new_roll"])
    assert kp.shape == g["kp"].shape and rot.shape == g["rot"].shape
    assert rel(kp, g["kp"]) < 1e-6 and rel(rot, g["rot"]) < 1e-6
    # the single z-shift: the batch mean of z lands on 0.33
    assert abs(kp[:, :, 2].mean().item() - 0.33) < 1e-6
    assert fv.pose.transform_kp_with_new_pose is fv.transform_kp_with_new_pose


def test_new_pose_equal_to_old_pose_is_transform_kp_up_to_z_shift():
    g = load_golden("animate.pt")["new_pose"]
    kp, rot = fv.transform_kp_with_new_pose(g["kp_c"], g["yaw"], g["pitch"], g["roll"], g["t"], g["delta"],
                                            g["yaw"], g["pitch"], g["roll"])
    ref, R = fv.transform_kp(g["kp_c"], g["yaw"], g["pitch"], g["roll"], g["t"], torch.ones(2, 1, 1, 1))
    ref = ref + g["delta"]                      # R inv(R) = identity leaves delta as it is
    ref[:, :, 2] += 0.33 - ref[:, :, 2].mean()
    assert torch.equal(rot, R) and rel(kp, ref) < 1e-6


def test_frames_yardstick_truncates_and_clips():
    k = torch.arange(256, dtype=torch.float32)
    below = torch.nextafter(k / 255, torch.zeros(()))
    drv = torch.stack([k / 255, below, torch.full((256,), -0.5)]).view(1, 3, 16, 16)
    gen = torch.stack([torch.full((256,), 1.5), torch.ones(256), torch.zeros(256)]).view(1, 3, 16, 16)
    out = frames_u8_numpy(drv, gen)
    assert out.shape == (1, 16, 32, 3) and out.dtype == torch.uint8
    exact = (255 * (k / 255).numpy()).astype(np.uint8)
    assert np.array_equal(out[0, :, :16, 0].reshape(-1).numpy(), exact)
    # just below k / 255 never rounds up to k: truncation, not rounding
    assert (out[0, :, :16, 1].reshape(-1).int() <= torch.from_numpy(exact).int()).all()
    assert (out[0, :, :16, 2] == 0).all()                       # below 0 clips to 0
    assert (out[0, :, 16:, 0] == 255).all() and (out[0, :, 16:, 1] == 255).all()
    assert (out[0, :, 16:, 2] == 0).all()


def test_load_reference_models_round_trip(tmp_path):
    torch.manual_seed(3)
    src = {"afe": fv.AFE(), "generator": fv.Generator()}
    path = str(tmp_path / "00000007-checkpoint.pth.tar")
    torch.save({**{k: m.state_dict() for k, m in src.items()}, "epoch": 7}, path)
    got = fv.checkpoint.load_reference_models(path, names=("afe", "generator"))
    assert set(got) == {"afe", "generator"}
    for name, m in src.items():
        assert type(got[name]) is type(m)
        sd, gd = m.state_dict(), got[name].state_dict()
        assert list(sd) == list(gd)
        for k in sd:
            assert torch.equal(sd[k], gd[k]), (name, k)
    with pytest.raises(KeyError, match="mfe"):
        fv.checkpoint.load_reference_models(path, names=("afe", "mfe"))
    with pytest.raises(KeyError, match="efe"):
        fv.checkpoint.load_reference_models(path, names=("afe",), efe=True)
    bad = src["afe"].state_dict()
    bad["not_a_key"] = bad.pop("mid_conv.bias")
    torch.save({"afe": bad}, path)
    with pytest.raises(KeyError, match="not_a_key"):
        fv.checkpoint.load_reference_models(path, names=("afe",))
    # the existing two-model loader keeps its behaviour
    assert fv.checkpoint.MODELS == ("afe", "generator")


def _toy_nets():
    torch.manual_seed(1)
    return (fv.AFE(False, [16, 32], n_res=1, C=8, D=4),
            fv.CKD(False, down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3),
            fv.HPE_EDE(False, n_filters=[16, 32, 64], n_blocks=[1, 1], n_bins=6, K=3),
            fv.MFE(False, **TOY_MFE), fv.Generator(True, 1, [32, 16], D=4, C=8))


def test_animator_and_infer_raise_on_cpu_tensors():
    nets = _toy_nets()
    anim = fv.Animator(*nets)
    assert not any(m.training for m in nets)                    # construction puts them in eval mode
    with pytest.raises(RuntimeError, match="GPU only"):
        anim.set_source(torch.rand(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="GPU only"):
        anim.drive(torch.rand(2, 3, 64, 64))
    mfe, gen = nets[3], nets[4]
    fs = torch.randn(1, 8, 4, 8, 8)
    kp, R = torch.zeros(1, 3, 3), torch.eye(3)[None]
    with pytest.raises(RuntimeError, match="GPU only"):
        mfe.infer(fs, kp, kp, R, R)
    with pytest.raises(RuntimeError, match="GPU only"):
        gen.infer(fs, torch.zeros(1, 4, 4, 8, 8), kp, kp, R, R, torch.ones(1, 1, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.warp.mfe_input(torch.randn(1, 3, 4, 8, 8), kp, kp, R, R, torch.float32)
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.warp.motion_warp(torch.zeros(1, 4, 4, 8, 8), fs, kp, kp, R, R, torch.float32)
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.warp.frames_u8(torch.rand(1, 3, 4, 4), torch.rand(1, 3, 4, 4))


def test_infer_raises_in_training_mode():
    mfe = fv.MFE(False, **TOY_MFE).train()
    kp, R = torch.zeros(1, 3, 3), torch.eye(3)[None]
    with pytest.raises(RuntimeError, match=r"eval\(\)"):
        mfe.infer(torch.randn(1, 8, 4, 8, 8), kp, kp, R, R)
    gen = fv.Generator(True, 1, [32, 16], D=4, C=8).train()
    with pytest.raises(RuntimeError, match=r"eval\(\)"):
        gen.infer(torch.randn(1, 8, 4, 8, 8), torch.zeros(1, 4, 4, 8, 8), kp, kp, R, R, None)
