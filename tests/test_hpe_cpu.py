"""CPU checks of the head pose estimator's module layer: state-dict keys and constructor RNG draws
against the reference (tests/golden/hpe_keys.json, the init_sum checksums of tests/golden/hpe.pt),
the forms that must raise, and transform_kp / HeadPoseLoss (torch ops on tiny tensors, device
agnostic) against the `pose` fixture within 1e-6 relative."""
import json
import os

import pytest
import torch

import fvamd  # noqa: F401
import facevae_amd as fv
from golden_io import load_golden

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOY = dict(n_filters=[16, 32, 64], n_blocks=[1, 1], n_bins=6, K=3)

CTORS = {
    "stem": lambda: torch.nn.Sequential(fv.ConvBlock2D("CNA", 3, 16, 7, 2, 3, False), fv.MaxPool2d(3, 2, 1)),
    "bneck_id": lambda: fv.ResBottleneck(32, 32, 1, False),
    "bneck_proj": lambda: fv.ResBottleneck(16, 32, 1, False),
    "bneck_s2": lambda: fv.ResBottleneck(32, 64, 2, False),
    "hpe": lambda: fv.HPE_EDE(False, **TOY),
}


def _keys():
    with open(os.path.join(GOLD, "hpe_keys.json")) as f:
        return json.load(f)


def test_state_dict_keys_match_reference():
    ref = _keys()
    assert ref["toy_config"] == TOY
    toy = fv.HPE_EDE(False, **TOY).state_dict()
    assert list(toy.keys()) == ref["toy"] and len(toy) == 115
    assert {k: list(v.shape) for k, v in toy.items()} == ref["toy_shapes"]
    assert sum(p.numel() for p in fv.HPE_EDE(False, **TOY).parameters()) == 17782
    sd = fv.HPE_EDE().state_dict()
    assert list(sd.keys()) == ref["default"] and len(sd) == 402
    assert {k: list(v.shape) for k, v in sd.items()} == ref["default_shapes"]
    assert not any("idx_tensor" in k for k in sd)


@pytest.mark.parametrize("case", list(CTORS))
def test_constructor_draws_match_reference(case):
    gd = load_golden("hpe.pt")[case]
    torch.manual_seed(int(gd["seed"]))
    sd = CTORS[case]().state_dict()
    assert set(gd["init_sum"]) == {k for k, v in sd.items() if v.is_floating_point()}
    for k, v in gd["init_sum"].items():
        assert sd[k].double().sum().item() == v.item(), k


def test_unsupported_forms_raise():
    with pytest.raises(NotImplementedError):
        fv.HPE_EDE(use_weight_norm=True)
    with pytest.raises(NotImplementedError):
        fv.ResBottleneck(32, 32, 1, True)
    with pytest.raises(NotImplementedError):
        fv.ResBottleneck(32, 48, 1, False)            # 48 // 4 = 12 is not 8 * 2^k
    with pytest.raises(NotImplementedError):
        fv.ResBottleneck(32, 16, 1, False)            # 16 // 4 = 4 < 8
    with pytest.raises(NotImplementedError):
        fv.MaxPool2d(2, 2, 0)
    # the new forms exist with batch norm and without spectral norm only
    for args in (("CNA", 3, 16, 7, 2, 3, True), ("CNA", 8, 8, 3, 2, 1, True), ("CN", 8, 8, 1, 1, 0, True),
                 ("CN", 8, 8, 1, 2, 0, True), ("CN", 8, 8, 3, 1, 1, True), ("CN", 8, 8, 3, 1, 1, False),
                 ("CNA", 8, 8, 7, 2, 3, False), ("CNA", 8, 8, 5, 2, 2, False), ("CN", 8, 8, 1, 3, 0, False),
                 ("CNA", 3, 24, 7, 2, 3, False)):
        with pytest.raises(NotImplementedError):
            fv.ConvBlock2D(*args)
    with pytest.raises(NotImplementedError):
        fv.ConvBlock2D("CN", 8, 8, 1, 1, 0, False, activation_type="instance")
    for args in (("CNA", 3, 16, 7, 2, 3, False), ("CNA", 8, 8, 3, 2, 1, False), ("CN", 8, 16, 1, 1, 0, False),
                 ("CN", 8, 16, 1, 2, 0, False)):
        fv.ConvBlock2D(*args)


def test_cpu_tensor_and_odd_sizes_are_rejected():
    net = fv.HPE_EDE(False, **TOY)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.ResBottleneck(32, 32, 1, False)(torch.zeros(1, 32, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.MaxPool2d(3, 2, 1)(torch.zeros(1, 8, 4, 4))
    # 36 = 2 * 2 * 9: the stem and the pool pass, the stride-2 bottleneck sees 9 x 8
    with pytest.raises(ValueError, match=r"res_layers\.2"):
        net._check_sizes(36, 32)
    with pytest.raises(ValueError, match=r"pre_layers\.1"):
        net._check_sizes(32, 34)
    with pytest.raises(ValueError, match=r"pre_layers\.0"):
        net._check_sizes(33, 32)
    net._check_sizes(32, 48)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_transform_kp_and_head_pose_loss_match_reference():
    gd = load_golden("hpe.pt")["pose"]
    names = ("kp", "yaw", "pitch", "roll", "t", "scale")
    ins = [gd["inputs"][n].clone().requires_grad_(True) for n in names]
    kp, R = fv.transform_kp(*ins)
    assert _rel(kp, gd["kp_out"]) < 1e-6 and _rel(R, gd["R"]) < 1e-6
    ((kp * gd["g_kp"]).sum() + (R * gd["g_R"]).sum()).backward()
    for n, v in zip(names, ins):
        assert _rel(v.grad, gd["d_inputs"][n]) < 1e-6, n
    est = [gd["inputs"][n].clone().requires_grad_(True) for n in names[1:4]]
    loss = fv.HeadPoseLoss()(*est, *[gd["real"][n] for n in names[1:4]])
    assert _rel(loss, gd["loss"]) < 1e-6
    loss.backward()
    for n, v in zip(names[1:4], est):
        assert _rel(v.grad, gd["d_loss"][n]) < 1e-6, n
    # the composition order of utils.py:57: Ry(pitch) @ Rx(yaw) @ Rz(roll)
    a = gd["inputs"]
    want = fv.rotation_matrix_y(a["pitch"]) @ fv.rotation_matrix_x(a["yaw"]) @ fv.rotation_matrix_z(a["roll"])
    assert torch.equal(R.detach(), want)
