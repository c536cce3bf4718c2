"""CPU checks of the canonical keypoint detector's module layer: state-dict keys, shapes and
parameter counts against the reference (tests/golden/ckd_keys.json), the constructor RNG draws
against the init_sum checksums of tests/golden/ckd.pt, the forms that must raise, and the three
keypoint losses (torch ops on tiny tensors, device agnostic) against the `losses` fixture within
1e-6 relative."""
import json
import os

import pytest
import torch

import fvamd  # noqa: F401
import facevae_amd as fv
from golden_io import load_golden

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOY = dict(down_seq=[3, 8, 16, 32], up_seq=[32, 16, 8], D=4, K=3)


def _keys():
    with open(os.path.join(GOLD, "ckd_keys.json")) as f:
        return json.load(f)


def test_state_dict_keys_match_reference():
    ref = _keys()
    assert ref["toy_config"] == TOY
    net = fv.CKD(False, **TOY)
    toy = net.state_dict()
    assert list(toy.keys()) == ref["toy"] and len(toy) == 39
    assert {k: list(v.shape) for k, v in toy.items()} == ref["toy_shapes"]
    assert sum(p.numel() for p in net.parameters()) == ref["toy_params"] == 28371
    net = fv.CKD()
    sd = net.state_dict()
    assert list(sd.keys()) == ref["default"] and len(sd) == 74
    assert {k: list(v.shape) for k, v in sd.items()} == ref["default_shapes"]
    assert sum(p.numel() for p in net.parameters()) == ref["default_params"] == 41940047
    assert (net.C, net.D, net.scale_factor) == (1024, 16, 0.25)


def test_constructor_draws_match_reference():
    gd = load_golden("ckd.pt")["ckd"]
    torch.manual_seed(int(gd["seed"]))
    sd = fv.CKD(False, **TOY).state_dict()
    assert set(gd["init_sum"]) == {k for k, v in sd.items() if v.is_floating_point()}
    for k, v in gd["init_sum"].items():
        assert sd[k].double().sum().item() == v.item(), k


def test_unsupported_forms_raise():
    with pytest.raises(NotImplementedError, match="use_weight_norm"):
        fv.CKD(use_weight_norm=True)
    with pytest.raises(NotImplementedError, match="batch-norm"):
        fv.CKD(False, [3, 8, 24, 32], [32, 16, 8], 4, 3)         # 24 is not 8 * 2^k
    with pytest.raises(NotImplementedError, match="batch-norm"):
        fv.CKD(False, [3, 4, 32], [32, 8], 4, 3)                 # 4 < 8
    with pytest.raises(NotImplementedError, match="depth split"):
        fv.CKD(False, [3, 8, 32], [32, 8], 3, 3)                 # 32 * 3 = 96
    with pytest.raises(NotImplementedError, match="3-D conv"):
        fv.CKD(False, [3, 8, 32], [32, 12], 4, 3)                # 12 input channels into out_conv
    with pytest.raises(NotImplementedError, match="down_seq"):
        fv.CKD(False, [8, 8, 32], [32, 8], 4, 3)
    with pytest.raises(NotImplementedError, match="D must be"):
        fv.CKD(False, [3, 8, 32], [8, 8], 1, 3)
    with pytest.raises(NotImplementedError, match="K"):
        fv.CKD(False, [3, 8, 32], [32, 8], 4, 300)
    fv.CKD(False, [3, 8, 32], [32, 24, 8], 4, 1)                 # 24 channels run on the padded BN, K = 1


def test_cpu_tensor_and_odd_sizes_are_rejected():
    net = fv.CKD(False, **TOY)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 3, 64, 96))
    from facevae_amd import ops_ckd
    with pytest.raises(RuntimeError, match="GPU only"):
        ops_ckd.ResizeFn.apply(torch.zeros(1, 3, 8, 8), 0.5, torch.float32)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops_ckd.SoftArgmaxFn.apply(torch.zeros(1, 3, 2, 4, 4))
    net._check_sizes(64, 96)                      # 16 x 24 -> 8 x 12 -> 4 x 6 -> 2 x 3
    with pytest.raises(ValueError, match=r"down\.0 "):
        net._check_sizes(60, 96)                  # 15 x 24
    with pytest.raises(ValueError, match=r"down\.1 "):
        net._check_sizes(64, 72)                  # 16 x 18 -> 8 x 9
    with pytest.raises(ValueError, match=r"down\.2 "):
        net._check_sizes(48, 96)                  # 12 x 24 -> 6 x 12 -> 3 x 6
    with pytest.raises(ValueError, match="no pixel"):
        net._check_sizes(3, 96)
    fv.CKD()._check_sizes(256, 256)
    with pytest.raises(ValueError, match=r"down\.4 "):
        fv.CKD()._check_sizes(320, 256)           # 80 -> 40 -> 20 -> 10 -> 5


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_keypoint_losses_match_reference():
    gd = load_golden("ckd.pt")["losses"]
    kp, rev, delta = gd["kp"], gd["rev"], gd["delta"]
    # the fixture's hinge is active: an off-diagonal pair is closer than sqrt(Dt)
    d = torch.cdist(kp, kp).square() + 10 * torch.eye(kp.shape[1])
    assert d.min().item() < 0.1

    a, b = kp.clone().requires_grad_(True), rev.clone().requires_grad_(True)
    loss = fv.EquivarianceLoss()(a, b)
    loss.backward()
    assert _rel(loss, gd["equivariance"]["loss"]) < 1e-6
    assert _rel(a.grad, gd["equivariance"]["d_kp"]) < 1e-6 and _rel(b.grad, gd["equivariance"]["d_rev"]) < 1e-6

    a = kp.clone().requires_grad_(True)
    crit = fv.KeypointPriorLoss()
    assert (crit.Dt, crit.zt) == (0.1, 0.33)
    loss = crit(a)
    loss.backward()
    assert _rel(loss, gd["prior"]["loss"]) < 1e-6
    assert _rel(a.grad, gd["prior"]["d_kp"]) < 1e-6

    a = delta.clone().requires_grad_(True)
    loss = fv.DeformationPriorLoss()(a)
    loss.backward()
    assert _rel(loss, gd["deformation"]["loss"]) < 1e-6
    assert _rel(a.grad, gd["deformation"]["d_delta"]) < 1e-6
