"""CPU checks of the motion field estimator's module layer: state-dict keys and constructor RNG
draws against the reference (tests/golden/mfe_keys.json, the init_sum checksums of
tests/golden/mfe.pt), and the forms that must raise."""
import json
import os

import pytest
import torch

import fvamd  # noqa: F401
import facevae_amd as fv
from golden_io import load_golden

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOY = dict(down_seq=[16, 16, 24], up_seq=[24, 16, 8], K=3, D=4, C1=8, C2=3)


def _keys():
    with open(os.path.join(GOLD, "mfe_keys.json")) as f:
        return json.load(f)


def test_state_dict_keys_match_reference():
    ref = _keys()
    assert ref["toy_config"] == TOY
    assert list(fv.MFE(False, **TOY).state_dict().keys()) == ref["toy"]
    sd = fv.MFE().state_dict()
    assert list(sd.keys()) == ref["default"]
    assert {k: list(v.shape) for k, v in sd.items()} == ref["default_shapes"]


@pytest.mark.parametrize("case", ["down3d", "up3d", "mfe"])
def test_constructor_draws_match_reference(case):
    gd = load_golden("mfe.pt")[case]
    torch.manual_seed(int(gd["seed"]))
    mod = {"down3d": lambda: fv.DownBlock3D(16, 24, False), "up3d": lambda: fv.UpBlock3D(24, 8, False),
           "mfe": lambda: fv.MFE(False, **TOY)}[case]()
    sd = mod.state_dict()
    assert set(gd["init_sum"]) == {k for k, v in sd.items() if v.is_floating_point()}
    for k, v in gd["init_sum"].items():
        assert sd[k].double().sum().item() == v.item(), k


def test_unsupported_forms_raise():
    with pytest.raises(NotImplementedError):
        fv.MFE(use_weight_norm=True)
    with pytest.raises(NotImplementedError):
        fv.ConvBlock3D("CN", 16, 16, 3, 1, 1, False)
    with pytest.raises(NotImplementedError):
        fv.ConvBlock3D("CNA", 16, 16, 5, 1, 2, False)
    with pytest.raises(NotImplementedError):
        fv.ConvBlock3D("CNA", 16, 16, 3, 1, 1, True)
    with pytest.raises(NotImplementedError):
        fv.Conv3d(16, 16, 5, 1, 2)


def test_cpu_tensor_is_rejected():
    mfe = fv.MFE(False, **TOY)
    fs = torch.zeros(1, 8, 4, 8, 8)
    kp = torch.zeros(1, 3, 3)
    R = torch.eye(3)[None]
    with pytest.raises(RuntimeError, match="GPU only"):
        mfe(fs, kp, kp, R, R)
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.DownBlock3D(16, 24, False)(torch.zeros(1, 16, 2, 4, 4))
