"""Patch discriminator, CPU side: state-dict layout and seed-identical init against the reference
fixtures (tests/golden/make_golden_disc.py), the hinge GAN loss values, the new config fields."""
import json
import os

import pytest
import torch

import fvamd  # noqa: F401
import facevae_amd as fv
from golden_io import load_golden

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return load_golden("discriminator.pt")


def test_default_discriminator_keys():
    keys = json.load(open(os.path.join(GOLD, "disc_keys.json")))
    assert len(keys) == 28
    assert list(fv.Discriminator().state_dict()) == keys


def test_init_matches_reference_bit_for_bit(gold):
    """Same RNG draw order as the reference constructors: conv weight, bias, then spectral norm's
    u and v per layer; the instance norm draws nothing."""
    torch.manual_seed(11)
    D = fv.Discriminator(True, [8, 16, 32, 64], K=2)
    sd = D.state_dict()
    assert list(sd) == list(gold["init"])
    for k in sd:
        assert torch.equal(sd[k], gold["init"][k]), k
    torch.manual_seed(12)
    blk = fv.ConvBlock2D("CNA", 5, 16, 3, 2, 1, True, "instance", "leakyrelu")
    sd = blk.state_dict()
    assert list(sd) == list(gold["block"]["init"])
    for k in sd:
        assert torch.equal(sd[k], gold["block"]["init"][k]), k


def test_gan_loss_values(gold):
    gan = fv.GANLoss()
    o_f, o_r = gold["fake"]["output"], gold["real"]["output"]
    # G (generator form) belongs to the first pair of forwards, G1 / G2 to the second pair
    assert torch.allclose(gan(o_f, True, False), gold["G"], rtol=1e-6, atol=0)
    assert torch.allclose(gan(gold["fake2"], False, True), gold["G1"], rtol=1e-6, atol=0)
    assert torch.allclose(gan(gold["real2"], True, True), gold["G2"], rtol=1e-6, atol=0)
    assert gold["G1"].item() > 0 and gold["G2"].item() > 0 and o_r.shape == o_f.shape
    x = torch.tensor([[-3.0, -1.0, -0.5, 0.0, 0.5, 1.0, 3.0]])
    assert gan(x, True, True).item() == pytest.approx((4 + 2 + 1.5 + 1 + 0.5) / 7, rel=1e-6)
    assert gan(x, False, True).item() == pytest.approx((0.5 + 1 + 1.5 + 2 + 4) / 7, rel=1e-6)
    assert gan(x, True, False).item() == pytest.approx(0.0, abs=1e-7)


def test_feature_matching_needs_the_gpu(gold):
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.FeatureMatchingLoss()(gold["fake"]["features"], gold["real"]["features"])


def test_config_defaults():
    cfg = fv.FaceVAEConfig()
    assert cfg.w_G == 0.0 and cfg.w_F == 0.0
    assert tuple(cfg.disc_down_seq) == (64, 128, 256, 512)
    toy = fv.FaceVAEConfig.toy()
    assert toy.w_G == 0.0 and toy.w_F == 0.0


def test_block_still_rejects_what_is_not_built():
    with pytest.raises(NotImplementedError):
        fv.ConvBlock2D("CNA", 8, 8, 3, 2, 1, True)                       # stride 2 with batch norm
    with pytest.raises(NotImplementedError):
        fv.ConvBlock2D("CNA", 8, 8, 5, 2, 2, True, "instance", "leakyrelu")   # stride 2, 5x5
    with pytest.raises(NotImplementedError):
        fv.ConvBlock2D("NAC", 8, 8, 3, 1, 1, True, "instance")
    with pytest.raises(NotImplementedError):
        fv.ConvBlock2D("CN", 8, 8, 3, 1, 1, True)                        # "CN" needs activation_type "none"
