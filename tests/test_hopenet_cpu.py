"""CPU-side checks of the frozen Hopenet teacher: the state-dict layout and parameter counts, the
seeded constructor's draws, the torch restatement (tests/hopenet_reference.py) against the fixture
made from the reference (tests/golden/hopenet.pt, make_golden_hopenet.py), the preprocessing's
restatement against F.interpolate, state-dict round trips and the module's refusals (no GPU calls)."""
import json
import os

import pytest
import torch

import hopenet_reference as R
from golden_io import load_golden

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fv():
    import fvamd  # noqa: F401
    import facevae_amd
    return facevae_amd


@pytest.fixture(scope="module")
def gold():
    return load_golden("hopenet.pt")


@pytest.fixture(scope="module")
def x224(gold):
    frames = R.make_inputs()
    assert torch.equal(R.checksum(frames), gold["l1111"]["input_sum"])
    x = R.preprocess(frames)
    assert torch.equal(R.checksum(x), gold["l1111"]["prep_sum"])
    return x


def test_keys_and_parameter_counts(fv):
    keys = json.load(open(os.path.join(GOLD, "hopenet_keys.json")))
    for name, count, params in (("l1111", 110, 8_427_794), ("l3463", 326, 23_919_890)):
        layers, bins, _ = R.NETS[name]
        m = fv.Hopenet(None, layers, bins)
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == keys[name]
        assert len(got) == count and sum(p.numel() for p in m.parameters()) == params
        assert "idx_tensor" not in dict(m.named_buffers()) and "fc_finetune.weight" in m.state_dict()
        assert not m.training and not any(p.requires_grad for p in m.parameters())
    assert len(fv.Hopenet().state_dict()) == 326                       # the defaults are the ResNet-50
    m = fv.Hopenet(R.Bottleneck, [1, 1, 1, 1], 6)                      # a block class with expansion 4 is accepted
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == keys["bins6"]


@pytest.mark.parametrize("name", list(R.NETS))
def test_seeded_constructor_matches_the_reference(fv, gold, name):
    layers, bins, gain = R.NETS[name]
    g = gold[name]
    torch.manual_seed(int(g["seed"]))
    m = fv.Hopenet(None, layers, bins)
    assert torch.equal(R.state_checksums(m), g["init_sums"])
    assert torch.equal(R.state_checksums(R.overwrite(m, int(g["stat_seed"]), gain)), g["state_sums"])
    assert torch.equal(R.state_checksums(R.build(R.RefHopenet, layers, bins, gain)), g["state_sums"])


@pytest.mark.parametrize("name", list(R.NETS))
def test_restatement_reproduces_the_fixture(gold, x224, name):
    layers, bins, gain = R.NETS[name]
    g = gold[name]
    net = R.build(R.RefHopenet, layers, bins, gain)
    feat, taps = R.features_of(net, x224)
    ang = net(x224)
    df, da = R.rel_l2(feat, g["features"]), (ang - g["angles"]).abs().max().item()
    print(f"{name}: features {df:.2e} rel-L2, angles {da:.2e} rad")
    assert df <= 1e-6 and da <= 1e-6
    for i, t in enumerate(taps):
        assert R.rel_l2(R.sample(t), g["taps"][str(i)]) <= 1e-6, i
    ef, ea = R.emulate_bf16(net, x224)
    dev = (R.rel_l2(ef, g["features"]), (ea - g["angles"]).abs().max().item())
    print(f"{name}: bf16 emulation {dev[0]:.2e} rel-L2, {dev[1]:.2e} rad (fixture {g['bf16_dev'].tolist()})")
    assert 0.5 * g["bf16_dev"][0] <= dev[0] <= 2 * g["bf16_dev"][0]


@pytest.mark.parametrize("src,dst", R.RESIZES)
def test_preprocess_restatement_is_bit_equal_to_interpolate(src, dst):
    x = torch.rand(2, 3, *src, generator=torch.Generator().manual_seed(src[0] * 1000 + dst[1]))
    assert torch.equal(R.preprocess(x, dst), R.preprocess_torch(x, dst))


def test_state_dict_round_trip(fv):
    ref = R.build(R.RefHopenet, (1, 1, 1, 1), 66, seed=77, stat_seed=78)
    m = fv.Hopenet(None, [1, 1, 1, 1], 66)
    m.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), ref.state_dict().values()))
    back = R.RefHopenet(R.Bottleneck, [1, 1, 1, 1], 66)
    back.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(R.state_checksums(back), R.state_checksums(ref))


def test_refusals(fv):
    class Basic:
        expansion = 1

    with pytest.raises(NotImplementedError, match="expansion 4"):
        fv.Hopenet(Basic, [2, 2, 2, 2], 66)
    m = fv.Hopenet(None, [1, 1, 1, 1], 66)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(torch.rand(1, 3, 224, 224))
    with pytest.raises(RuntimeError, match="GPU only"):
        m.teacher_angles(torch.rand(1, 3, 40, 56))
    m.train()
    with pytest.raises(RuntimeError, match="frozen teacher"):
        m(torch.rand(1, 3, 224, 224))
