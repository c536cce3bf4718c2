"""CPU checks of the expression feature extractor's module layer: state-dict keys, shapes and
parameter counts of EFE_conv5, SameBlock3D, ResBlock3D(30) and ContrastiveLoss_linear against the
reference (tests/golden/efe_keys.json), the constructor RNG draws against the init_sum checksums
of tests/golden/efe.pt, the forms that must raise, the descriptor `mix` runs on at the default
size (cin = cout = 32 in bf16 at W = 64: the MFMA path, which is the one with fused BN-statistics
records), the argument checks of the fv_efe_kpcat_* entries (made before any launch) and the
"GPU only" errors.  ContrastiveLoss_linear is torch ops on any device, so its fixture is checked
here too (1e-4, the gate of the GPU test)."""
import ctypes
import json
import os

import pytest
import torch

import fvamd  # noqa: F401
import facevae_amd as fv
from facevae_amd import _lib as L, ops, ops3d, ops_efe
from golden_io import load_golden

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOY = dict(down_seq=[3, 8, 16, 32], up_seq=[16, 8, 8], D=4, K=3, n_res=2)


def _keys():
    with open(os.path.join(GOLD, "efe_keys.json")) as f:
        return json.load(f)


def _same_keys(mod, ref):
    sd = mod.state_dict()
    assert list(sd.keys()) == ref["keys"]
    assert {k: list(v.shape) for k, v in sd.items()} == ref["shapes"]
    assert sum(p.numel() for p in mod.parameters()) == ref["params"]


def _same_init(sd, init_sum):
    assert set(init_sum) == {k for k, v in sd.items() if v.is_floating_point()}
    for k, v in init_sum.items():
        assert sd[k].double().sum().item() == v.item(), k


def perturb_bn(mod, seed):
    """tests/golden/make_golden_efe.py's: every batch norm's weight in [0.5, 1.5], bias N(0, 0.5)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if hasattr(m, "running_mean") and getattr(m, "weight", None) is not None:
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.5)


def test_state_dict_keys_match_reference():
    ref = _keys()
    assert ref["toy_config"] == TOY
    toy = fv.EFE_conv5(False, **TOY)
    _same_keys(toy, ref["toy"])
    assert len(toy.state_dict()) == 74 and ref["toy"]["params"] == 15246
    net = fv.EFE_conv5()
    _same_keys(net, ref["default"])
    assert len(net.state_dict()) == 123 and ref["default"]["params"] == 3625122
    assert (net.C, net.D, net.K, net.scale_factor) == (256, 16, 15, 0.25)
    _same_keys(fv.SameBlock3D(30, 15, False), ref["same3d_30_15"])
    _same_keys(fv.ResBlock3D(30, False), ref["res3d_30"])
    crit = fv.ContrastiveLoss_linear(mode="non-direction")
    _same_keys(crit, ref["contrastive_default"])
    assert len(crit.state_dict()) == 25 and ref["contrastive_default"]["params"] == 1314816
    assert crit.projection[6].bias.requires_grad is False
    _same_keys(fv.ContrastiveLoss_linear(), ref["contrastive_direction"])
    assert len(fv.ContrastiveLoss_linear().state_dict()) == 0


def test_constructor_draws_match_reference():
    g = load_golden("efe.pt")
    torch.manual_seed(int(g["efe"]["seed"]))
    _same_init(fv.EFE_conv5(False, **TOY).state_dict(), g["efe"]["no_vae"]["init_sum"])
    ctors = dict(c30_d4=lambda: fv.ResBlock3D(30, False), c30_d5=lambda: fv.ResBlock3D(30, False),
                 c6=lambda: fv.ResBlock3D(6, False), same30to15=lambda: fv.SameBlock3D(30, 15, False))
    for name, ctor in ctors.items():
        torch.manual_seed(int(g["resblock"][name]["seed"]))
        _same_init(ctor().state_dict(), g["resblock"][name]["init_sum"])
    torch.manual_seed(int(g["contrastive"]["non_direction"]["seed"]))
    _same_init(fv.ContrastiveLoss_linear(mode="non-direction").state_dict(), g["contrastive"]["non_direction"]["init_sum"])


def test_unsupported_forms_raise():
    with pytest.raises(NotImplementedError, match="use_weight_norm"):
        fv.EFE_conv5(use_weight_norm=True)
    with pytest.raises(NotImplementedError, match="use_vae"):
        fv.EFE_conv5(use_vae=False)
    with pytest.raises(NotImplementedError, match=r"down_seq\[-1\]"):
        fv.EFE_conv5(False, [3, 8, 16, 64], [16, 8, 8], 4, 3)
    with pytest.raises(NotImplementedError, match=r"down_seq\[0\]"):
        fv.EFE_conv5(False, [8, 8, 32], [16, 8], 4, 3)
    with pytest.raises(NotImplementedError, match="batch-norm"):
        fv.EFE_conv5(False, [3, 8, 24, 32], [16, 8, 8], 4, 3)
    with pytest.raises(NotImplementedError, match="depth split"):
        fv.EFE_conv5(False, [3, 8, 32], [16, 8], 3, 3)
    with pytest.raises(NotImplementedError, match="3-D conv"):
        fv.EFE_conv5(False, [3, 8, 32], [16, 12], 4, 3)
    with pytest.raises(NotImplementedError, match="D must be"):
        fv.EFE_conv5(False, [3, 8, 32], [8, 8], 1, 3)
    with pytest.raises(NotImplementedError, match="K"):
        fv.EFE_conv5(False, [3, 8, 32], [16, 8], 4, 300)
    with pytest.raises(NotImplementedError, match="at most 64"):
        fv.EFE_conv5(False, [3, 8, 32], [16, 8], 4, 33)           # 2K = 66 pads to 128
    fv.EFE_conv5(False, [3, 8, 32], [16, 8], 4, 32)               # 2K = 64: no pad
    with pytest.raises(NotImplementedError, match="at most 64"):
        fv.ResBlock3D(70, False)
    with pytest.raises(NotImplementedError, match="spectral"):
        fv.SameBlock3D(8, 8, True)
    assert fv.ResBlock3D(30, False).padded and not fv.ResBlock3D(32, False).padded


def test_size_check_names_the_layer():
    net = fv.EFE_conv5(False, **TOY)
    net._check_sizes(64, 64)                      # 16 x 16 -> (Same) -> 8 x 8 -> 4 x 4
    with pytest.raises(ValueError, match=r"down\.2 leaves 8 x 8"):
        net._check_sizes(128, 128)
    with pytest.raises(ValueError, match=r"down\.2 leaves 4 x 6"):
        net._check_sizes(64, 96)
    with pytest.raises(ValueError, match=r"down\.1 .*even"):
        net._check_sizes(60, 64)                  # 15 x 16
    with pytest.raises(ValueError, match=r"down\.2 .*even"):
        net._check_sizes(72, 64)                  # 18 x 16 -> 9 x 8
    with pytest.raises(ValueError, match="no pixel"):
        net._check_sizes(3, 64)
    fv.EFE_conv5()._check_sizes(256, 256)
    with pytest.raises(ValueError, match=r"down\.4 leaves 8 x 8"):
        fv.EFE_conv5()._check_sizes(512, 512)


def test_mix_descriptor_takes_the_mfma_path():
    """At K = 15 `mix` runs at pad_pow2(30) = 32 channels: in bf16 at W = 64 that is the descriptor of
    the AFE trunk (c32_fast), which alone writes fused BN-statistics records."""
    assert ops.pad_pow2(2 * 15) == 32 and ops.pad_pow2(6) == 8 and ops.pad_pow2(8) == 8
    d = ops3d.desc3(torch.bfloat16, 2, 16, 64, 64, 32, 32)
    assert L.query("fv_conv3d_stats_blocks", ctypes.byref(d)) > 0
    assert L.query("fv_conv3d_wk_bytes", ctypes.byref(d)) == 27 * 32 * 32 * 2
    for bad in (ops3d.desc3(torch.float32, 2, 16, 64, 64, 32, 32), ops3d.desc3(torch.bfloat16, 2, 4, 8, 8, 8, 8)):
        assert L.query("fv_conv3d_stats_blocks", ctypes.byref(bad)) == 0       # the direct kernels
        assert L.query("fv_conv3d_wk_bytes", ctypes.byref(bad)) > 0
    d30 = ops3d.desc3(torch.bfloat16, 2, 16, 64, 64, 30, 30)
    assert L.query("fv_conv3d_wk_bytes", ctypes.byref(d30)) == 0               # why the block pads


def test_kpcat_argument_checks():
    """The checks run before any launch, so they need no GPU."""
    lib = L.load()
    ok = (2, 15, 32, 16, 64, 64)
    assert L.query("fv_efe_kpcat_ws_bytes", *ok) > 0
    assert L.query("fv_efe_kpcat_ws_bytes", 1, 3, 8, 4, 8, 8) > 0
    bad = {"D": (2, 15, 32, 1, 64, 64), "H": (2, 15, 32, 16, 1, 64), "W": (2, 15, 32, 16, 64, 1),
           "K0": (2, 0, 8, 16, 64, 64), "K257": (2, 257, 1024, 4, 4, 4), "Cp30": (2, 15, 30, 16, 64, 64),
           "Cp64": (2, 15, 64, 16, 64, 64), "Cp8": (2, 5, 8, 4, 4, 4)}
    for name, a in bad.items():
        assert L.query("fv_efe_kpcat_ws_bytes", *a) == 0, name
        n, k, cp, d, h, w = a
        st = lib.fv_efe_kpcat_fwd(L.FV_F32, None, None, n, k, cp, d, h, w, 0.01, None, None)
        assert st == L.FV_E_UNSUPPORTED, (name, st)
        assert lib.fv_last_error()
        st = lib.fv_efe_kpcat_bwd(L.FV_BF16, None, None, n, k, cp, d, h, w, 0.01, None, None, None, None)
        assert st == L.FV_E_UNSUPPORTED, (name, st)
    assert lib.fv_efe_kpcat_fwd(L.FV_F64, None, None, *ok, 0.01, None, None) == L.FV_E_UNSUPPORTED
    assert lib.fv_efe_kpcat_fwd(L.FV_F32, None, None, *ok, 0.0, None, None) == L.FV_E_UNSUPPORTED
    assert lib.fv_efe_kpcat_fwd(L.FV_F32, None, None, *ok, 0.01, None, None) == L.FV_E_BADARG     # null pointers


def test_cpu_tensors_are_rejected():
    net = fv.EFE_conv5(False, **TOY)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 3, 64, 64), None, torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops_efe.KpCatFn.apply(torch.zeros(1, 3, 2, 4, 4), torch.zeros(1, 3, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.ResBlock3D(30, False)(torch.zeros(1, 30, 2, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        fv.SameBlock3D(30, 15, False)(torch.zeros(1, 30, 2, 4, 4))


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("mode", ["direction", "non-direction"])
def test_contrastive_loss_matches_reference(mode):
    gd = load_golden("efe.pt")["contrastive"][mode.replace("-", "_")]
    seed = int(gd["seed"])
    torch.manual_seed(seed)
    crit = fv.ContrastiveLoss_linear(mode=mode).train()
    perturb_bn(crit, seed + 3)
    # channels_last inputs, as EFE_conv5 hands x_c / x_a_c over: the flatten order must stay NCHW
    f1 = gd["f1"].clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    f2 = gd["f2"].clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    loss = crit(f1, f2)
    loss.backward()
    assert _rel(loss, gd["loss"]) < 1e-4
    assert _rel(f1.grad, gd["d_f1"]) < 1e-4 and _rel(f2.grad, gd["d_f2"]) < 1e-4
    named = dict(crit.named_parameters())
    assert set(gd["grads"]) == {k for k, p in named.items() if p.grad is not None}
    for k, ref in gd["grads"].items():
        got = named[k].grad
        got = got[::16] if got.dim() == 2 else got       # the fixture keeps every 16th row of a matrix
        assert _rel(got, ref) < 1e-4, (k, _rel(got, ref))
    for k, ref in gd["buffers"].items():
        got = crit.state_dict()[k]
        assert _rel(got.float(), ref.float()) < 1e-4, k
    if mode != "direction":
        assert named["projection.6.bias"].grad is None
