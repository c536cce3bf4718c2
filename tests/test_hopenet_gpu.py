"""The frozen Hopenet teacher on one MI355X: the preprocessing kernel (bit-equal to torch on the
CPU), the pointwise inference GEMM against torch fp64 on the same rounded operands, one frozen
bottleneck against the product's own ResBottleneck, and the module against the fixture made from the
reference (tests/golden/hopenet.pt; regenerated weights, tests/hopenet_reference.py).

Gates: rel-L2 <= 1e-5 for fp32 results; rel-L2 <= 4e-3 and |d| <= 1.6e-2 max|ref| for
bf16-stored results; 1e-3 rel-L2 for a module's fp32 maps and 3.1e-4 rad for its angles; in bf16
mode 3 x the deviation of the reference's own bf16 emulation (stored in the fixture)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import _lib as L, ops, ops_hopenet as OH  # noqa: E402
from facevae_amd.hopenet import Bottleneck  # noqa: E402
from golden_io import load_golden  # noqa: E402
import hopenet_reference as R  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
GUARD, SENT = 1024, 777.0          # elements on either side of an output


def lib_status(name, *args):
    return getattr(L.load(), name)(*args)


def guarded(n, dtype):
    """-> (the whole buffer, the n-element view between two sentinel regions)."""
    raw = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
    return raw, raw[GUARD:GUARD + n]


def guards_intact(raw):
    return bool((raw[:GUARD] == SENT).all()) and bool((raw[-GUARD:] == SENT).all())


def gates(y, ref, dtype, what):
    y, ref = y.double().cpu(), ref.double().cpu()
    r = ((y - ref).norm() / ref.norm()).item()
    m = ((y - ref).abs().max() / ref.abs().max()).item()
    print(f"{what} [{'bf16' if dtype == BF16 else 'fp32'}]: rel-L2 {r:.3e}  max|d|/max|ref| {m:.3e}")
    if dtype == F32:
        assert r <= 1e-5, (what, r)
    else:
        assert r <= 4e-3 and m <= 1.6e-2, (what, r, m)


# ---------------------------------------------------------------------------------- preprocessing
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("src,dst", [((40, 56), (224, 224)), ((256, 256), (224, 224)), ((17, 23), (9, 31)),
                                     ((224, 224), (224, 224)), ((3, 5), (7, 2))])
def test_prep_bit_equal_to_torch_cpu(src, dst, n):
    x = torch.rand(n, 3, *src, generator=torch.Generator().manual_seed(src[0] + 7 * n))
    want = R.preprocess_torch(x, dst)
    raw, y = guarded(n * 3 * dst[0] * dst[1], F32)
    m3, s3 = (ctypes.c_float * 3)(*OH.IMAGENET_MEAN), (ctypes.c_float * 3)(*OH.IMAGENET_STD)
    xg = x.to(DEV)
    L.call("fv_hopenet_prep_fwd", xg.data_ptr(), n, src[0], src[1], dst[0], dst[1], m3, s3, y.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().view(n, 3, *dst), want)
    assert guards_intact(raw)
    assert torch.equal(fv.Hopenet(None, [1, 1, 1, 1], 6).preprocess(xg, dst).cpu(), want)


def test_prep_limits_return_unsupported():
    x = torch.zeros(64, device=DEV)
    m3, s3 = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    for n, h, w, ho, wo in ((0, 4, 4, 2, 2), (65536, 1, 1, 1, 1), (1, 0, 4, 2, 2), (1, 4, 4, 2, 0), (1, 4, 4, -1, 2),
                            (1, 46341, 46341, 2, 2), (1, 4, 4, 46341, 46341)):
        st = lib_status("fv_hopenet_prep_fwd", x.data_ptr(), n, h, w, ho, wo, m3, s3, x.data_ptr(), L.stream())
        assert st == L.FV_E_UNSUPPORTED, (n, h, w, ho, wo, st)


# ---------------------------------------------------------------------------------- pointwise GEMM
PW_CASES = [
    (2, 7, 7, 32, 32, 1),        # 98 pixels: a short last tile
    (1, 6, 10, 96, 64, 2),       # 15 output pixels, less than one tile; stride addressing
    (3, 5, 9, 160, 96, 1),       # several K steps; widths that are not powers of two
    (1, 16, 16, 64, 256, 1),     # several column tiles
    (2, 8, 12, 2048, 32, 1),     # the deepest K of the workload
    (1, 4, 4, 32, 2048, 1),      # the widest output
    (8, 64, 64, 32, 128, 1),     # 256 pixel tiles x 128 channels: the 128-channel tile's threshold
    (8, 64, 64, 32, 128, 2),     # the same output channels below it: 64 pixel tiles of the 64-channel tile
]
SWITCHES = ("scale", "shift", "res", "in_relu", "out_relu")


def pw_operands(case, dtype, on, seed=0):
    n, h, w, cin, cout, s = case
    g = torch.Generator().manual_seed(1000 + seed + cin + cout)
    ho, wo = h // s, w // s
    x = torch.randn(n, h, w, cin, generator=g).to(dtype)                          # both signs: the ReLUs matter
    wt = torch.randn(cout, cin, generator=g) / cin ** 0.5
    scale = (0.5 + torch.rand(cout, generator=g)) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1).float()
    shift = 0.5 * torch.randn(cout, generator=g)
    res = torch.randn(n, ho, wo, cout, generator=g).to(dtype)
    return dict(x=x, w=wt, scale=scale if "scale" in on else None, shift=shift if "shift" in on else None,
                res=res if "res" in on else None, in_relu="in_relu" in on, out_relu="out_relu" in on)


def pw_reference(case, dtype, o):
    """fp64 on the rounded operands: x and res as stored, w * scale formed in fp32 and rounded once."""
    s = case[5]
    wk = (o["w"] * o["scale"].view(-1, 1) if o["scale"] is not None else o["w"]).to(dtype).double()
    x = o["x"][:, ::s, ::s, :].double()
    if o["in_relu"]:
        x = x.clamp(min=0)
    y = x @ wk.t()
    if o["shift"] is not None:
        y = y + o["shift"].double()
    if o["res"] is not None:
        y = y + o["res"].double()
    return y.clamp(min=0) if o["out_relu"] else y


def pw_run(case, dtype, o):
    n, h, w, cin, cout, s = case
    d = OH.pw_desc(dtype, n, h, w, s, cin, cout, o["in_relu"], o["out_relu"])
    assert L.query("fv_pw_infer_wk_elems", ctypes.byref(d)) == cout * cin
    wraw, wk = guarded(cout * cin, dtype)
    wd = o["w"].to(DEV)
    sc = o["scale"].to(DEV) if o["scale"] is not None else None
    L.call("fv_pw_infer_weight_prep", ctypes.byref(d), wd.data_ptr(), L.ptr(sc), wk.data_ptr(), L.stream())
    xd = o["x"].to(DEV)
    sh = o["shift"].to(DEV) if o["shift"] is not None else None
    rs = o["res"].to(DEV) if o["res"] is not None else None
    outs = []
    for _ in range(2):
        raw, y = guarded(n * (h // s) * (w // s) * cout, dtype)
        L.call("fv_pw_infer_fwd", ctypes.byref(d), xd.data_ptr(), wk.data_ptr(), L.ptr(sh), L.ptr(rs), y.data_ptr(), L.stream())
        torch.cuda.synchronize()
        assert guards_intact(raw) and guards_intact(wraw)
        outs.append(y.clone())
    assert torch.equal(outs[0], outs[1])                                           # reruns are bit-identical
    return outs[0].view(n, h // s, w // s, cout)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("on", [(), SWITCHES], ids=["plain", "all"])
@pytest.mark.parametrize("case", PW_CASES, ids=lambda c: "x".join(map(str, c)))
def test_pw_infer_vs_fp64(case, on, dtype):
    o = pw_operands(case, dtype, on)
    gates(pw_run(case, dtype, o), pw_reference(case, dtype, o), dtype, f"pw {case} {'all' if on else 'plain'}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("switch", SWITCHES)
def test_pw_infer_each_switch_alone(switch, dtype):
    case = PW_CASES[2]
    o = pw_operands(case, dtype, (switch,), seed=3)
    ref = pw_reference(case, dtype, o)
    plain = pw_reference(case, dtype, pw_operands(case, dtype, (), seed=3))
    assert ((ref - plain).norm() / plain.norm()).item() > 0.1                      # the switch matters on these operands
    gates(pw_run(case, dtype, o), ref, dtype, f"pw {case} {switch}")


def test_pw_infer_refusals():
    buf = torch.zeros(1 << 16, device=DEV)
    p = buf.data_ptr()
    q = p + (1 << 17)

    def fwd(n, h, w, s, cin, cout, y=None, res=None, x=None):
        d = OH.pw_desc(F32, n, h, w, s, cin, cout)
        return d, lib_status("fv_pw_infer_fwd", ctypes.byref(d), x or p, p, None, res, y or q, L.stream())

    for bad in ((1, 4, 4, 1, 24, 32), (1, 4, 4, 1, 32, 48), (1, 4, 4, 3, 32, 32), (1, 5, 4, 2, 32, 32), (1, 4, 5, 2, 32, 32),
                (0, 4, 4, 1, 32, 32), (1, 4, 4, 1, 8192, 32), (1, 4, 4, 1, 32, 0)):
        d, st = fwd(*bad)
        assert st == L.FV_E_UNSUPPORTED, (bad, st)
        assert L.query("fv_pw_infer_wk_elems", ctypes.byref(d)) == 0
        assert lib_status("fv_pw_infer_weight_prep", ctypes.byref(d), p, None, p, L.stream()) == L.FV_E_UNSUPPORTED
    d = OH.pw_desc(torch.float64, 1, 4, 4, 1, 32, 32)
    assert lib_status("fv_pw_infer_fwd", ctypes.byref(d), p, p, None, None, q, L.stream()) == L.FV_E_UNSUPPORTED
    assert fwd(1, 4, 4, 1, 32, 32, y=p)[1] == L.FV_E_BADARG                        # y is x
    assert fwd(1, 4, 4, 1, 32, 32, y=p + 64)[1] == L.FV_E_BADARG                   # y overlaps x
    assert fwd(1, 4, 4, 1, 32, 32, x=p + 8192, y=p, res=p)[1] == L.FV_E_BADARG     # y is res
    assert b"alias" in L.load().fv_last_error()
    assert fwd(1, 4, 4, 1, 32, 32, x=p, y=p + 2048, res=p + 8192)[1] == 0         # adjacent, not overlapping


def randomise_bn(mods, g, signed=True):
    with torch.no_grad():
        for m in mods:
            c = m.num_features
            m.running_mean.copy_(0.2 * torch.randn(c, generator=g))
            m.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
            sign = (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float() if signed else 1.0
            m.weight.copy_((0.5 + torch.rand(c, generator=g)) * sign)
            m.bias.copy_(0.1 * torch.randn(c, generator=g))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_frozen_bottleneck_equals_resbottleneck(dtype):
    """64 -> 256 with projection, 7 x 7, N = 2, against ResBottleneck(...).eval() in fp32 with zero
    conv biases and the same weights and statistics, on the same (rounded) input."""
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(21)
    ref = fv.ResBottleneck(64, 256, 1, False)
    stages = list(ref.layers) + [ref.down_sample]
    randomise_bn([s.bn for s in stages], g)
    with torch.no_grad():
        for s in stages:
            s.conv.bias.zero_()
    ds = torch.nn.Sequential(torch.nn.Conv2d(64, 256, 1, bias=False), torch.nn.BatchNorm2d(256))
    blk = Bottleneck(64, 64, 1, ds).eval()
    pairs = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3), (ds[0], ds[1])]
    with torch.no_grad():
        for (conv, bn), s in zip(pairs, stages):
            conv.weight.copy_(s.conv.weight)
            bn.load_state_dict(s.bn.state_dict())
    x = torch.randn(2, 64, 7, 7, generator=g).to(dtype).float().to(DEV)
    ref = ref.to(DEV).eval().set_compute_dtype(F32)
    with torch.no_grad():
        want = ref(x).float()
        got = OH._FrozenBlock(blk.to(DEV), dtype).forward(x.to(dtype).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert got.dtype == dtype and got.shape == want.shape
    gates(got.float(), want, dtype, "frozen bottleneck 64 -> 256, 7 x 7")


# ---------------------------------------------------------------------------------- the module
@pytest.fixture(scope="module")
def gold():
    return load_golden("hopenet.pt")


@pytest.fixture(scope="module")
def frames():
    return R.make_inputs().to(DEV)


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(name):
        if name not in cache:
            layers, bins, gain = R.NETS[name]
            cache[name] = R.build(fv.Hopenet, layers, bins, gain).to(DEV)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(R.NETS))
def test_module_fp32_matches_reference(gold, frames, nets, name):
    g = gold[name]
    net = nets(name).set_compute_dtype(F32)
    x = net.preprocess(frames)
    assert torch.equal(R.checksum(x.cpu()), g["prep_sum"])                         # bit-equal preprocessing
    taps = []
    feat = net._features(x, taps)
    ang = torch.stack(net.teacher_angles(frames))
    assert ang.shape == (3, 3) and ang.dtype == F32 and not ang.requires_grad
    df, da = R.rel_l2(feat.cpu(), g["features"]), (ang.cpu() - g["angles"]).abs().max().item()
    dt = [R.rel_l2(R.sample(t.cpu()), g["taps"][str(i)]) for i, t in enumerate(taps)]
    print(f"{name} fp32: features {df:.2e} rel-L2, angles {da:.2e} rad, taps {['%.1e' % v for v in dt]}")
    assert len(taps) == 5 and max(dt) <= 1e-3
    assert df <= 1e-3 and da <= 3.1e-4
    again = torch.stack(net.forward(x))
    assert torch.equal(again, ang)                                                 # cached plan, bit-identical rerun


@pytest.mark.parametrize("name", list(R.NETS))
def test_module_bf16_within_three_emulation_deviations(gold, frames, nets, name):
    g = gold[name]
    net = nets(name).set_compute_dtype(BF16)
    x = net.preprocess(frames)
    feat = net._features(x)
    ang = torch.stack(net.forward(x))
    df, da = R.rel_l2(feat.cpu(), g["features"]), (ang.cpu() - g["angles"]).abs().max().item()
    ef, ea = g["bf16_dev"].tolist()
    print(f"{name} bf16: features {df:.2e} rel-L2 (emulation {ef:.2e}), angles {da:.2e} rad (emulation {ea:.2e})")
    net.set_compute_dtype(ops.FP8)                                                 # fp8 mode runs in bf16
    assert torch.equal(torch.stack(net.forward(x)), ang)
    net.set_compute_dtype(F32)
    assert df <= 3 * ef and da <= 3 * ea


def test_cache_follows_load_state_dict(frames, nets):
    net = R.build(fv.Hopenet, (1, 1, 1, 1), 66).to(DEV).set_compute_dtype(F32)
    first = torch.stack(net.teacher_angles(frames))
    other = R.build(R.RefHopenet, (1, 1, 1, 1), 66, seed=91, stat_seed=92)
    want = other(R.preprocess(frames.cpu()))
    net.load_state_dict(other.state_dict(), strict=True)
    got = torch.stack(net.teacher_angles(frames)).cpu()
    assert (got - want).abs().max().item() <= 3.1e-4
    assert (got - first.cpu()).abs().max().item() > 1e-2                           # the outputs moved with the weights
    with torch.no_grad():                                                          # an in-place edit bumps _version
        net.bn1.bias.add_(0.5)
        other.bn1.bias.add_(0.5)
    moved = torch.stack(net.teacher_angles(frames)).cpu()
    assert (moved - other(R.preprocess(frames.cpu()))).abs().max().item() <= 3.1e-4
    assert (moved - got).abs().max().item() > 1e-3


def test_wrong_input_size_names_the_plane(nets):
    net = nets("bins6")
    with pytest.raises(ValueError, match="7 x 7"):
        net(torch.rand(1, 3, 192, 192, device=DEV))
    with pytest.raises(ValueError, match="7 x 7"):
        net.teacher_angles(torch.rand(1, 3, 40, 56, device=DEV), size=(224, 256))


def test_head_pose_loss_with_teacher(frames, nets):
    teacher = nets("bins6").set_compute_dtype(F32)
    torch.manual_seed(5)
    hpe = fv.HPE_EDE(False, n_filters=[16, 32, 64], n_blocks=[1, 1], n_bins=6, K=3).to(DEV).train()
    img = torch.rand(3, 3, 32, 64, generator=torch.Generator().manual_seed(6)).to(DEV)
    yaw, pitch, roll, _, _ = hpe(img)
    loss = fv.HeadPoseLoss()(yaw, pitch, roll, *teacher.teacher_angles(img))
    loss.backward()
    assert torch.isfinite(loss).item() and loss.item() > 0
    assert sum(float(p.grad.abs().sum()) for p in hpe.parameters() if p.grad is not None) > 0
    assert all(p.grad is None for p in teacher.parameters())
