"""Exact-operand parity of the 2-D conv kernel families: operands, float64 references, the
conditions that make the result independent of summation order, a bit comparator and a guarded
allocator.  Test infrastructure only; nothing here touches the GPU library, so the comparator
and every case's conditions are checked on the CPU (tests/test_exact_operands_cpu.py) and the
launches in tests/test_conv_exact_gpu.py.

The idea: with small-integer operands every product and every partial sum of a convolution is an
integer far below 2^24, hence exact in fp32 in ANY order.  Tile shape, split count, k order and
reduce tree then cannot change the accumulator, and a kernel's output must equal the float64
reference bit for bit after the one rounding to the output type.  What is left to go wrong is
what the test is after: an index, a boundary, a split, a tap, an epilogue.

Operands (all exact in bf16):
  activations, and the dy of a data gradient    integers in -2 .. 2
  weights, and the dy of a weight gradient      -1, 0, 1 (zeros: a share ZERO_SHARE, raised by
                                                thinning until a case's conditions hold)
  bias, residual                                integers in -3 .. 3
  prologue scale / shift                        0.5, 1, 2 / -1, 0, 1
  prologue slope                                0.25 in the forward, 0 (ReLU) in the weight gradient
The prologue's output act(x * scale + shift) is a multiple of 1/8 of magnitude <= 5.

Conditions (check_conditions; asserted on the CPU, they are properties of the inputs, not
tolerances).  With q the operand quantum (1; 1/8 behind a prologue):
  * A = sum of |terms| (conv(|x|, |w|) + |b|) of every output of every operation has
    A / q <= 2^CAP_LOG2: every partial sum, in any order, is a multiple of q below 2^24 q and so
    exact in fp32;
  * every product has magnitude <= 4 (<= 5 behind a prologue: 2 * 2 + 1);
  * the per-channel sum of |y| / q is <= 2^24, so a statistics record's sum is exact;
  * store-pass cases (a residual joins an already rounded tile): |conv + bias| + |res| <= 256,
    integers that bf16 holds exactly, so the result does not depend on where the kernel rounds.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

# log2 of the cap on A / q.  2^22 leaves two bits below fp32's 2^24.  If the bf16 MFMA turned out
# to align its products in a window narrower than fp32 (as the scaled fp8 MFMA does within a
# group of 8), 11 keeps every running sum inside 12 bits; the operands are then thinned to fit.
CAP_LOG2 = 22
ZERO_SHARE = 1.0 / 3.0
FWD_SLOPE = 0.25
CANARY = 1024.0          # exact in bf16
GUARD = 4096             # canary elements on each side of a guarded buffer

# ---------------------------------------------------------------------------- cases
# (k, cin, cout, H, W, ups, pro): the stride-1 cases of tests/test_kernels_gpu.py CONV_CASES
# (H, W is the conv INPUT size; the output is twice that under ups), and the smallest case of
# each kernel those do not reach: (3, 64, 128, 32, 64) for conv3c64_fwd, (3, 128, 256, 4, 64) for
# the 256-co tile of conv3_halo_fwd3 without a store pass.
#
# case -> the kernel kinds its bf16 launches take, as fv_conv2d_fwd_kernel names them (the
# FV_CONVK_* of include/facevae.h): (the forward, which asks for statistics records; the data
# gradient, None behind a prologue).  The same at every N a case runs at.  fp32 runs conv_fwd_kernel
# (V1) throughout.  tests/test_exact_operands_cpu.py holds the table against the library and asks
# that every kind appears in it; tests/test_conv_exact_gpu.py asserts the kind before each launch.
CONV_KINDS = {
    # the register-staged kernel: cin % 64 != 0, a BN prologue, or W % 8 != 0
    (3, 32, 64, 12, 10, False, False): ("V1", "V1"),
    (3, 64, 128, 16, 16, False, True): ("V1", None),
    (7, 64, 3, 16, 16, False, False): ("V1", "V1"),
    (3, 32, 32, 8, 6, True, True): ("V1", None),
    (3, 16, 32, 7, 9, False, False): ("V1", "V1"),
    (3, 64, 128, 12, 20, False, False): ("V1", "V1"),
    (3, 128, 64, 10, 6, True, False): ("V1", "V1"),
    (7, 64, 3, 9, 13, False, False): ("V1", "V1"),
    (1, 512, 256, 6, 10, False, False): ("V1", "V1"),
    # DMA-fed conv_fwd_v2 (cin % 64 == 0, W % 8 == 0) on one side or both; conv1x1_stream takes
    # the 1x1 data gradient (the forward asks for statistics, which it does not write)
    (1, 256, 512, 8, 8, False, False): ("V2", "C1S"),
    (7, 3, 64, 16, 16, False, False): ("V1", "V2"),
    (3, 128, 64, 8, 8, True, False): ("V2", "V2"),           # W / 2 % 16 != 0: no sub-pixel phases
    (3, 256, 256, 16, 16, False, False): ("V2", "V2"),
    (1, 128, 32, 8, 64, False, False): ("V2", "V1"),
    (1, 32, 128, 16, 64, False, False): ("V1", "V2"),
    (3, 64, 24, 8, 16, False, False): ("V2", "V1"),
    # 7x7 with W % 64 == 0: the packed in_conv kernel, the 7x7 halo kernel, the out_conv band kernel
    (7, 3, 64, 16, 64, False, False): ("C74", "HALO7"),
    (7, 64, 3, 8, 128, False, False): ("C7N", "C74"),
    (7, 64, 3, 20, 64, False, False): ("C7N", "C74"),
    (7, 64, 3, 64, 128, False, False): ("C7N", None),         # forward only, with FV_C7_BAND=64
    (7, 5, 64, 4, 64, False, False): ("HALO7", "HALO7"),
    # 3x3 with W % 64 == 0, H % 4 == 0.  64 -> 128 runs conv_fwd_v2 forward (halo3_bn: measured
    # faster) or, with H % 32 == 0, the 64-channel band kernel; its data gradient the 8-row 64-co
    # halo tile.  256 -> 256 at this size the 128-co halo tile, 128 -> 256 the 256-co one.
    (3, 64, 128, 8, 64, False, False): ("V2", "HALO3_FWD3"),
    (3, 64, 128, 32, 64, False, False): ("C64", "HALO3_FWD3"),
    (3, 256, 256, 4, 64, False, False): ("HALO3_FWD3", "HALO3_FWD3"),
    (3, 128, 256, 4, 64, False, False): ("HALO3_FWD3", "HALO3_FWD3"),
    (3, 128, 64, 12, 128, False, False): ("HALO3_FWD2", "V2"),    # 64-co tile, H % 8 != 0
    (3, 128, 64, 16, 64, False, False): ("HALO3_FWD3", "V2"),     # 64-co tile, 8 rows
    # sub-pixel phases of upsample + 3x3, and the data gradient at the low resolution
    (3, 128, 64, 16, 16, True, False): ("SUBPIX_V2", "DGRAD_LOWRES_V2"),
    (3, 256, 128, 16, 32, True, False): ("SUBPIX_V2", "DGRAD_LOWRES_V2"),
    (3, 128, 64, 8, 64, True, False): ("UPBAND", "DGRAD_LOWRES_HALO"),
    (3, 256, 128, 4, 64, True, False): ("SUBPIX_HALO", "DGRAD_LOWRES_HALO"),
    (3, 128, 128, 32, 64, True, False): ("UPBAND", "DGRAD_LOWRES_HALO"),
    # the full-size UpBlock2D convs: weight gradient only (their large-P plans)
    (3, 128, 64, 128, 128, True, False): (None, None),
    (3, 256, 128, 64, 64, True, False): (None, None),
}
CONV_CASES = list(CONV_KINDS)
C7_BAND_CASE = (7, 64, 3, 64, 128, False, False)
FULL_SIZE_UP = [(3, 128, 64, 128, 128, True, False), (3, 256, 128, 64, 64, True, False)]
# also at N = 1 and N = 3: pixel tiles straddle image boundaries / P is no multiple of a tile
N13_CASES = [
    (3, 32, 64, 12, 10, False, False),
    (3, 64, 128, 12, 20, False, False),
    (3, 64, 128, 8, 64, False, False),
    (3, 128, 64, 16, 16, True, False),
    (7, 64, 3, 20, 64, False, False),
    (1, 128, 32, 8, 64, False, False),
]
# (N, cin_valid, cout, H_out, W_out): tests/test_disc_gpu.py S2_CASES
S2_CASES = [
    (2, 5, 16, 16, 24),
    (2, 18, 64, 8, 8),
    (2, 64, 128, 6, 10),
    (3, 32, 32, 10, 14),
    (1, 128, 256, 4, 4),
    (2, 16, 24, 9, 7),
]
# name -> (cin, cout, N, H, W): tests/test_epilogue_gpu.py FWD_CASES a, b, c (bias + residual)
SR_CASES = {
    "a_256co": (128, 256, 1, 8, 64),
    "b_128co": (256, 256, 1, 8, 64),
    "c_64co": (128, 64, 1, 8, 64),
}
# all three are conv3_halo_fwd3 launches (residual, store-pass mode 1): co tiles of 256, 128 and 64 (8 rows)
SR_KINDS = {"a_256co": "HALO3_FWD3", "b_128co": "HALO3_FWD3", "c_64co": "HALO3_FWD3"}
# the data gradient of test_epilogue_gpu.dgrad_case through fv_conv2d_bwd_data_sr (dx only;
# store-pass mode 2 on the 8-row 64-co tile of conv3_halo_fwd3)
SR_DGRAD_CASE = (3, 64, 128, 8, 64, False, False)
SR_DGRAD_KIND = "HALO3_FWD3"


def conv_kinds(case, dtype):
    """(forward, data gradient) kernel kinds of a case in dtype: CONV_KINDS in bf16, V1 in fp32"""
    f, g = CONV_KINDS[case]
    return (f, g) if dtype == torch.bfloat16 else (f and "V1", g and "V1")


def _with_n(cases, ns):
    return [(c, n) for c in cases for n in ns]


FWD_LIST = _with_n([c for c in CONV_CASES if c not in FULL_SIZE_UP], [2]) + _with_n(N13_CASES, [1, 3])
BWD_LIST = _with_n([c for c in CONV_CASES if c not in FULL_SIZE_UP and c != C7_BAND_CASE], [2]) + _with_n(N13_CASES, [1, 3])
WGRAD_LIST = BWD_LIST + _with_n(FULL_SIZE_UP, [2])
DGRAD_LIST = [(c, n) for c, n in BWD_LIST if not c[6]]       # as test_conv_bwd: no dgrad behind a prologue


def case_id(v):
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], tuple):
        (k, cin, cout, H, W, ups, pro), n = v
        return f"k{k}_{cin}to{cout}_{H}x{W}{'_ups' if ups else ''}{'_pro' if pro else ''}_n{n}"
    if isinstance(v, tuple):
        return "_".join(str(i) for i in v)
    return str(v)


# ---------------------------------------------------------------------------- operands
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(shape, lo, hi, g):
    """integers in lo .. hi (inclusive) as float64"""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


class _Ternary:
    """-1 / 0 / 1 tensor whose share of zeros can be raised without redrawing: thinning only ever
    clears entries, so a thinner tensor is a masked copy of a denser one."""

    def __init__(self, shape, g):
        self.u = torch.rand(shape, generator=g, dtype=torch.float64)
        self.s = _ints(shape, 0, 1, g) * 2 - 1

    def at(self, zero_share):
        return (self.u >= zero_share).double() * self.s


def prologue(x, sc, sh, slope):
    v = x * sc[None, :, None, None] + sh[None, :, None, None]
    return torch.where(v > 0, v, v * slope)


def conv_input(x, ups, pro):
    """what the conv multiplies: the prologue (sc, sh, slope) or None, then the nearest x2 upsample"""
    if pro is not None:
        x = prologue(x, *pro)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return x


def pool2_sum(t):
    """sums of the 2x2 quads (the backward of a nearest x2 upsample), exact on integers"""
    N, C, H, W = t.shape
    return t.view(N, C, H // 2, 2, W // 2, 2).sum((3, 5))


# ---------------------------------------------------------------------------- float64 references
def ref_forward(x, w, b, k, ups=False, pro=None, stride=1):
    return F.conv2d(conv_input(x, ups, pro), w, b, stride=stride, padding=k // 2)


def ref_dgrad(xi_shape, w, gy, k, stride=1):
    """dL/d(conv input) at the conv's own resolution (the upsampled one under ups), by autograd"""
    xi = torch.zeros(xi_shape, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xi, w, None, stride=stride, padding=k // 2)
    return torch.autograd.grad(y, xi, gy)[0]


def ref_wgrad(xi, w_shape, gy, k, stride=1):
    dw = torch.nn.grad.conv2d_weight(xi, w_shape, gy, stride=stride, padding=k // 2)
    return dw, gy.sum((0, 2, 3))


def _abs_fwd(xi, w, b, k, stride, s):
    """A of a forward in units of q = 1 / s, in fp32 (exact below 2^24; a sum of non-negative
    terms above that cannot round down past the cap)"""
    a = F.conv2d(xi.abs().float() * s, w.abs().float(), None, stride=stride, padding=k // 2)
    return a + (b.abs().float() * s)[None, :, None, None] if b is not None else a


def _abs_dgrad(xi_shape, w, gy, k, stride):
    if stride == 1:
        return F.conv_transpose2d(gy.abs().float(), w.abs().float(), None, padding=k // 2)
    return F.conv_transpose2d(gy.abs().float(), w.abs().float(), None, stride=stride, padding=k // 2, output_padding=1)


def _abs_wgrad(xi, w_shape, gy, k, stride, s):
    return torch.nn.grad.conv2d_weight(xi.abs().float() * s, w_shape, gy.abs().float(), stride=stride, padding=k // 2)


class ExactCase:
    """Operands, conditions and float64 references of one conv case; every tensor is float64 on
    the CPU, computed once on first use and never modified.

    Stride 1: (k, cin, cout, H, W, ups, pro) with (H, W) the conv input size.  Stride 2
    (stride=2): k = 3, (H, W) the OUTPUT size, the input (2H, 2W).  res=True adds a residual
    and the store-pass condition |conv + bias| + |res| <= 256."""

    def __init__(self, case, N, stride=1, res=False, cap_log2=None):
        self.k, self.cin, self.cout, self.H, self.W, self.ups, self.pro = case
        self.N, self.stride, self.res, self.case = N, stride, res, case
        self.cap = float(2 ** (CAP_LOG2 if cap_log2 is None else cap_log2))
        self.s = 8.0 if self.pro else 1.0                 # 1 / q
        k, cin, cout = self.k, self.cin, self.cout
        g = _gen("exact", case, N, stride, res)
        hin, win = (2 * self.H, 2 * self.W) if stride == 2 else (self.H, self.W)
        self.x = _ints((N, cin, hin, win), -2, 2, g)
        self._w = _Ternary((cout, cin, k, k), g)
        self.b = _ints((cout,), -3, 3, g)
        self.sc = torch.exp2(_ints((cin,), -1, 1, g))
        self.sh = _ints((cin,), -1, 1, g)
        ho, wo = (self.H, self.W) if stride == 2 else ((2 * self.H, 2 * self.W) if self.ups else (self.H, self.W))
        self.out_shape = (N, cout, ho, wo)
        self.r = _ints(self.out_shape, -3, 3, g) if res else None
        self.gy_d = _ints(self.out_shape, -2, 2, g)
        self._gy_w = _Ternary(self.out_shape, g)
        self.pro_fwd = (self.sc, self.sh, FWD_SLOPE) if self.pro else None
        self.pro_wg = (self.sc, self.sh, 0.0) if self.pro else None

    # -- operands whose zero share depends on the conditions
    def _w_ok(self, w):
        xi = conv_input(self.x, self.ups, self.pro_fwd)
        if _abs_fwd(xi, w, self.b, self.k, self.stride, self.s).max().item() > self.cap:
            return False
        if not self.pro:
            a = _abs_dgrad(xi.shape, w, self.gy_d, self.k, self.stride)
            if (pool2_sum(a) if self.ups else a).max().item() > self.cap:
                return False
        if self.res:
            y = F.conv2d(xi, w, self.b, padding=self.k // 2)
            return (y.abs() + self.r.abs()).max().item() <= 256
        return True

    @functools.cached_property
    def w_zero_share(self):
        z = ZERO_SHARE
        while not self._w_ok(self._w.at(z)):
            z = 1 - (1 - z) * 0.75
        return z

    @functools.cached_property
    def w(self):
        return self._w.at(self.w_zero_share)

    @functools.cached_property
    def xi_wg(self):
        return conv_input(self.x, self.ups, self.pro_wg)

    @functools.cached_property
    def gy_w_zero_share(self):
        z = ZERO_SHARE
        shape = (self.cout, self.cin, self.k, self.k)
        while max(_abs_wgrad(self.xi_wg, shape, self._gy_w.at(z), self.k, self.stride, self.s).max().item(),
                  self._gy_w.at(z).abs().sum((0, 2, 3)).max().item()) > self.cap:
            z = 1 - (1 - z) * 0.75
        return z

    @functools.cached_property
    def gy_w(self):
        return self._gy_w.at(self.gy_w_zero_share)

    # -- float64 references
    @functools.cached_property
    def y(self):
        """conv + bias (the fp32 accumulator the statistics see)"""
        return ref_forward(self.x, self.w, self.b, self.k, self.ups, self.pro_fwd, self.stride)

    @functools.cached_property
    def dx_conv(self):
        """data gradient at the conv's resolution (the high one under ups)"""
        assert not self.pro
        N, _, ho, wo = self.out_shape
        shape = (N, self.cin, 2 * ho, 2 * wo) if self.stride == 2 else (N, self.cin, ho, wo)
        return ref_dgrad(shape, self.w, self.gy_d, self.k, self.stride)

    @functools.cached_property
    def dw_db(self):
        return ref_wgrad(self.xi_wg, (self.cout, self.cin, self.k, self.k), self.gy_w, self.k, self.stride)

    # -- conditions
    def check_conditions(self, ops=("fwd", "dgrad", "wgrad")):
        """Assert the conditions of the module docstring for the listed operations; returns the
        measured figures."""
        out = {}
        cap, s, k = self.cap, self.s, self.k
        pmax = 5.0 if self.pro else 4.0
        if "fwd" in ops:
            xi = conv_input(self.x, self.ups, self.pro_fwd)
            assert bool((xi * s == torch.round(xi * s)).all()) and bool((self.w == torch.round(self.w)).all())
            out["fwd_A"] = _abs_fwd(xi, self.w, self.b, k, self.stride, s).max().item()
            out["fwd_prod"] = (xi.abs().max() * self.w.abs().max()).item()
            out["fwd_max"] = self.y.abs().max().item()
            out["fwd_chan_sum"] = (self.y.abs().sum((0, 2, 3)).max() * s).item()
            assert out["fwd_A"] <= cap, out
            assert out["fwd_prod"] <= pmax, out
            assert out["fwd_chan_sum"] <= 2.0 ** 24, out
            assert bool((self.y * s == torch.round(self.y * s)).all()), "reference is not a multiple of q"
            if self.res:
                out["sr_max"] = (self.y.abs() + self.r.abs()).max().item()
                assert out["sr_max"] <= 256, out
        if "dgrad" in ops:
            assert not self.pro
            a = _abs_dgrad(None, self.w, self.gy_d, k, self.stride)
            out["dgrad_A"] = (pool2_sum(a) if self.ups else a).max().item()
            out["dgrad_prod"] = (self.gy_d.abs().max() * self.w.abs().max()).item()
            out["dgrad_max"] = self.dx_conv.abs().max().item()
            assert out["dgrad_A"] <= cap and out["dgrad_prod"] <= 4.0, out
        if "wgrad" in ops:
            out["wgrad_A"] = _abs_wgrad(self.xi_wg, (self.cout, self.cin, k, k), self.gy_w, k, self.stride, s).max().item()
            out["bgrad_A"] = self.gy_w.abs().sum((0, 2, 3)).max().item()
            out["wgrad_prod"] = (self.xi_wg.abs().max() * self.gy_w.abs().max()).item()
            assert out["wgrad_A"] <= cap and out["bgrad_A"] <= cap and out["wgrad_prod"] <= pmax, out
        return out


@functools.lru_cache(maxsize=None)
def conv_case(case, N):
    return ExactCase(case, N)


@functools.lru_cache(maxsize=None)
def s2_case(case):
    N, cin, cout, H, W = case
    return ExactCase((3, cin, cout, H, W, False, False), N, stride=2)


@functools.lru_cache(maxsize=None)
def sr_case(name):
    cin, cout, N, H, W = SR_CASES[name]
    return ExactCase((3, cin, cout, H, W, False, False), N, res=True)


# ---------------------------------------------------------------------------- comparator
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def mismatches(got, want):
    """-> (mask of mismatching elements, want rounded to got's dtype): the raw bits differ, or
    either side is NaN (a NaN never matches, not even the same NaN).  want.to(dtype) is torch's
    round-to-nearest-even, the rounding of the kernels' stores."""
    got = got.detach().cpu()
    want = want.detach().cpu()
    assert got.shape == want.shape, f"shape {tuple(got.shape)} against reference {tuple(want.shape)}"
    wr = want.to(got.dtype)
    it = _BITS[got.dtype]
    bad = got.contiguous().view(it) != wr.contiguous().view(it)
    bad |= torch.isnan(got) | torch.isnan(wr)
    return bad, wr


def mismatch_report(got, want):
    """-> None when got equals want bit for bit, else a dict: count, total, the first ten
    coordinates with both values, and the bounding box (lo, hi inclusive per dimension)."""
    bad, wr = mismatches(got, want)
    n = int(bad.sum())
    if n == 0:
        return None
    idx = bad.nonzero()
    g = got.detach().cpu()
    first = [(tuple(int(i) for i in c), float(g[tuple(c)]), float(wr[tuple(c)])) for c in idx[:10]]
    return dict(count=n, total=bad.numel(), first=first, lo=tuple(int(i) for i in idx.min(0).values),
                hi=tuple(int(i) for i in idx.max(0).values))


def assert_exact(got, want, what):
    """got (bf16 / fp32, any device) must equal want (float64) bit for bit after want.to(dtype)."""
    rep = mismatch_report(got, want)
    if rep is None:
        return
    names = {4: "nchw", 5: "ncdhw"}.get(got.dim()) or [f"d{i}" for i in range(got.dim())]
    lines = [f"{what}: {rep['count']} of {rep['total']} elements differ from the float64 reference "
             f"(as {got.dtype}); coordinates are ({', '.join(names)})",
             "  bounding box: " + ", ".join(f"{a}..{b}" for a, b in zip(rep["lo"], rep["hi"]))
             + f"  of shape {tuple(got.shape)}"]
    lines += [f"  {c}: got {g!r}, want {w!r}" for c, g, w in rep["first"]]
    raise AssertionError("\n".join(lines))


# ---------------------------------------------------------------------------- guarded allocation
class Guarded:
    """A flat buffer [GUARD canary | numel NaN | GUARD canary]; `t` is the middle part shaped for
    the launch.  A kernel must write every element it owns (no NaN left where the test looks) and
    nothing else (check_canary)."""

    def __init__(self, shape, dtype, device="cuda", nhwc=False, ndhwc=False):
        numel = math.prod(shape)
        self.buf = torch.full((numel + 2 * GUARD,), CANARY, dtype=dtype, device=device)
        self.flat = self.buf[GUARD:GUARD + numel]
        self.flat.fill_(float("nan"))
        if nhwc:          # logical NCHW shape over NHWC memory (torch.channels_last)
            N, C, H, W = shape
            self.t = self.flat.view(N, H, W, C).permute(0, 3, 1, 2)
        elif ndhwc:       # logical NCDHW shape over NDHWC memory (torch.channels_last_3d)
            N, C, D, H, W = shape
            self.t = self.flat.view(N, D, H, W, C).permute(0, 4, 1, 2, 3)
        else:
            self.t = self.flat.view(shape)

    def data_ptr(self):
        return self.flat.data_ptr()

    def check_canary(self, what):
        n = self.flat.numel()
        lo, hi = self.buf[:GUARD], self.buf[GUARD + n:]
        bl, bh = (lo != CANARY).nonzero().flatten().cpu(), (hi != CANARY).nonzero().flatten().cpu()
        assert bl.numel() == 0 and bh.numel() == 0, (
            f"{what}: written outside the buffer of {n} elements: {bl.numel()} before it (nearest at "
            f"{int(bl.max()) - GUARD if bl.numel() else None}), {bh.numel()} after it (first at offset "
            f"{n + int(bh.min()) if bh.numel() else None})")
