"""Exact-operand parity of the 3-D conv kernels (csrc/conv3d.hip, csrc/conv3d_gemm.hip): the
case tables, operands, float64 references and conditions.  The idea, the operand generators, the
comparator and the guarded allocator are those of tests/exact_operands.py;
this file adds the third dimension and the plans each case is there to reach (section 20).
Nothing here touches the GPU library: the conditions and the comparator are checked on the CPU
(tests/test_exact_operands3d_cpu.py), the launches are in tests/test_conv3d_exact_gpu.py.

Operands (all exact in bf16):
  activations, and the dy of a data gradient    integers in -2 .. 2
  weights, and the dy of a weight gradient      -1, 0, 1, thinned until the conditions hold
  bias, residual                                integers in -3 .. 3

Conditions (ExactCase3.check_conditions; properties of the inputs, not tolerances):
  * A = sum of |terms| of every output of every operation <= 2^CAP_LOG2: every partial sum in any
    order is an integer below 2^24, exact in fp32;
  * every product has magnitude <= 4;
  * sr cases (a residual or a statistics record is involved): |conv + bias| + |res| <= 256, so
    conv + bias and conv + bias + res are integers that bf16 holds: it does not matter where the
    kernel rounds, and a record accumulated from the stored bf16 value sees the reference's value.
    A record then sums block_pixels <= 2112 integers of magnitude <= 256: exact in fp32.
The thinning loop (_wy) tests exactly the conditions check_conditions asserts for the weights.

References: float64 on the CPU -- F.conv3d (behind the nearest (1, 2, 2) upsample under ups),
autograd for dx, torch.nn.grad.conv3d_weight for dw, dy.sum for db.  They are computed in slices
over N (a conv is independent per image; dw and db are sums over images, exact in float64), so
the two large cases stay within a few hundred MB of scratch, once per case.
"""
import functools

import torch
import torch.nn.functional as F

from exact_operands import (CANARY, CAP_LOG2, GUARD, ZERO_SHARE, Guarded, _Ternary, _gen, _ints,  # noqa: F401
                            assert_exact, mismatch_report)

BF16, F32 = torch.bfloat16, torch.float32

# ---------------------------------------------------------------------------- case tables
# C = 32 fast path (bf16, cin = cout = 32, W = 64, H % 4 == 0):
# (N, D, H, forward kernel, forward chunks ndc, chunk length, wgrad images per block, wgrad chunks)
# derived by hand from c3_ndc / c3r_chunk_ok / c3w_nper / c3w_ndc of csrc/conv3d.hip; the GPU test
# asserts them through the public queries before it launches.  Not covered: c3w_nper = 4 and the
# depth-chunk loop of c3w_ndc at large batch (both need N * H >= 4096 rows).
C32_CASES = [
    (1, 1, 4, "fwd", 1, 1, 1, 1),        # D = 1: both depth neighbours outside the volume
    (2, 2, 8, "fwd", 1, 2, 1, 1),        # 4-slot ring, chunk of 2; two row tiles, two images
    (1, 3, 4, "fwd", 1, 3, 1, 1),        # chunk of 3: every ring slot live once
    (1, 5, 4, "fwd", 1, 5, 1, 1),        # chunk of 5: the ring wraps
    (1, 6, 4, "fwd", 2, 3, 1, 1),        # two chunks of 3: a chunk that starts at d0 = 3 (slot phase 3)
    (1, 12, 4, "fwd", 4, 3, 1, 2),       # four chunks of 3; wgrad 2 x 6 (chunk start 6: x-ring phase 2)
    (2, 4, 8, "dr", 1, 4, 1, 1),         # dr, 2 peeled groups (no steady-state loop)
    (1, 7, 4, "dr", 1, 7, 1, 1),         # dr, 3 groups: one pass of the steady-state loop
    (1, 8, 4, "dr", 2, 4, 1, 2),         # dr, 2 x 4 at small N; wgrad 2 x 4
    (1, 10, 4, "dr", 1, 10, 1, 2),       # dr, 4 groups; wgrad 2 x 5 (chunk start 5: phase 1)
    (1, 13, 8, "dr", 1, 13, 1, 2),       # dr, 5 groups; wgrad ragged 7 + 6
    (1, 16, 12, "dr", 4, 4, 1, 4),       # dr, 4 x 4; three row tiles: top, middle and bottom halo
    (3, 19, 4, "dr", 1, 19, 1, 4),       # dr, 7 groups; wgrad ragged 5, 5, 5, 4; odd N
    (1, 9, 4, "fwd", 1, 9, 1, 2),        # non-dr 9; wgrad ragged 5 + 4
    (1, 17, 4, "fwd", 1, 17, 1, 4),      # non-dr 17; wgrad ragged 5, 5, 5, 2
    (1, 33, 4, "fwd", 1, 33, 1, 8),      # non-dr 33; wgrad ndc 8: 5 x 6, 3 and one EMPTY chunk (zero slab)
    (512, 2, 4, "fwd", 1, 2, 2, 1),      # wgrad nper = 2: the image loop re-primes both rings
    (64, 16, 16, "dr", 1, 16, 1, 1),     # dr, one chunk of 16 (the production walk); wgrad 256 blocks
]
C32_LARGE = [(512, 2, 4), (64, 16, 16)]

# direct kernels (conv3d_direct_fwd / conv3d_direct_wgrad): (N, cin, cout, D, H, W), dtypes, ops
DIRECT_CASES = [
    ((2, 16, 16, 3, 5, 8), (F32, BF16), ("fwd", "dgrad", "wgrad")),     # odd H, several blocks
    ((1, 24, 16, 3, 4, 8), (F32, BF16), ("fwd", "dgrad", "wgrad")),     # cin != cout, cin no power of two
    ((1, 64, 8, 2, 3, 5), (F32, BF16), ("fwd", "dgrad", "wgrad")),      # the cin limit (acc[65] of the wgrad)
    ((1, 3, 8, 2, 4, 6), (F32, BF16), ("fwd", "wgrad")),                # cin = 3: no dgrad (cin % 8 != 0)
    ((2, 32, 32, 4, 4, 64), (F32,), ("fwd", "dgrad", "wgrad")),         # the fast shape in fp32: direct
    ((1, 32, 32, 2, 6, 64), (BF16,), ("fwd", "dgrad", "wgrad")),        # edge of c32_fast: H % 4 != 0
]
C32_EDGE = (1, 32, 32, 2, 6, 64)

# general-channel implicit GEMM (fv_conv3dg_*): name -> (N, cin, cout, D, H, W of the output, k, ups)
# Not covered: the 512 MB slab cap of wg_plan (no test-sized shape reaches it).
GEMM_CASES = {
    # the eight CASES of tests/test_mfe_gpu.py
    "80to64_k3": (2, 80, 64, 3, 4, 6, 3, False),            # cin no power of two; K straddles taps
    "24to40_border": (1, 24, 40, 2, 2, 2, 3, False),        # every voxel on the border; cout % 16 != 0
    "512to1024_deep": (1, 512, 1024, 2, 2, 2, 3, False),    # K = 13 824; 32 x 64 tiles, 8 voxels
    "16to8_ups": (2, 16, 8, 2, 4, 4, 3, True),              # upsample gather
    "112to16_k7": (1, 112, 16, 4, 8, 8, 7, False),          # 7 taps, D < ksize
    "32to4_k1": (1, 32, 4, 2, 3, 5, 1, False),              # cout < 8, 1 tap; dgrad element gather, 1 chunk
    "64to32_split": (3, 64, 32, 5, 6, 10, 3, False),        # several voxel tiles; voxel split in the wgrad
    "8to256_bigtile": (1, 8, 256, 2, 64, 64, 3, False),     # 64 x 128 tile plan, no ragged tile
    # new
    "16to6_k3": (2, 16, 6, 3, 5, 7, 3, False),              # cout % 4 != 0: scalar store; dgrad partial chunk
    "24to20_ups": (1, 24, 20, 2, 6, 10, 3, True),           # cout % 8 != 0 under ups; upsample_bwd, 3 octets
    "8to1_k7": (1, 8, 1, 3, 5, 6, 7, False),                # one output channel; most taps outside
    "72to72_k3": (1, 72, 72, 2, 3, 5, 3, False),            # 3 x 32-wide tiles, last 8 wide; wgrad nco = nci = 2 ragged
    "8to72_bigtile_ragged": (1, 8, 72, 3, 75, 73, 3, False),  # 64 x 128 plan; P % 128 = 41, cout % 64 = 8
    "8to8_k1_dbcap": (1, 8, 8, 3, 300, 300, 1, False),      # P = 270 000: db nparts cap 1024, dbper 264
}
MFE_CASE_NAMES = list(GEMM_CASES)[:8]


def c32_id(c):
    return f"n{c[0]}_d{c[1]}_h{c[2]}"


def direct_id(c):
    return "x".join(str(i) for i in c)


# ---------------------------------------------------------------------------- helpers
def _chunks(N, voxels_per_image, budget=1 << 17):
    """slices over N of at most `budget` voxels each (at least one image)"""
    step = max(1, budget // max(1, voxels_per_image))
    return [slice(i, min(N, i + step)) for i in range(0, N, step)]


def upsample(x):
    return F.interpolate(x, scale_factor=(1, 2, 2), mode="nearest")


def pool2_sum3(t):
    """sums over the 2 x 2 (h, w) quads: the backward of the nearest (1, 2, 2) upsample"""
    N, C, D, H, W = t.shape
    return t.view(N, C, D, H // 2, 2, W // 2, 2).sum((4, 6))


class ExactCase3:
    """Operands, conditions and float64 references of one 3-D conv case; every tensor is float64
    on the CPU, computed once on first use and never modified.  (D, H, W) is the OUTPUT volume;
    under ups the input is (D, H / 2, W / 2).  sr=True: a residual and / or statistics records
    are involved (the condition |conv + bias| + |res| <= 256 joins the thinning)."""

    def __init__(self, key, N, cin, cout, D, H, W, k=3, ups=False, sr=False, cap_log2=None):
        self.key, self.N, self.cin, self.cout, self.D, self.H, self.W = key, N, cin, cout, D, H, W
        self.k, self.ups, self.sr = k, ups, sr
        self.cap = float(2 ** (CAP_LOG2 if cap_log2 is None else cap_log2))
        g = _gen("exact3d", key, N, cin, cout, D, H, W, k, ups, sr)
        hi, wi = (H // 2, W // 2) if ups else (H, W)
        self.in_shape = (N, cin, D, hi, wi)
        self.out_shape = (N, cout, D, H, W)
        self.w_shape = (cout, cin, k, k, k)
        self.x = _ints(self.in_shape, -2, 2, g)
        self._w = _Ternary(self.w_shape, g)
        self.b = _ints((cout,), -3, 3, g)
        self.r = _ints(self.out_shape, -3, 3, g)
        self.gy_d = _ints(self.out_shape, -2, 2, g)
        self._gy_w = _Ternary(self.out_shape, g)
        self._sl = _chunks(N, D * H * W)
        self._fig = {}

    # -- sliced evaluation
    def _xi(self, x):
        return upsample(x) if self.ups else x

    def _fwd(self, x, w, b):
        return torch.cat([F.conv3d(self._xi(x[s]), w, b, 1, self.k // 2) for s in self._sl])

    def _abs_fwd(self, w):
        """max A of the forward, in fp32 (sums of non-negative integers: exact below 2^24, and a
        sum above that cannot round down past the cap)"""
        xa, wa, ba = self.x.abs().float(), w.abs().float(), self.b.abs().float()
        return max(F.conv3d(self._xi(xa[s]), wa, ba, 1, self.k // 2).max().item() for s in self._sl)

    def _abs_dgrad(self, w):
        """max A of the data gradient; under ups the pooled A (the four stored values are summed)"""
        m = 0.0
        wa = w.abs().float()
        for s in self._sl:
            a = F.conv_transpose3d(self.gy_d[s].abs().float(), wa, None, 1, self.k // 2)
            m = max(m, (pool2_sum3(a) if self.ups else a).max().item())
        return m

    def _try_w(self, z):
        w = self._w.at(z)
        if self._abs_fwd(w) > self.cap or self._abs_dgrad(w) > self.cap:
            return None
        y = self._fwd(self.x, w, self.b)
        if self.sr and (y.abs() + self.r.abs()).max().item() > 256:
            return None
        return z, w, y

    @functools.cached_property
    def _wy(self):
        z = ZERO_SHARE
        while True:
            got = self._try_w(z)
            if got is not None:
                return got
            z = 1 - (1 - z) * 0.75

    @property
    def w_zero_share(self):
        return self._wy[0]

    @property
    def w(self):
        return self._wy[1]

    @property
    def y(self):
        """conv + bias"""
        return self._wy[2]

    @functools.cached_property
    def conv(self):
        """the conv without its bias"""
        return self.y - self.b[None, :, None, None, None]

    @functools.cached_property
    def dx_conv(self):
        """data gradient at the conv's own resolution (the high one under ups), by autograd"""
        out = []
        for s in self._sl:
            xi = torch.zeros(self._xi(self.x[s]).shape, dtype=torch.float64, requires_grad=True)
            y = F.conv3d(xi, self.w, None, 1, self.k // 2)
            out.append(torch.autograd.grad(y, xi, self.gy_d[s])[0])
        return torch.cat(out)

    def dx_low(self, dtype):
        """what fv_conv3dg_upsample_bwd owes: the four STORED (rounded to dtype) high-resolution
        gradients summed, then rounded again by the comparator"""
        assert self.ups
        return pool2_sum3(self.dx_conv.to(dtype).double())

    def _wgrad(self, x, gy):
        dw = torch.zeros(self.w_shape, dtype=torch.float64)
        for s in self._sl:
            dw += torch.nn.grad.conv3d_weight(self._xi(x[s]), self.w_shape, gy[s], 1, self.k // 2).double()
        return dw

    def _wgrad_ok(self, gy):
        return (self._wgrad(self.x.abs().float(), gy.abs().float()).max().item() <= self.cap
                and gy.abs().sum((0, 2, 3, 4)).max().item() <= self.cap)

    @functools.cached_property
    def gy_w_zero_share(self):
        z = ZERO_SHARE
        while not self._wgrad_ok(self._gy_w.at(z)):
            z = 1 - (1 - z) * 0.75
        return z

    @functools.cached_property
    def gy_w(self):
        return self._gy_w.at(self.gy_w_zero_share)

    @functools.cached_property
    def dw_db(self):
        return self._wgrad(self.x, self.gy_w), self.gy_w.sum((0, 2, 3, 4))

    # -- conditions
    def check_conditions(self, ops=("fwd", "dgrad", "wgrad")):
        """Assert the conditions of the module docstring for the listed operations; returns the
        measured figures (cached per operation)."""
        cap = self.cap
        for op in ops:
            if op in self._fig:
                continue
            f = {}
            if op == "fwd":
                assert bool((self.w == torch.round(self.w)).all()) and bool((self.y == torch.round(self.y)).all())
                f["fwd_A"] = self._abs_fwd(self.w)
                f["fwd_prod"] = (self.x.abs().max() * self.w.abs().max()).item()
                f["fwd_max"] = self.y.abs().max().item()
                f["w_zero_share"] = self.w_zero_share
                assert f["fwd_A"] <= cap and f["fwd_prod"] <= 4.0, f
                if self.sr:
                    f["sr_max"] = (self.y.abs() + self.r.abs()).max().item()
                    assert f["sr_max"] <= 256, f
            elif op == "dgrad":
                f["dgrad_A"] = self._abs_dgrad(self.w)
                f["dgrad_prod"] = (self.gy_d.abs().max() * self.w.abs().max()).item()
                f["dgrad_max"] = self.dx_conv.abs().max().item()
                assert f["dgrad_A"] <= cap and f["dgrad_prod"] <= 4.0, f
            elif op == "wgrad":
                f["wgrad_A"] = self._wgrad(self.x.abs().float(), self.gy_w.abs().float()).max().item()
                f["bgrad_A"] = self.gy_w.abs().sum((0, 2, 3, 4)).max().item()
                f["wgrad_prod"] = (self.x.abs().max() * self.gy_w.abs().max()).item()
                f["gy_zero_share"] = self.gy_w_zero_share
                assert f["wgrad_A"] <= cap and f["bgrad_A"] <= cap and f["wgrad_prod"] <= 4.0, f
            else:
                raise ValueError(op)
            self._fig[op] = f
        out = {}
        for op in ops:
            out.update(self._fig[op])
        return out


@functools.lru_cache(maxsize=None)
def c32_case(N, D, H):
    return ExactCase3("c32", N, 32, 32, D, H, 64, sr=True)


@functools.lru_cache(maxsize=None)
def direct_case(shape):
    N, cin, cout, D, H, W = shape
    return ExactCase3("direct", N, cin, cout, D, H, W, sr=True)


@functools.lru_cache(maxsize=None)
def gemm_case(name):
    N, cin, cout, D, H, W, k, ups = GEMM_CASES[name]
    return ExactCase3(name, N, cin, cout, D, H, W, k=k, ups=ups)


def drop_tap(w, co, ci):
    """-> (w with the first non-zero (kd, kh, kw) tap of the pair (co, ci) cleared, that tap)"""
    t = tuple(int(i) for i in w[co, ci].nonzero()[0])
    w2 = w.clone()
    w2[(co, ci) + t] = 0
    return w2, t
