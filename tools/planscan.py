"""Every public geometry query of the 2-D conv over a sweep of descriptors (CPU only; no launch).

    python tools/planscan.py [--out DUMP] [--kernels]

One line per descriptor: its fields, then fv_conv_wk_elems, fv_conv_wt_elems,
fv_conv2d_stats_block_pixels, fv_conv2d_stats_blocks, fv_conv2d_sr_records with its pixels for
dgrad 0 and 1, fv_conv2d_dgrad_lowres, fv_conv_weight_prep_batchable, fv_conv2d_wgrad_nsplit,
fv_conv2d_wgrad_slab_elems and fv_conv2d_wgrad_bias_slab_elems, or "rejected" where check_desc
refuses it.  --kernels appends a last column: fv_conv2d_fwd_kernel for the forward (plain / with a
residual / with statistics) and the data gradient, so that the other columns of two builds can be
compared byte for byte (FV_LIB_PATH selects the build; one that lacks the entry prints "-").

The lines go to --out (tens of MB for the whole sweep); stdout gets a digest: per (dtype, ksize)
group the line count and the SHA-256 of its lines, then the totals.  A planner refactor keeps every
digest; profiles/conv_plan/ holds those of the FwdPlan change for the default switches,
FV_DISABLE_SUBPIX=1 and FV_C1S=0.
"""
import argparse
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fvamd  # noqa: E402,F401
from facevae_amd import _lib as L  # noqa: E402

CHANNELS = (8, 16, 32, 64, 128, 256, 512)
COUTS = (3, 4, 8, 16, 24, 32, 64, 128, 256, 512)
# (N, H, W) of the output: the benchmark's configs (256^2 B = 32 / 64, 512^2 B = 8: the full, half
# and quarter resolutions of the model) ...
SHAPES = [(n, r, r) for n, res in ((32, 256), (64, 256), (8, 512)) for r in (res, res // 2, res // 4)]
# ... the shapes of the test tables (tests/exact_operands.py, test_kernels_gpu.py, test_epilogue_gpu.py) at their N ...
_T = [(12, 10), (16, 16), (8, 8), (16, 12), (7, 9), (12, 20), (20, 12), (9, 13), (6, 10), (8, 64), (16, 64), (8, 16), (8, 128),
      (20, 64), (64, 128), (4, 64), (12, 128), (32, 32), (32, 64), (16, 128), (64, 256), (256, 256), (128, 128)]
SHAPES += [(2, h, w) for h, w in _T] + [(1, 8, 64), (1, 12, 10), (1, 32, 32), (3, 8, 64), (3, 12, 20), (3, 20, 64)]
# ... and N = 1, 3 and 64 at a model resolution
SHAPES += [(1, 64, 64), (3, 64, 64), (64, 32, 32), (1, 256, 256), (3, 128, 128)]


def pad_pow2(c):
    p = 8
    while p < c:
        p *= 2
    return p


def descriptors():
    for dtype in (L.FV_F32, L.FV_BF16):
        for ks in (1, 3, 7):
            for ups, pro in ((0, 0), (0, 1), (1, 0), (1, 1)):
                for cin in CHANNELS:
                    for cv in (cin, 3):
                        for cout in COUTS:
                            # the channel strides with a plain epilogue, the epilogue switches at ldy = cout
                            for ldy, sig, nchw in ((cout, 0, 0), (pad_pow2(cout), 0, 0), (2 * cout, 0, 0), (cout, 1, 0),
                                                   (cout, 0, 1), (cout, 1, 1)):
                                for n, h, w in SHAPES:
                                    yield L.ConvDesc(dtype, n, h, w, cin, cv, cout, ldy, ks, ups, pro, 0.2, sig, nchw)


FIELDS = ("dtype", "n", "h", "w", "cin", "cin_valid", "cout", "ldy", "ksize", "upsample", "pro_act", "epi_sigmoid",
          "out_nchw_f32")


def line(d, lib, kernels):
    r = ctypes.byref(d)
    head = " ".join(str(getattr(d, f)) for f in FIELDS)
    if lib.fv_conv2d_stats_block_pixels(r) == 0:
        return head + " | rejected"
    bp0, bp1 = ctypes.c_int(0), ctypes.c_int(0)
    sr0 = lib.fv_conv2d_sr_records(r, 0, ctypes.byref(bp0))
    sr1 = lib.fv_conv2d_sr_records(r, 1, ctypes.byref(bp1))
    cols = (lib.fv_conv_wk_elems(r), lib.fv_conv_wt_elems(r), lib.fv_conv2d_stats_block_pixels(r),
            lib.fv_conv2d_stats_blocks(r), sr0, bp0.value, sr1, bp1.value, lib.fv_conv2d_dgrad_lowres(r),
            lib.fv_conv_weight_prep_batchable(r), lib.fv_conv2d_wgrad_nsplit(r), lib.fv_conv2d_wgrad_slab_elems(r),
            lib.fv_conv2d_wgrad_bias_slab_elems(r))
    s = head + " | " + " ".join(str(c) for c in cols)
    if kernels:
        q = getattr(lib, "fv_conv2d_fwd_kernel", None)
        if q is None or q.argtypes is None:
            s += " | -"
        else:
            s += " | " + " ".join(L.CONV_KERNELS[q(r, *a)] for a in ((0, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 0, 0)))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write every line to this file")
    ap.add_argument("--kernels", action="store_true", help="append the fv_conv2d_fwd_kernel column")
    a = ap.parse_args()
    lib = L.load()
    out = open(a.out, "w") if a.out else None
    groups, total, n, rejected = {}, hashlib.sha256(), 0, 0
    for d in descriptors():
        s = line(d, lib, a.kernels) + "\n"
        if out:
            out.write(s)
        g = groups.setdefault((d.dtype, d.ksize), [0, hashlib.sha256()])
        g[0] += 1
        g[1].update(s.encode())
        total.update(s.encode())
        n += 1
        rejected += s.endswith("rejected\n")
    for (dtype, ks), (cnt, h) in sorted(groups.items()):
        print(f"dtype {dtype} ksize {ks}: {cnt} descriptors, sha256 {h.hexdigest()}")
    print(f"total: {n} descriptors ({rejected} rejected), sha256 {total.hexdigest()}")


if __name__ == "__main__":
    main()
