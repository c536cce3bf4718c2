"""torch.autograd.Functions of the AFE 3-D trunk over libfacevae (fv_conv3d_*, fv_depth_split).
No CPU fallback: every compute call goes through `_lib.call`.

Reference semantics restated (file:line in Luh1124/face-vae):
  AFE.forward's x.view(N, C, D, H, W) of the mid_conv output (models.py:941-942),
  ResBlock3D = x + NAC(NAC(x)) with ConvBlock3D "NAC" = SyncBatchNorm -> ReLU -> Conv3d 3x3x3
  (modules.py:52-56, _ResBlock 116-126, ResBlock3D 133-135; _ConvBlock 8-42).

Layout: 5-D activations are NDHWC (torch.channels_last_3d) in the storage dtype of the
compute mode.  A depth slice is then an NHWC image, so the BN statistics / apply / backward
kernels of ops.py run unchanged on the [N, C, D*H, W] channels_last alias (`as4d`).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from . import ops
from ._lib import call, ptr, query, stream

CL3 = torch.channels_last_3d
F32 = torch.float32


def as4d(x5: torch.Tensor) -> torch.Tensor:
    """[N, C, D, H, W] NDHWC tensor -> the [N, C, D*H, W] NHWC alias of the same memory."""
    N, C, D, H, W = x5.shape
    return x5.as_strided((N, C, D * H, W), (C * D * H * W, 1, W * C, C))


def as5d(x4: torch.Tensor, D: int) -> torch.Tensor:
    N, C, DH, W = x4.shape
    H = DH // D
    return x4.as_strided((N, C, D, H, W), (C * DH * W, 1, H * W * C, W * C, C))


def to_ndhwc(x: torch.Tensor, dtype) -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
    if x.dtype == dtype and x.is_contiguous(memory_format=CL3):
        return x
    return x.to(dtype).contiguous(memory_format=CL3)


def desc3(dtype, n, d, h, w, cin, cout):
    return L.Conv3dDesc(L.dtype_code(dtype), n, d, h, w, cin, cout)


def _dkey(d):
    return (d.dtype, d.n, d.d, d.h, d.w, d.cin, d.cout)


class Conv3dState:
    """Per-forward prepared weights of one Conv3d (wk forward, wt data gradient): the ones a
    W3PrepBatch made for this forward when they match (shape and weight version), else one
    fv_conv3d_weight_prep of its own."""

    def __init__(self, conv, d, device, need_wt):
        w = conv.weight
        if w.dtype != F32 or not w.is_contiguous():
            raise RuntimeError("conv3d weights must be contiguous fp32")
        self.conv, self.d, self.w = conv, d, w
        pre = conv.__dict__.get("_c3prep")
        if pre is not None and pre[0] == _dkey(d) and pre[1] == w._version and pre[2] is w:
            self.wk, self.wt = pre[3], pre[4]
            return
        nbytes = query("fv_conv3d_wk_bytes", ctypes.byref(d))
        if nbytes == 0:
            raise RuntimeError(f"conv3d: unsupported shape cin={d.cin} cout={d.cout}")
        self.wk = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.wt = torch.empty(nbytes, dtype=torch.uint8, device=device) if need_wt else None
        call("fv_conv3d_weight_prep", ctypes.byref(d), ptr(w), ptr(self.wk), ptr(self.wt), stream())

    def release(self):
        self.wk = None


class W3PrepBatch:
    """fv_conv3d_weight_prep_multi: the forward and data-gradient weight layouts of every conv of
    a 3-D trunk in one launch per forward (the per-conv path launched 2 per conv: 24 per AFE
    step).  Buffers persist per shape (stable addresses for graph replay); each conv finds its
    pair through `_c3prep`, checked against the shape and the weight's version."""

    def __init__(self, convs):
        self.convs = list(convs)
        self.bufs = {}

    def prep(self, d, device):
        if not self.convs:
            return
        k = _dkey(d)
        if k not in self.bufs:
            nbytes = query("fv_conv3d_wk_bytes", ctypes.byref(d))
            if nbytes == 0:
                return
            self.bufs = {k: [(torch.empty(nbytes, dtype=torch.uint8, device=device),
                              torch.empty(nbytes, dtype=torch.uint8, device=device)) for _ in self.convs]}
        pairs = self.bufs[k]
        n = len(self.convs)
        ws = [c.weight for c in self.convs]
        if any(w.dtype != F32 or not w.is_contiguous() or not w.is_cuda for w in ws):
            return
        P = ctypes.c_void_p * n
        call("fv_conv3d_weight_prep_multi", ctypes.byref(d), n, P(*[w.data_ptr() for w in ws]),
             P(*[a.data_ptr() for a, _ in pairs]), P(*[b.data_ptr() for _, b in pairs]), stream())
        for c, w, (a, b) in zip(self.convs, ws, pairs):
            c.__dict__["_c3prep"] = (k, w._version, w, a, b)


def conv3d_forward(cs: Conv3dState, x, bias, res=None, stats=False):
    """-> (y NDHWC, BN records (part, nb, bp) or None when the shape has no fused partials)."""
    d = cs.d
    y = torch.empty((d.n, d.cout, d.d, d.h, d.w), dtype=x.dtype, device=x.device, memory_format=CL3)
    rec = None
    part = None
    if stats:
        nb = query("fv_conv3d_stats_blocks", ctypes.byref(d))
        if nb > 0:
            bp = query("fv_conv3d_stats_block_pixels", ctypes.byref(d))
            part = torch.empty(nb * 2 * d.cout, dtype=F32, device=x.device)
            rec = (part, nb, bp)
    call("fv_conv3d_fwd", ctypes.byref(d), ptr(x), ptr(cs.wk), ptr(bias), ptr(res), ptr(y), ptr(part), stream())
    if ops.CHECK is not None:
        ops.CHECK("fwd3", cs, x=x, bias=bias, res=res, y=y)
    return y, rec


def conv3d_backward(cs: Conv3dState, x, dy, need_dx=True):
    d = cs.d
    dev = dy.device
    dw = torch.empty_like(cs.w)
    db = torch.empty(d.cout, dtype=F32, device=dev)
    nws = query("fv_conv3d_wgrad_ws_bytes", ctypes.byref(d))
    ws = ops._empty(max(nws, 4) // 4, F32, dev)
    call("fv_conv3d_bwd_weight", ctypes.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(db), ptr(ws) if nws else None,
         stream())
    dx = None
    if need_dx:
        dx = torch.empty((d.n, d.cin, d.d, d.h, d.w), dtype=dy.dtype, device=dev, memory_format=CL3)
        call("fv_conv3d_bwd_data", ctypes.byref(d), ptr(dy), ptr(cs.wt), ptr(dx), stream())
    if ops.CHECK is not None:
        ops.CHECK("bwd3", cs, x=x, dy=dy, dw=dw, db=db, dx=dx)
    return dx, dw, db


def bn3d_stats(bn, x5, rec, training, comm):
    """BN statistics of a 5-D activation: from the producing conv's records when present,
    else one statistics pass over the tensor."""
    if not training:
        return ops.bn_finalize(bn, None, 0, False)
    N, C, D, H, W = x5.shape
    if rec is not None:
        part, nb, bp = rec
        return ops.bn_from_records(bn, part, nb, bp, N * D * H * W, C, True, comm)
    return ops.bn_from_tensor(bn, as4d(x5), True, comm)


class ResBlock3DFn(torch.autograd.Function):
    """ResBlock3D: x + NAC(NAC(x)), NAC = SyncBN -> ReLU -> Conv3d 3x3x3 (modules.py:116-135).
    The BN-apply+ReLU outputs are materialised once each; conv1's epilogue writes BN2's
    statistics records, conv2's epilogue adds the residual."""

    @staticmethod
    def forward(ctx, x, w1, b1, g1, be1, w2, b2, g2, be2, blk):
        dtype = ops.storage(blk.compute_dtype())
        xb = to_ndhwc(x, dtype)
        N, C, D, H, W = xb.shape
        training = blk.training
        comm = blk.bn_comm()
        c1, c2 = blk.conv1, blk.conv2
        r1 = bn3d_stats(blk.bn1, xb, None, training, comm)
        a1 = as5d(ops.bn_act_forward(as4d(xb), r1, 0.0, False, blk.bn1), D)
        d1 = desc3(dtype, N, D, H, W, C, c1.out_channels)
        cs1 = Conv3dState(c1, d1, x.device, True)
        t1, rec = conv3d_forward(cs1, a1, b1, stats=training)
        r2 = bn3d_stats(blk.bn2, t1, rec, training, comm)
        a2 = as5d(ops.bn_act_forward(as4d(t1), r2, 0.0, False, blk.bn2), D)
        d2 = desc3(dtype, N, D, H, W, c1.out_channels, c2.out_channels)
        cs2 = Conv3dState(c2, d2, x.device, True)
        out, _ = conv3d_forward(cs2, a2, b2, res=xb)
        cs1.release()
        cs2.release()
        ctx.blk, ctx.cs1, ctx.cs2, ctx.r1, ctx.r2, ctx.comm = blk, cs1, cs2, r1, r2, comm
        ctx.save_for_backward(x, xb, t1, a1, a2)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, xb, t1, a1, a2 = ctx.saved_tensors
        blk, cs1, cs2, r1, r2, comm = ctx.blk, ctx.cs1, ctx.cs2, ctx.r1, ctx.r2, ctx.comm
        D = xb.shape[2]
        dout = to_ndhwc(dout, xb.dtype)
        da2, dw2, db2 = conv3d_backward(cs2, a2, dout)
        dt1, dg2, dbe2 = ops.bn_act_backward(as4d(da2), as4d(t1), blk.bn2, r2, 0.0, False, comm)
        da1, dw1, db1 = conv3d_backward(cs1, a1, as5d(dt1, D))
        dxb, dg1, dbe1 = ops.bn_act_backward(as4d(da1), as4d(xb), blk.bn1, r1, 0.0, False, comm,
                                             addend=as4d(dout))
        dx = as5d(dxb, D)
        if dx.dtype != x.dtype:
            dx = dx.to(x.dtype)
        return dx, dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2, None


class DepthSplitFn(torch.autograd.Function):
    """h [N, C*D, H, W] -> h.view(N, C, D, H, W) (models.py:941-942) between the build's NHWC and
    NDHWC layouts (fv_depth_split); the backward is the inverse permutation."""

    @staticmethod
    def forward(ctx, h, C, D, dtype):
        hb, Cp = ops.to_nhwc(h, dtype)
        N, CD, H, W = h.shape
        if Cp != CD or CD != C * D:
            raise RuntimeError(f"depth split: channels {CD} != C*D = {C * D}")
        out = torch.empty((N, C, D, H, W), dtype=dtype, device=h.device, memory_format=CL3)
        call("fv_depth_split", L.dtype_code(dtype), ptr(hb), N, H * W, C, D, 0, ptr(out), stream())
        ctx.shape, ctx.dtype, ctx.hdtype = (N, C, D, H, W), dtype, h.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, D, H, W = ctx.shape
        gb = to_ndhwc(g, ctx.dtype)
        dh = torch.empty((N, C * D, H, W), dtype=ctx.dtype, device=g.device, memory_format=ops.CL)
        call("fv_depth_split", L.dtype_code(ctx.dtype), ptr(gb), N, H * W, C, D, 1, ptr(dh), stream())
        return dh.to(ctx.hdtype), None, None, None


class DepthMergeFn(torch.autograd.Function):
    """fs [N, C, D, H, W] -> fs.view(N, C*D, H, W) (models.py:1103) into the NHWC layout."""

    @staticmethod
    def forward(ctx, fs, dtype):
        fb = to_ndhwc(fs, dtype)
        N, C, D, H, W = fb.shape
        out = torch.empty((N, C * D, H, W), dtype=dtype, device=fs.device, memory_format=ops.CL)
        call("fv_depth_split", L.dtype_code(dtype), ptr(fb), N, H * W, C, D, 1, ptr(out), stream())
        ctx.shape, ctx.dtype, ctx.fdtype = (N, C, D, H, W), dtype, fs.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, D, H, W = ctx.shape
        # dense NHWC with exactly C*D channels (to_nhwc would pad a channel count that is no
        # power of two, e.g. the MFE's 112 * 16, which this permutation must not see)
        gb = ops.grad_in(g, ctx.dtype)
        dfs = torch.empty((N, C, D, H, W), dtype=ctx.dtype, device=g.device, memory_format=CL3)
        call("fv_depth_split", L.dtype_code(ctx.dtype), ptr(gb), N, H * W, C, D, 0, ptr(dfs), stream())
        return dfs.to(ctx.fdtype), None


def depth_split(h, C, D, mode):
    return DepthSplitFn.apply(h, C, D, ops.storage(mode))


def depth_merge(fs, mode):
    return DepthMergeFn.apply(fs, ops.storage(mode))


# ----------------------------------------------------------------------------------------
# general-channel 3-D convs of the MFE (conv3d_gemm.hip, fv_conv3dg_*)
# ----------------------------------------------------------------------------------------

def descg(dtype, n, d, h, w, cin, cout, ksize, ups=False):
    """Descriptor of a general 3-D conv; (d, h, w) is the OUTPUT volume (twice the input's h, w
    under `ups`)."""
    return L.Conv3dgDesc(L.dtype_code(dtype), n, d, h, w, cin, cout, ksize, int(bool(ups)))


class Conv3dgState:
    """Per-forward prepared weights of one general Conv3d: wk (forward) and wt (data gradient)."""

    def __init__(self, w, d, device, need_wt):
        if w.dtype != F32 or not w.is_contiguous():
            raise RuntimeError("conv3d weights must be contiguous fp32")
        call("fv_conv3dg_check", ctypes.byref(d))          # raises FaceVAELibError when unsupported
        self.d, self.w = d, w
        self.wk = torch.empty(query("fv_conv3dg_wk_bytes", ctypes.byref(d)), dtype=torch.uint8, device=device)
        self.wt = None
        if need_wt:
            self.wt = torch.empty(query("fv_conv3dg_wt_bytes", ctypes.byref(d)), dtype=torch.uint8, device=device)
        call("fv_conv3dg_weight_prep", ctypes.byref(d), ptr(w), ptr(self.wk), ptr(self.wt), stream())

    def release(self):
        self.wk = None


def _tdtype(d):
    return torch.bfloat16 if d.dtype == L.FV_BF16 else F32


def conv3dg_forward(cs: Conv3dgState, x, bias):
    """x NDHWC [n, cin, d, h(/2), w(/2)] -> y NDHWC [n, cout, d, h, w]."""
    d = cs.d
    hin, win = (d.h // 2, d.w // 2) if d.upsample else (d.h, d.w)
    if tuple(x.shape) != (d.n, d.cin, d.d, hin, win) or x.dtype != _tdtype(d) or not x.is_contiguous(memory_format=CL3):
        raise RuntimeError(f"conv3dg: input {tuple(x.shape)} {x.dtype} does not match its descriptor")
    y = torch.empty((d.n, d.cout, d.d, d.h, d.w), dtype=x.dtype, device=x.device, memory_format=CL3)
    call("fv_conv3dg_fwd", ctypes.byref(d), ptr(x), ptr(cs.wk), ptr(bias), ptr(y), stream())
    if ops.CHECK is not None:
        ops.CHECK("fwdg", cs, x=x, bias=bias, y=y)
    return y


def conv3dg_backward(cs: Conv3dgState, x, dy, need_dx=True, need_db=True):
    """-> (dx NDHWC like x or None, dw fp32 in the parameter layout, db fp32 or None)."""
    d = cs.d
    dev = dy.device
    if tuple(dy.shape) != (d.n, d.cout, d.d, d.h, d.w) or dy.dtype != x.dtype or not dy.is_contiguous(memory_format=CL3):
        raise RuntimeError(f"conv3dg: gradient {tuple(dy.shape)} {dy.dtype} does not match its descriptor")
    dw = torch.empty_like(cs.w)
    db = torch.empty(d.cout, dtype=F32, device=dev) if need_db else None
    ws = ops._empty(query("fv_conv3dg_wgrad_ws_bytes", ctypes.byref(d)), torch.uint8, dev)
    call("fv_conv3dg_bwd_weight", ctypes.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(db), ptr(ws), stream())
    dx = None
    if need_dx:
        dx = torch.empty((d.n, d.cin, d.d, d.h, d.w), dtype=dy.dtype, device=dev, memory_format=CL3)
        call("fv_conv3dg_bwd_data", ctypes.byref(d), ptr(dy), ptr(cs.wt), ptr(dx), stream())
        if d.upsample:
            lo = torch.empty((d.n, d.cin, d.d, d.h // 2, d.w // 2), dtype=dy.dtype, device=dev, memory_format=CL3)
            call("fv_conv3dg_upsample_bwd", ctypes.byref(d), ptr(dx), ptr(lo), stream())
            dx = lo
    if ops.CHECK is not None:
        ops.CHECK("bwdg", cs, x=x, dy=dy, dw=dw, db=db, dx=dx)
    return dx, dw, db


class Conv3dFn(torch.autograd.Function):
    """Bare nn.Conv3d(cin, cout, k, 1, k // 2) with bias (MFE.compress, MFE.mask_conv:
    models.py:1054, 1057): y NDHWC in the storage dtype."""

    @staticmethod
    def forward(ctx, x, weight, bias, ksize, dtype):
        xb = to_ndhwc(x, dtype)
        N, C, D, H, W = xb.shape
        d = descg(dtype, N, D, H, W, C, weight.shape[0], ksize)
        cs = Conv3dgState(weight, d, x.device, ctx.needs_input_grad[0])
        y = conv3dg_forward(cs, xb, bias)
        cs.release()
        ctx.cs = cs
        ctx.save_for_backward(x, xb)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, xb = ctx.saved_tensors
        dx, dw, db = conv3dg_backward(ctx.cs, xb, to_ndhwc(dy, xb.dtype), ctx.needs_input_grad[0],
                                      ctx.needs_input_grad[2])
        if dx is not None and dx.dtype != x.dtype:
            dx = dx.to(x.dtype)
        return dx, dw, db, None, None


class _PaddedBN:
    """BN holder padded to `cp` channels (gamma 1, beta 0, mean 0, var 1 in the pad) for the BN
    kernels, which take 8 * 2^k channels; the padded conv channels are all zero, stay zero
    through BN + ReLU, and are cut off again.  Only channel counts that are not 8 * 2^k (none
    in the default MFE) come this way."""

    def __init__(self, bn, gamma, beta, cp):
        c = bn.num_features
        dev = gamma.device
        one, zero = torch.ones(cp - c, device=dev), torch.zeros(cp - c, device=dev)
        self.bn, self.num_features, self.eps, self.momentum = bn, cp, bn.eps, bn.momentum
        self.track_running_stats = bn.track_running_stats
        self.weight = torch.cat([gamma.detach(), one])
        self.bias = torch.cat([beta.detach(), zero])
        self.running_mean = torch.cat([bn.running_mean, zero])
        self.running_var = torch.cat([bn.running_var, one])
        self.num_batches_tracked = bn.num_batches_tracked

    def write_back(self):
        c = self.bn.num_features
        self.bn.running_mean.copy_(self.running_mean[:c])
        self.bn.running_var.copy_(self.running_var[:c])


def _pad_rows(t, cp):
    return torch.cat([t.detach(), t.new_zeros((cp - t.shape[0],) + tuple(t.shape[1:]))]).contiguous()


class CNA3DFn(torch.autograd.Function):
    """ConvBlock3D "CNA": Conv3d -> SyncBatchNorm -> ReLU (modules.py:8-42, 52-56), with
    DownBlock3D's AvgPool3d((1, 2, 2)) fused into the BN/ReLU pass (blk.pool) or UpBlock3D's
    nearest (1, 2, 2) upsample folded into the conv's gather (blk.upsample) (modules.py:59-94).
    In NDHWC the [N, C, D*H, W] alias turns both into their 2-D 2x2 forms (row d*H + h <-> rows
    2(d*H + h), +1 as H is even), so the BN kernels of ops.py run unchanged."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, blk):
        dtype = ops.storage(blk.compute_dtype())
        xb = to_ndhwc(x, dtype)
        N, Cin, D, Hi, Wi = xb.shape
        H, W = (2 * Hi, 2 * Wi) if blk.upsample else (Hi, Wi)
        conv, bn = blk.conv, blk.bn
        cout = conv.out_channels
        cp = ops.pad_pow2(cout)
        training = blk.training
        comm = blk.bn_comm()
        pbn = bn
        cin_w = weight.shape[1]
        cut_in = Cin == cin_w and Cin % 8 != 0
        if cut_in:
            # a channel count the conv kernels do not take (SameBlock3D(30, 15) on its own): pad on entry
            xb = pad_channels(xb, ops.pad_pow2(Cin))
            Cin = xb.shape[1]
        if Cin != cin_w:
            # the input carries zero pad channels (EFE_conv5.mix runs at pad_pow2(2K) channels): the
            # weight gets zero columns for them
            if Cin != ops.pad_pow2(cin_w):
                raise RuntimeError(f"ConvBlock3D: input with {Cin} channels for a conv of {cin_w} "
                                   f"({cin_w}, or {ops.pad_pow2(cin_w)} with a zero pad)")
            wp = weight.new_zeros((cout, Cin) + tuple(weight.shape[2:]))
            wp[:, :cin_w] = weight.detach()
            weight = wp
        if cp != cout:
            weight, bias, pbn = _pad_rows(weight, cp), _pad_rows(bias, cp), _PaddedBN(bn, gamma, beta, cp)
        d = descg(dtype, N, D, H, W, Cin, cp, conv.kernel_size, blk.upsample)
        cs = Conv3dgState(weight, d, x.device, ctx.needs_input_grad[0])
        y = conv3dg_forward(cs, xb, bias)
        r = ops.bn_from_tensor(pbn, as4d(y), training, comm)
        if training and pbn is not bn:
            pbn.write_back()
        z = as5d(ops.bn_act_forward(as4d(y), r, 0.0, blk.pool, pbn), D)
        if cp != cout:
            z = z[:, :cout].contiguous(memory_format=CL3)
        cs.release()
        ctx.blk, ctx.cs, ctx.r, ctx.comm, ctx.pbn, ctx.cout = blk, cs, r, comm, pbn, cout
        ctx.cin_w, ctx.cut_in = cin_w, cut_in
        ctx.save_for_backward(x, xb, y)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, xb, y = ctx.saved_tensors
        blk, cs, r, cout = ctx.blk, ctx.cs, ctx.r, ctx.cout
        D = y.shape[2]
        cp = y.shape[1]
        dz = to_ndhwc(dz, y.dtype)
        if cp != cout:
            full = torch.zeros((dz.shape[0], cp) + tuple(dz.shape[2:]), dtype=dz.dtype, device=dz.device).contiguous(
                memory_format=CL3)
            full[:, :cout] = dz
            dz = full
        dy, dg, dbt = ops.bn_act_backward(as4d(dz), as4d(y), ctx.pbn, r, 0.0, blk.pool, ctx.comm)
        dx, dw, db = conv3dg_backward(cs, xb, as5d(dy, D), ctx.needs_input_grad[0])
        if dx is not None and ctx.cut_in:
            dx = dx[:, :ctx.cin_w].contiguous(memory_format=CL3)
        if dx is not None and dx.dtype != x.dtype:
            dx = dx.to(x.dtype)
        if dw.shape[1] != ctx.cin_w:
            dw = dw[:, :ctx.cin_w].contiguous()
        return dx, dw[:cout], db[:cout], dg[:cout], dbt[:cout], None


class _PaddedConv3:
    """Conv3d holder whose [C][C][3][3][3] weight and [C] bias are zero-padded to cp channels both
    ways for this forward (what Conv3dState reads of a conv: `weight`, `out_channels`)."""

    def __init__(self, weight, bias, cp):
        c = weight.shape[0]
        w = weight.new_zeros((cp, cp) + tuple(weight.shape[2:]))
        w[:c, :c] = weight.detach()
        self.weight, self.bias = w, _pad_rows(bias, cp)
        self.in_channels = self.out_channels = cp


class _PadState:
    """The cp-channel images of a padded ResBlock3D's parameters and batch-norm buffers, kept per
    block and device: the pad (zero weights and biases; gamma 1, beta 0, mean 0, var 1) is written
    once, and a forward copies only the live [:C] parts in -- two strided copies for the conv weights
    and one multi-tensor copy for the ten vectors -- instead of re-building every image with
    zeros / cat (24 small launches per block and forward)."""

    def __init__(self, blk, cp, device):
        self.C, self.cp, self.device = blk.bn1.num_features, cp, device
        self.convs = [_PaddedConv3(c.weight, c.bias, cp) for c in (blk.conv1, blk.conv2)]
        self.bns = [_PaddedBN(bn, bn.weight, bn.bias, cp) for bn in (blk.bn1, blk.bn2)]

    @staticmethod
    def of(blk, cp, device):
        st = blk.__dict__.get("_padstate")
        if st is None or st.cp != cp or st.device != device:
            st = _PadState(blk, cp, device)
            blk.__dict__["_padstate"] = st
        return st

    def refresh(self, w1, b1, g1, be1, w2, b2, g2, be2):
        C = self.C
        with torch.no_grad():
            self.convs[0].weight[:C, :C].copy_(w1)
            self.convs[1].weight[:C, :C].copy_(w2)
            dst, src = [self.convs[0].bias[:C], self.convs[1].bias[:C]], [b1, b2]
            for pbn, g, be in ((self.bns[0], g1, be1), (self.bns[1], g2, be2)):
                pbn.num_batches_tracked = pbn.bn.num_batches_tracked
                dst += [pbn.weight[:C], pbn.bias[:C], pbn.running_mean[:C], pbn.running_var[:C]]
                src += [g, be, pbn.bn.running_mean, pbn.bn.running_var]
            torch._foreach_copy_(dst, [t.detach() for t in src])
        return self.convs[0], self.convs[1], self.bns[0], self.bns[1]

    def write_back(self):
        C = self.C
        with torch.no_grad():
            torch._foreach_copy_([t for p in self.bns for t in (p.bn.running_mean, p.bn.running_var)],
                                 [t[:C] for p in self.bns for t in (p.running_mean, p.running_var)])


def pad_channels(x5, cp):
    """NDHWC [N, C, D, H, W] -> NDHWC [N, cp, D, H, W] with zeros in channels [C, cp)."""
    N, C, D, H, W = x5.shape
    out = torch.empty((N, cp, D, H, W), dtype=x5.dtype, device=x5.device, memory_format=CL3).zero_()
    out[:, :C] = x5
    return out


class ResBlock3DPadFn(torch.autograd.Function):
    """ResBlock3D(C) for a C that is not 8 * 2^k, run at cp = pad_pow2(C) channels on the kernels of
    ResBlock3DFn: weights and biases zero-padded per forward (_PaddedConv3), the two batch norms
    through _PaddedBN, both kept in the block's _PadState.  The pad channels are zero on entry and stay exactly zero: batch norm maps 0
    to 0 there (mean 0, shift 0), ReLU keeps it, the padded weight rows and biases are zero and so
    is the residual.  x with C channels is padded on entry and the output cut on exit; x with cp
    channels (pad zero: fv_efe_kpcat_fwd's output, or the previous block's) stays at cp channels,
    with no copy either way, and so does its gradient."""

    @staticmethod
    def forward(ctx, x, w1, b1, g1, be1, w2, b2, g2, be2, blk):
        dtype = ops.storage(blk.compute_dtype())
        C = blk.bn1.num_features
        cp = ops.pad_pow2(C)
        if x.shape[1] not in (C, cp):
            raise RuntimeError(f"ResBlock3D({C}): input with {x.shape[1]} channels ({C}, or {cp} with a zero pad)")
        cut = x.shape[1] == C
        xb = to_ndhwc(x, dtype)
        if cut:
            xb = pad_channels(xb, cp)
        N, _, D, H, W = xb.shape
        training = blk.training
        comm = blk.bn_comm()
        ps = _PadState.of(blk, cp, x.device)
        c1, c2, bn1, bn2 = ps.refresh(w1, b1, g1, be1, w2, b2, g2, be2)
        d = desc3(dtype, N, D, H, W, cp, cp)
        r1 = bn3d_stats(bn1, xb, None, training, comm)
        a1 = as5d(ops.bn_act_forward(as4d(xb), r1, 0.0, False, bn1), D)
        cs1 = Conv3dState(c1, d, x.device, True)
        t1, rec = conv3d_forward(cs1, a1, c1.bias, stats=training)
        r2 = bn3d_stats(bn2, t1, rec, training, comm)
        a2 = as5d(ops.bn_act_forward(as4d(t1), r2, 0.0, False, bn2), D)
        cs2 = Conv3dState(c2, d, x.device, True)
        out, _ = conv3d_forward(cs2, a2, c2.bias, res=xb)
        if training:
            ps.write_back()
        cs1.release()
        cs2.release()
        ctx.cs1, ctx.cs2, ctx.r1, ctx.r2, ctx.comm, ctx.bn1, ctx.bn2 = cs1, cs2, r1, r2, comm, bn1, bn2
        ctx.C, ctx.cut, ctx.xdtype = C, cut, x.dtype
        ctx.save_for_backward(xb, t1, a1, a2)
        return out[:, :C].contiguous(memory_format=CL3) if cut else out

    @staticmethod
    def backward(ctx, dout):
        xb, t1, a1, a2 = ctx.saved_tensors
        cs1, cs2, r1, r2, comm, C = ctx.cs1, ctx.cs2, ctx.r1, ctx.r2, ctx.comm, ctx.C
        D = xb.shape[2]
        dout = to_ndhwc(dout, xb.dtype)
        if ctx.cut:
            dout = pad_channels(dout, xb.shape[1])
        da2, dw2, db2 = conv3d_backward(cs2, a2, dout)
        dt1, dg2, dbe2 = ops.bn_act_backward(as4d(da2), as4d(t1), ctx.bn2, r2, 0.0, False, comm)
        da1, dw1, db1 = conv3d_backward(cs1, a1, as5d(dt1, D))
        dxb, dg1, dbe1 = ops.bn_act_backward(as4d(da1), as4d(xb), ctx.bn1, r1, 0.0, False, comm,
                                             addend=as4d(dout))
        dx = as5d(dxb, D)
        if ctx.cut:
            dx = dx[:, :C].contiguous(memory_format=CL3)
        if dx.dtype != ctx.xdtype:
            dx = dx.to(ctx.xdtype)
        return (dx, dw1[:C, :C].contiguous(), db1[:C], dg1[:C], dbe1[:C], dw2[:C, :C].contiguous(), db2[:C], dg2[:C],
                dbe2[:C], None)
