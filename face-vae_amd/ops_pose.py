"""torch.autograd.Functions of the head pose estimator (HPE_EDE, models.py:990-1037 of
Luh1124/face-vae) over the fv_stem7s2_* / fv_maxpool3s2_* / fv_subsample2_* / fv_bn2_add_relu_fwd /
fv_pose_* entries of libfacevae (csrc/pose.hip), built on the conv and batch-norm plumbing of
ops.py.  As there, no CPU fallback, activations NHWC in the storage dtype, parameters fp32.

  StemFn          pre_layers: 7x7 stride-2 conv on the NCHW image -> BN -> act [-> MaxPool2d(3, 2, 1)
                  fused as the pool's prologue: the full-resolution activation is never written]
  MaxPool3s2Fn    nn.MaxPool2d(3, 2, 1) on its own
  ConvBNFn        ConvBlock2D "CNA" 3x3 stride 2, and "CN" 1x1 stride 1 / 2 (conv -> BN, no act)
  BottleneckFn    ResBottleneck (modules.py:138-152) as one Function: the three conv -> BN stages,
                  the optional projection, and relu(BN(a) + BN(b)) in one pass
  PoseHeadFn      global mean, fc_yaw / fc_pitch / fc_roll / fc_t / fc_scale, softmax expectation
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from . import ops as O
from ._lib import call, ptr, query, stream

CL = torch.channels_last
F32 = torch.float32


def _even(h, w, what):
    if h % 2 or w % 2:
        raise ValueError(f"facevae_amd {what}: the input height and width must be even (got {h} x {w})")


def _nhwc(n, c, h, w, dtype, device):
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=CL)


# ----------------------------------------------------------------------------------------
# elementwise passes
# ----------------------------------------------------------------------------------------

def maxpool_forward(x, pro=None, slope=0.0):
    """x NHWC [N, C, H, W] -> (pooled [N, C, H/2, W/2], argmax uint8); pro = (scale, shift): the
    pooled value is act(x * scale + shift)."""
    N, C, H, W = x.shape
    y = _nhwc(N, C, H // 2, W // 2, x.dtype, x.device)
    am = O._empty(N * (H // 2) * (W // 2) * C, torch.uint8, x.device)
    sc, sh = pro if pro is not None else (None, None)
    call("fv_maxpool3s2_fwd", L.dtype_code(x.dtype), ptr(x), N, H, W, C, ptr(sc), ptr(sh), float(slope), ptr(y),
         ptr(am), stream())
    return y, am


def maxpool_backward(g, am, H, W):
    N, C = g.shape[:2]
    dx = _nhwc(N, C, H, W, g.dtype, g.device)
    call("fv_maxpool3s2_bwd", L.dtype_code(g.dtype), ptr(g), ptr(am), N, H, W, C, ptr(dx), stream())
    return dx


def subsample_forward(x):
    N, C, H, W = x.shape
    y = _nhwc(N, C, H // 2, W // 2, x.dtype, x.device)
    call("fv_subsample2_fwd", L.dtype_code(x.dtype), ptr(x), N, H, W, C, ptr(y), stream())
    return y


def subsample_backward(g, H, W):
    N, C = g.shape[:2]
    dx = _nhwc(N, C, H, W, g.dtype, g.device)
    call("fv_subsample2_bwd", L.dtype_code(g.dtype), ptr(g), N, H, W, C, ptr(dx), stream())
    return dx


def join_forward(ya, ra, yb, rb=None):
    """relu(ya * ra.scale + ra.shift + (yb * rb.scale + rb.shift if rb else yb))."""
    N, C, H, W = ya.shape
    out = torch.empty_like(ya)
    call("fv_bn2_add_relu_fwd", L.dtype_code(ya.dtype), ptr(ya), ptr(ra.scale), ptr(ra.shift), ptr(yb),
         ptr(rb.scale if rb is not None else None), ptr(rb.shift if rb is not None else None), N * H * W, C, ptr(out),
         stream())
    return out


def relu_backward(g, out):
    dx = torch.empty_like(out)
    call("fv_relu_bwd", L.dtype_code(out.dtype), ptr(g), ptr(out), out.numel(), ptr(dx), stream())
    return dx


def add2(a, b):
    out = torch.empty_like(a)
    call("fv_add2", L.dtype_code(a.dtype), ptr(a), ptr(b), a.numel(), ptr(out), stream())
    return out


# ----------------------------------------------------------------------------------------
# stem
# ----------------------------------------------------------------------------------------

class StemFn(torch.autograd.Function):
    """ConvBlock2D("CNA", 3, cout, 7, 2, 3) on the NCHW fp32 image, optionally with the following
    MaxPool2d(3, 2, 1) fused (fuse_pool): BN-apply + act run as the pool's prologue.  The image
    gets no gradient (it is data, trainer.py:272-273)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, blk, fuse_pool):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        dtype = O.storage(blk.compute_dtype())
        dc = L.dtype_code(dtype)
        conv, bn = blk.conv, blk.bn
        N, cin, H, W = x.shape
        if cin != 3:
            raise ValueError("facevae_amd stem: a 3-channel image is expected")
        _even(H, W, "stem (7x7 stride-2 conv)")
        Ho, Wo = H // 2, W // 2
        if fuse_pool:
            _even(Ho, Wo, "max pool after the stem")
        cout = conv.out_channels
        dev = x.device
        x32 = x.detach().float().contiguous()
        w = conv.weight_param()
        if w.dtype != F32 or not w.is_contiguous():
            raise RuntimeError("conv weights must be contiguous fp32")
        wk = O._empty(query("fv_stem7s2_wk_elems", cout), dtype, dev)
        call("fv_stem7s2_weight_prep", dc, ptr(w), cout, ptr(wk), stream())
        training = blk.training
        comm = blk.bn_comm()
        y = _nhwc(N, cout, Ho, Wo, dtype, dev)
        part = None
        if training:
            nb, bp = query("fv_stem7s2_stats_blocks", N, H, W), query("fv_stem7s2_stats_block_pixels")
            part = O._empty(nb * 2 * cout, F32, dev)
        call("fv_stem7s2_fwd", dc, ptr(x32), N, H, W, cout, ptr(wk), ptr(bias), ptr(y), ptr(part), stream())
        if training:
            r = O.bn_from_records(bn, part, nb, bp, N * Ho * Wo, cout, True, comm)
        else:
            r = O.bn_finalize(bn, None, 0, False)
        am = None
        if fuse_pool:
            z, am = maxpool_forward(y, (r.scale, r.shift), blk.slope)
        else:
            z = O.bn_act_forward(y, r, blk.slope, False, bn)
        ctx.blk, ctx.r, ctx.comm, ctx.am, ctx.geo = blk, r, comm, am, (N, H, W, cout)
        ctx.save_for_backward(x32, y)
        return z

    @staticmethod
    def backward(ctx, dz):
        x32, y = ctx.saved_tensors
        blk, r = ctx.blk, ctx.r
        N, H, W, cout = ctx.geo
        dz = O.grad_in(dz, y.dtype)
        if ctx.am is not None:
            dz = maxpool_backward(dz, ctx.am, H // 2, W // 2)     # gradient of the activation output
        dy, dg, dbt = O.bn_act_backward(dz, y, blk.bn, r, blk.slope, False, ctx.comm)
        ws = O._empty(query("fv_stem7s2_wgrad_ws_bytes", N, H, W, cout) // 4, F32, y.device)
        dw = torch.empty_like(blk.conv.weight_param())
        db = torch.empty(cout, dtype=F32, device=y.device)
        call("fv_stem7s2_bwd_weight", L.dtype_code(y.dtype), ptr(x32), ptr(dy), N, H, W, cout, ptr(dw), ptr(db),
             ptr(ws), stream())
        return None, dw, db, dg, dbt, None, None


class MaxPool3s2Fn(torch.autograd.Function):
    """nn.MaxPool2d(3, 2, 1) (even H, W; channels a multiple of 8)."""

    @staticmethod
    def forward(ctx, x, dtype):
        if not x.is_cuda:
            raise RuntimeError("facevae_amd ops run on the GPU only (HIP); got a CPU tensor")
        N, C, H, W = x.shape
        _even(H, W, "MaxPool2d(3, 2, 1)")
        if C % 8:
            raise NotImplementedError("facevae_amd MaxPool2d: the channel count must be a multiple of 8")
        xb = x if (x.dtype == dtype and O.nhwc_view(x)) else x.to(dtype).contiguous(memory_format=CL)
        y, am = maxpool_forward(xb)
        ctx.am, ctx.hw, ctx.xdtype = am, (H, W), x.dtype
        return y

    @staticmethod
    def backward(ctx, g):
        dxb = maxpool_backward(O.grad_in(g, g.dtype), ctx.am, *ctx.hw)
        return dxb.to(ctx.xdtype), None


# ----------------------------------------------------------------------------------------
# conv -> BN stages
# ----------------------------------------------------------------------------------------

class _Stage:
    """Per-forward state of one conv -> BN stage: cs (ConvState / S2ConvState), the conv input
    xin (after the subsample of a stride-2 1x1 conv), the conv output y (the BN input), the
    BNResult r, and the stage's input size."""
    __slots__ = ("conv", "bn", "cs", "xin", "y", "r", "kind", "in_hw")


def stage_forward(conv, bn, xb, cin_pad, stride, dtype, training, comm, need_wt):
    """conv (1x1 at stride 1 / 2, 3x3 at stride 1 / 2, padding k // 2) -> BN statistics.  xb NHWC
    with cin_pad channels.  The BN is not applied here: the caller applies (r.scale, r.shift)
    with its activation (bn_act_forward) or in the bottleneck join."""
    N, _, H, W = xb.shape
    k = conv.kernel_size
    cout = conv.out_channels
    dev = xb.device
    st = _Stage()
    st.conv, st.bn, st.in_hw = conv, bn, (H, W)
    if stride == 2:
        _even(H, W, f"stride-2 {k}x{k} conv")
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    y = _nhwc(N, cout, Ho, Wo, dtype, dev)
    d = O.desc(dtype, N, Ho, Wo, cin_pad, conv.in_channels, cout, cout, k)
    if k == 3 and stride == 2:
        st.kind = "s2"
        st.xin = xb
        st.cs = O.S2ConvState(conv, d, (H, W), dtype, dev, training, need_wt)
        O.conv_s2_forward(st.cs, xb, conv.bias, y)
        st.r = O.bn_from_tensor(bn, y, training, comm)
    else:
        st.kind = "sub" if stride == 2 else "s1"
        st.xin = subsample_forward(xb) if stride == 2 else xb
        st.cs = O.ConvState(conv, d, dtype, dev, training, need_wt)
        part = O.conv_forward(st.cs, st.xin, conv.bias, y=y, stats=training)
        st.r = O.bn_from_partials(bn, part, st.cs, True, comm) if training else O.bn_finalize(bn, None, 0, False)
    st.cs.release()
    st.y = y
    return st


def stage_backward(st, dout, slope, comm, need_dx=True):
    """dout: gradient of act(BN(y)) (slope 1: the identity activation) -> (dx at the stage's
    input resolution or None, dW, db, dgamma, dbeta)."""
    dy, dg, dbt = O.bn_act_backward(dout, st.y, st.bn, st.r, slope, False, comm)
    if st.kind == "s2":
        dx, dw, db = O.conv_s2_backward(st.cs, st.xin, dy, need_dx=need_dx)
    else:
        dx, dw, db = O.conv_backward(st.cs, st.xin, dy, st.y.shape[1], need_dx=need_dx)
        if st.kind == "sub" and dx is not None:
            dx = subsample_backward(dx, *st.in_hw)
    return dx, dw, db, dg, dbt


class ConvBNFn(torch.autograd.Function):
    """ConvBlock2D "CNA" with a 3x3 stride-2 conv, and "CN" (conv -> BN, no activation) with a
    1x1 conv at stride 1 or 2 (ResBottleneck's pieces, modules.py:143-147), on their own."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, blk):
        dtype = O.storage(blk.compute_dtype())
        xb, cin_pad = O.to_nhwc(x, dtype)
        comm = blk.bn_comm()
        st = stage_forward(blk.conv, blk.bn, xb, cin_pad, blk.stride, dtype, blk.training, comm,
                           ctx.needs_input_grad[0])
        z = O.bn_act_forward(st.y, st.r, blk.slope, False, blk.bn)
        ctx.st, ctx.comm, ctx.slope = st, comm, blk.slope
        ctx.save_for_backward(x)
        return z

    @staticmethod
    def backward(ctx, dz):
        x, = ctx.saved_tensors
        st = ctx.st
        dz = O.grad_in(dz, st.y.dtype)
        dxb, dw, db, dg, dbt = stage_backward(st, dz, ctx.slope, ctx.comm, ctx.needs_input_grad[0])
        dx = O.from_nhwc(dxb, x) if dxb is not None else None
        return dx, dw, db, dg, dbt, None


class BottleneckFn(torch.autograd.Function):
    """ResBottleneck: relu(down_sample(x) + layers(x)) with layers = CNA 1x1 -> CNA 3x3 (stride)
    -> CN 1x1 and down_sample = CN 1x1 (stride) or the identity.  params: the (weight, bias, gamma,
    beta) of layers.0, layers.1, layers.2 and, with a projection, of down_sample.  The two "CN"
    batch norms are applied inside the join (fv_bn2_add_relu_fwd), never materialised."""

    @staticmethod
    def forward(ctx, x, blk, *params):
        dtype = O.storage(blk.compute_dtype())
        xb, cin_pad = O.to_nhwc(x, dtype)
        training = blk.training
        comm = blk.bn_comm()
        need_dx = ctx.needs_input_grad[0]
        b0, b1, b2 = blk.layers[0], blk.layers[1], blk.layers[2]
        mid = b0.conv.out_channels
        s0 = stage_forward(b0.conv, b0.bn, xb, cin_pad, 1, dtype, training, comm, need_dx)
        z0 = O.bn_act_forward(s0.y, s0.r, b0.slope, False, b0.bn)
        s1 = stage_forward(b1.conv, b1.bn, z0, mid, blk.stride, dtype, training, comm, True)
        z1 = O.bn_act_forward(s1.y, s1.r, b1.slope, False, b1.bn)
        s2 = stage_forward(b2.conv, b2.bn, z1, mid, 1, dtype, training, comm, True)
        sd = None
        if blk.project:
            bd = blk.down_sample
            sd = stage_forward(bd.conv, bd.bn, xb, cin_pad, blk.stride, dtype, training, comm, need_dx)
            out = join_forward(s2.y, s2.r, sd.y, sd.r)
        else:
            out = join_forward(s2.y, s2.r, xb)
        ctx.blk, ctx.comm, ctx.stages = blk, comm, (s0, s1, s2, sd)
        ctx.save_for_backward(x, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out = ctx.saved_tensors
        blk, comm = ctx.blk, ctx.comm
        s0, s1, s2, sd = ctx.stages
        need_dx = ctx.needs_input_grad[0]
        b0, b1 = blk.layers[0], blk.layers[1]
        g = relu_backward(O.grad_in(dout, out.dtype), out)         # gradient of BN(a) + BN(b)
        dz1, dw2, db2, dg2, dbt2 = stage_backward(s2, g, 1.0, comm)
        dz0, dw1, db1, dg1, dbt1 = stage_backward(s1, dz1, b1.slope, comm)
        dxb, dw0, db0, dg0, dbt0 = stage_backward(s0, dz0, b0.slope, comm, need_dx)
        grads = [dw0, db0, dg0, dbt0, dw1, db1, dg1, dbt1, dw2, db2, dg2, dbt2]
        if sd is not None:
            dxs, dwd, dbd, dgd, dbtd = stage_backward(sd, g, 1.0, comm, need_dx)
            grads += [dwd, dbd, dgd, dbtd]
            if need_dx:
                dxb = add2(dxb, dxs)
        elif need_dx:
            dxb = add2(dxb, g)
        dx = O.from_nhwc(dxb, x) if need_dx else None
        return (dx, None) + tuple(grads)


# ----------------------------------------------------------------------------------------
# pose head
# ----------------------------------------------------------------------------------------

def _ptr5(ts):
    return (ctypes.c_void_p * 5)(*[t.data_ptr() for t in ts])


class PoseHeadFn(torch.autograd.Function):
    """models.py:1025-1036: mean over (H, W), the five Linear layers, softmax expectation of the
    three angle heads -> out [N, 7] fp32 = (yaw, pitch, roll, t0, t1, t2, scale)."""

    @staticmethod
    def forward(ctx, h, n_bins, dtype, *wb):
        ws_, bs_ = wb[0::2], wb[1::2]
        for t in wb:
            if t.dtype != F32 or not t.is_contiguous():
                raise RuntimeError("pose head: fc weights and biases must be contiguous fp32")
        hb, cp = O.to_nhwc(h, dtype)
        N, C, H, W = h.shape
        if cp != C:
            raise NotImplementedError("facevae_amd pose head: the feature channels must be 8 * a power of two")
        dev = h.device
        feat = torch.empty((N, C), dtype=F32, device=dev)
        call("fv_pose_pool_fwd", L.dtype_code(dtype), ptr(hb), N, H * W, C, ptr(feat), stream())
        out = torch.empty((N, 7), dtype=F32, device=dev)
        prob = torch.empty((N, 3, n_bins), dtype=F32, device=dev)
        call("fv_pose_head_fwd", ptr(feat), N, C, n_bins, _ptr5(ws_), _ptr5(bs_), ptr(out), ptr(prob), stream())
        ctx.n_bins, ctx.dtype, ctx.hw = n_bins, dtype, (H, W)
        ctx.save_for_backward(h, feat, prob, *ws_)
        return out

    @staticmethod
    def backward(ctx, g_out):
        h, feat, prob = ctx.saved_tensors[:3]
        ws_ = ctx.saved_tensors[3:]
        N, C = feat.shape
        H, W = ctx.hw
        dev = feat.device
        g = g_out.float().contiguous()
        dws = [torch.empty_like(w) for w in ws_]
        dbs = [torch.empty(w.shape[0], dtype=F32, device=dev) for w in ws_]
        dx = _nhwc(N, C, H, W, ctx.dtype, dev)
        ws = O._empty(query("fv_pose_head_ws_bytes", N, C, ctx.n_bins) // 4, F32, dev)
        call("fv_pose_head_bwd", L.dtype_code(ctx.dtype), ptr(g), ptr(feat), ptr(prob), N, H * W, C, ctx.n_bins,
             _ptr5(ws_), _ptr5(dws), _ptr5(dbs), ptr(dx), ptr(ws), stream())
        grads = []
        for dw, db in zip(dws, dbs):
            grads += [dw, db]
        return (O.from_nhwc(dx, h) if ctx.needs_input_grad[0] else None, None, None) + tuple(grads)
