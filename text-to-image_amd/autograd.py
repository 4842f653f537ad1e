"""torch.autograd.Functions whose forward AND backward are libt2i_hip.so kernels.

The critic's gradient penalty (reference models/wgancls/model.py:62-70) differentiates through a gradient, so every
Function on the critic path has a backward that is itself composed of Functions (conv <-> conv^T <-> filter-gradient
form a closed family: the double backward needs no new kernel type; layer norm, pixel norm and the minibatch standard deviation
carry a double-backward kernel of their own).  Generator-only ops (batch norm, tanh, slope norm) are first-order (``once_differentiable``), exactly what the
reference's two optimizers need.

``input_grads_only()`` marks the first-order pass of the gradient penalty (tf.gradients(y, [x]) at model.py:63,68):
there only d/d(input) is wanted, so filter / bias gradients are not launched.
"""
import contextlib
import weakref

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import kernels as K

_INPUTS_ONLY = [False]

# Gradient sinks: weight storage address -> view of the optimizer's gradient arena.  In the final (first-order) backward
# a filter gradient whose weight has a sink is ACCUMULATED by the GEMM epilogue straight into the arena and autograd gets
# `None` for it: no temporary dw tensor, no separate `grad += dw` pass (0.55 ms/iteration of elementwise adds before).
# Registered by optim.Arena.enable_sinks().  NOTIFY[0], if set (dp.DataParallel), is called with the parameter's address
# after each contribution has been issued: sunk gradients never reach AccumulateGrad, so the data-parallel bucket
# overlap counts these notifications instead of post-accumulate hooks.
SINKS = {}          # address -> (weakref to the parameter leaf, its slot of the gradient arena as a flat view)
NOTIFY = [None]


def register_sink(param, slot, first_touch=None):
    """first_touch: callable() -> bool (optim.Arena): True exactly once per step for a slot whose first contribution may be a plain store."""
    SINKS[param.data_ptr()] = (weakref.ref(param), slot, first_touch)


def sink_accumulate(ptr):
    """Must the contribution about to be written into the sink of the parameter at `ptr` be ADDED to what the slot holds?  False exactly for
    the first contribution of a step into a slot the arena does not zero (optim.Arena.zero_grad): that one is written as a plain store."""
    e = SINKS.get(ptr)
    if e is None or e[2] is None:
        return True
    return not e[2]()


def sink_at(ptr):
    """The arena slot registered for the parameter stored at `ptr`, or None.  An entry whose parameter has been freed is
    dropped: the allocator may hand its address to an unrelated tensor (a stale entry would swallow that tensor's
    gradient into a dead arena)."""
    e = SINKS.get(ptr)
    if e is None:
        return None
    if e[0]() is None:
        del SINKS[ptr]
        return None
    return e[1]


def _notify(t):
    cb = NOTIFY[0]
    if cb is not None and t is not None:
        cb(t.data_ptr())


def _sink_of(t):
    """The gradient-arena slot of parameter `t` if sinks are on and this is the final (first-order) backward."""
    if t is None or torch.is_grad_enabled():
        return None
    return sink_at(t.data_ptr())


class _Side:
    """Filter-gradient stream.  A sunk filter gradient feeds nothing but the optimizer, so it is off the backward's
    critical path (which is the bwd-data chain): launched on a second HIP stream it runs CONCURRENTLY with the next
    layers' bwd-data kernels and fills their tail waves (and vice versa).  All sunk filter gradients share this one
    stream, so accumulations into a slot keep their program order and the sums stay bit-identical to the one-stream
    schedule.  Inputs are kept alive until side_join() because the caching allocator only orders reuse on one stream."""
    stream = None
    keep = []


SIDE = _Side()


def enable_side_stream(on=True):
    SIDE.stream = torch.cuda.Stream() if on else None
    SIDE.keep = []


def side_join():
    """Make the current stream wait for every filter gradient issued so far (call before the optimizer reads the arena)."""
    if SIDE.stream is not None:
        torch.cuda.current_stream().wait_stream(SIDE.stream)
        SIDE.keep.clear()


def sunk_launch(launch, keep):
    """Run `launch()` — a sunk filter gradient: it feeds nothing but the optimizer — on the filter-gradient stream if there is one
    (see _Side), else on the current stream.  keep: the tensors it reads, held until side_join()."""
    if SIDE.stream is not None:
        SIDE.stream.wait_stream(torch.cuda.current_stream())      # its operands and the zeroed arena are ready
        K.WS_LANE[0] = 1                                          # its own split-K workspace
        try:
            with torch.cuda.stream(SIDE.stream):
                launch()
        finally:
            K.WS_LANE[0] = 0
        SIDE.keep.append(keep)
    else:
        launch()


def _filter_grad(x, gpre, geom, w, xform=None, xform_plane_rows=0):
    """dw for weight `w`: into its sink if it has one and this is the final backward, else as a differentiable Function.
    xform: the Winograd input transform of `x` the forward conv left behind (kernels.LAST_XFORM), or None; xform_plane_rows: that
    transform belongs to a larger, stacked batch of this many images whose leading images are `x` (stacked.py)."""
    if not torch.is_grad_enabled():
        sink = sink_at(w.data_ptr())
        if sink is not None:
            xs, gs = _c(x), _c(gpre)
            acc = sink_accumulate(w.data_ptr())
            if xs is not x:
                xform = None
            if SIDE.stream is not None:
                SIDE.stream.wait_stream(torch.cuda.current_stream())      # x, gpre and the zeroed arena are ready
                K.WS_LANE[0] = 1                                          # its own split-K workspace
                try:
                    with torch.cuda.stream(SIDE.stream):
                        K.conv_bwd_filter(xs, gs, geom[0], geom[1], out=sink, xform=xform, xform_plane_rows=xform_plane_rows, accumulate=acc)
                finally:
                    K.WS_LANE[0] = 0
                SIDE.keep.append((xs, gs, xform))
            else:
                K.conv_bwd_filter(xs, gs, geom[0], geom[1], out=sink, xform=xform, xform_plane_rows=xform_plane_rows, accumulate=acc)
            _notify(w)
            return None
    return ConvBwdFilterFn.apply(x, gpre, geom)


def _pair_ok(g, other, w):
    """Final (first-order) backward, sunk filter gradient, bf16 tensors on one stream: the layer's two backward GEMMs may share a
    launch (kernels.conv_bwd_pair).  Everything else keeps the two differentiable Functions."""
    return (not torch.is_grad_enabled() and SIDE.stream is None and g.dtype == torch.bfloat16 and
            other.dtype == torch.bfloat16 and g.is_cuda and sink_at(w.data_ptr()) is not None)


@contextlib.contextmanager
def input_grads_only():
    prev = _INPUTS_ONLY[0]
    _INPUTS_ONLY[0] = True
    try:
        yield
    finally:
        _INPUTS_ONLY[0] = prev


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


class ActBwdFn(Function):
    """gy * act'(.) with the derivative read from the activation OUTPUT y.  Linear in gy; piecewise-constant in y for
    lrelu/relu (zero second derivative — only the mask propagates into the double backward)."""

    @staticmethod
    def forward(ctx, gy, y, act, alpha):
        ctx.save_for_backward(y)
        ctx.act, ctx.alpha = act, alpha
        ctx.set_materialize_grads(False)
        return K.act_bwd(_c(gy), y, act, alpha)

    @staticmethod
    def backward(ctx, gg):
        if gg is None:
            return None, None, None, None
        (y,) = ctx.saved_tensors
        return ActBwdFn.apply(gg, y, ctx.act, ctx.alpha), None, None, None


def _act_bwd(gy, y, act, alpha):
    return ActBwdFn.apply(gy, y, act, alpha) if act != K.ACT_NONE else _c(gy)


class ColSumFn(Function):
    """[rows, C] -> [C]  (bias gradients)."""

    @staticmethod
    def forward(ctx, a):
        ctx.shape, ctx.dtype = a.shape, a.dtype
        return K.col_reduce(_c(a))[0]

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).expand(ctx.shape)


class Conv2dFn(Function):
    """y = act(conv(x, w) + b): reference utils/ops.py:58-63.  geom = (ConvDesc, workspace_bytes)."""

    @staticmethod
    def forward(ctx, x, w, b, geom, act, alpha, want_stats=False, out_dtype=None):
        """out_dtype: None = the storage mode's rule (kernels._act_dtype); a gradient piece passes the dtype of the tensor it is the
        gradient of, so that autograd never has to cast (bf16 storage)."""
        d, ws = geom
        x = _c(x)
        ctx.set_materialize_grads(False)   # an undefined upstream gradient must not become a zero-filled conv launch
        # want_stats: a batch norm consumes this output next; the GEMM epilogue leaves it the per-tile column sums
        # the filter gradient of this layer transforms the same x (fp32 Winograd): keep the transform if a gradient will be asked for
        ctx.geom_b = K.bwd_geom(geom)       # the backward GEMMs' descriptor (kernels.math_scope(bwd_math=...)); usually geom itself
        keep = bool(ctx.needs_input_grad[1]) and not _INPUTS_ONLY[0] and ctx.geom_b is geom
        y = (K.conv_fwd_stats(x, w, b, d, ws, act, alpha, keep_xform=keep, out_dtype=out_dtype) if want_stats
             else K.conv_fwd(x, w, b, d, ws, act, alpha, keep_xform=keep, out_dtype=out_dtype))
        ctx.xform = K.LAST_XFORM[0] if keep else None
        K.LAST_XFORM[0] = None
        ctx.save_for_backward(x, w, y if act != K.ACT_NONE else None)
        ctx.geom, ctx.act, ctx.alpha, ctx.has_bias = geom, act, alpha, b is not None
        ctx.bias_ref = b            # only its address is used (gradient sink lookup)
        return y

    @staticmethod
    def backward(ctx, gy):
        if gy is None:
            return None, None, None, None, None, None, None, None
        x, w, y = ctx.saved_tensors
        gx, gw, gb = conv2d_backward(x, w, y, gy, ctx.geom_b, ctx.act, ctx.alpha, ctx.has_bias, ctx.bias_ref, ctx.needs_input_grad[:3], ctx.xform)
        ctx.xform = None
        return gx, gw, gb, None, None, None, None, None


def conv2d_backward(x, w, y, gy, geom_b, act, alpha, has_bias, bias_ref, need, xform=None, xform_plane_rows=0):
    """Backward of y = act(conv(x, w) + b) for upstream gradient gy -> (gx, gw, gb); need = (x, w, b) wanted.  Shared by Conv2dFn and
    the per-part cases of stacked.SConv2dFn (a slice of a stacked pass is an ordinary pass of its own)."""
    params = not _INPUTS_ONLY[0]
    want_b = has_bias and need[2] and params
    gb = None
    bsink = _sink_of(bias_ref) if want_b else None
    if (want_b and act != K.ACT_NONE and not torch.is_grad_enabled() and gy.shape[-1] % 4 == 0):
        # final (first-order) backward: activation backward and bias gradient in ONE pass over the tensor
        gpre, gb = K.act_bwd_colsum(_c(gy), y, act, alpha, out=bsink)
        if bsink is not None:
            gb = None                       # already summed into the optimizer's arena
            _notify(bias_ref)
    else:
        gpre = _act_bwd(gy, y, act, alpha)
        if want_b and bsink is not None:
            K.col_reduce(_c(gpre), out=bsink)
            _notify(bias_ref)
        elif want_b:
            gb = ColSumFn.apply(gpre)
    if need[0] and need[1] and params and _pair_ok(gpre, x, w):
        # final backward on bf16 tensors: the input gradient and the (sunk) filter gradient in one launch
        gx = K.conv_bwd_pair(K.PAIR_BWD_DATA, _c(gpre), w, _c(x), _c(gpre), geom_b[0], geom_b[1], sink_at(w.data_ptr()), out_dtype=x.dtype,
                             accumulate=sink_accumulate(w.data_ptr()))
        _notify(w)
        return gx, None, gb
    gx = ConvBwdDataFn.apply(gpre, w, None, geom_b, K.ACT_NONE, 0.0, x.dtype) if need[0] else None
    gw = _filter_grad(x, gpre, geom_b, w, xform, xform_plane_rows) if (need[1] and params) else None
    return gx, gw, gb


class ConvBwdDataFn(Function):
    """dx = act(conv^T(dy, w) + b).  As a backward piece: b=None, act=NONE.  As a forward op this is
    tf conv2d_transpose (reference utils/ops.py:66-71) — same kernel, TF deconv filters are already HWIO of the adjoint."""

    @staticmethod
    def forward(ctx, dy, w, b, geom, act, alpha, out_dtype=None):
        d, ws = geom
        dy = _c(dy)
        ctx.set_materialize_grads(False)
        out = K.conv_bwd_data(dy, w, b, d, ws, act, alpha, out_dtype=out_dtype)
        ctx.save_for_backward(dy, w, out if act != K.ACT_NONE else None)
        ctx.geom, ctx.act, ctx.alpha, ctx.has_bias = geom, act, alpha, b is not None
        ctx.geom_b = K.bwd_geom(geom)
        ctx.bias_ref = b
        return out

    @staticmethod
    def backward(ctx, gg):
        if gg is None:
            return None, None, None, None, None, None, None
        dy, w, out = ctx.saved_tensors
        g_dy, g_w, g_b = bwd_data_backward(dy, w, out, gg, ctx.geom_b, ctx.act, ctx.alpha, ctx.has_bias, ctx.bias_ref, ctx.needs_input_grad[:3])
        return g_dy, g_w, g_b, None, None, None, None


def bwd_data_backward(dy, w, out, gg, geom_b, act, alpha, has_bias, bias_ref, need):
    """Backward of out = act(conv^T(dy, w) + b) for upstream gradient gg -> (g_dy, g_w, g_b).  Shared by ConvBwdDataFn and
    stacked.SBwdDataFn (whose double backward runs on the x_hat rows only)."""
    gpre = _act_bwd(gg, out, act, alpha)
    params = not _INPUTS_ONLY[0]
    if need[0] and need[1] and params and _pair_ok(gpre, dy, w):
        g_dy = K.conv_bwd_pair(K.PAIR_FWD, _c(gpre), w, _c(gpre), _c(dy), geom_b[0], geom_b[1], sink_at(w.data_ptr()), out_dtype=dy.dtype,
                               accumulate=sink_accumulate(w.data_ptr()))
        _notify(w)
        g_w = None
    else:
        g_dy = Conv2dFn.apply(gpre, w, None, geom_b, K.ACT_NONE, 0.0, False, dy.dtype) if need[0] else None
        g_w = _filter_grad(gpre, dy, geom_b, w) if (need[1] and params) else None
    g_b = None
    if has_bias and need[2] and params:
        bsink = _sink_of(bias_ref)
        if bsink is not None:
            K.col_reduce(_c(gpre), out=bsink)
            _notify(bias_ref)
        else:
            g_b = ColSumFn.apply(gpre)
    return g_dy, g_w, g_b


class ConvBwdFilterFn(Function):
    """dw = x (*) dy."""

    @staticmethod
    def forward(ctx, x, dy, geom):
        d, ws = geom
        x, dy = _c(x), _c(dy)
        ctx.save_for_backward(x, dy)
        ctx.geom = geom
        return K.conv_bwd_filter(x, dy, d, ws)

    @staticmethod
    def backward(ctx, ggw):
        x, dy = ctx.saved_tensors
        ggw = _c(ggw)
        g_x = ConvBwdDataFn.apply(dy, ggw, None, ctx.geom, K.ACT_NONE, 0.0, x.dtype) if ctx.needs_input_grad[0] else None
        g_dy = Conv2dFn.apply(x, ggw, None, ctx.geom, K.ACT_NONE, 0.0, False, dy.dtype) if ctx.needs_input_grad[1] else None
        return g_x, g_dy, None


class AddActFn(Function):
    """y = act(a + b): the residual joins (reference models/wgancls/model.py:145-146,190-191,206-207)."""

    @staticmethod
    def forward(ctx, a, b, act, alpha):
        ctx.set_materialize_grads(False)
        y = K.add_act(_c(a), _c(b), act, alpha)
        ctx.save_for_backward(y if act != K.ACT_NONE else None)
        ctx.act, ctx.alpha = act, alpha
        return y

    @staticmethod
    def backward(ctx, gy):
        if gy is None:
            return None, None, None, None
        (y,) = ctx.saved_tensors
        g = _act_bwd(gy, y, ctx.act, ctx.alpha)
        return g, g, None, None


class ConcatTileFn(Function):
    """[B,H,W,Cf] ++ tile([B,Ce]) -> [B,H,W,Cf+Ce]  (reference models/wgancls/model.py:153-155)."""

    @staticmethod
    def forward(ctx, feat, emb):
        ctx.cf, ctx.ce = feat.shape[-1], emb.shape[-1]
        ctx.set_materialize_grads(False)
        return K.concat_tile_fwd(_c(feat), _c(emb))

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        return ConcatTileBwdFn.apply(g, ctx.cf, ctx.ce)


class ConcatTileBwdFn(Function):
    @staticmethod
    def forward(ctx, g, cf, ce):
        return K.concat_tile_bwd(_c(g), cf, ce)

    @staticmethod
    def backward(ctx, gg_feat, gg_emb):
        return ConcatTileFn.apply(gg_feat, gg_emb), None, None


class NchwToNhwcFn(Function):
    """physical [B,C,H,W] -> physical [B,H,W,C] (reference utils/ops.py:132-134 to_nhwc)."""

    @staticmethod
    def forward(ctx, x):
        return K.nchw_to_nhwc(_c(x))

    @staticmethod
    def backward(ctx, g):
        return NhwcToNchwFn.apply(g)


class NhwcToNchwFn(Function):
    @staticmethod
    def forward(ctx, x):
        return K.nhwc_to_nchw(_c(x))

    @staticmethod
    def backward(ctx, g):
        return NchwToNhwcFn.apply(g)


class ActFn(Function):
    """y = act(x) as a standalone op (first-order for tanh, any order for lrelu/relu)."""

    @staticmethod
    def forward(ctx, x, act, alpha):
        y = K.act_fwd(_c(x), act, alpha)
        ctx.save_for_backward(y)
        ctx.act, ctx.alpha = act, alpha
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return ActBwdFn.apply(gy, y, ctx.act, ctx.alpha), None, None


class BatchNormTrainFn(Function):
    """Training-mode fused batch norm + activation: reference utils/ops.py:7-29.  Normalises with the biased batch
    variance; if moving_mean/var are given they are updated in place with the unbiased one (TF UPDATE_OPS semantics are
    decided by the caller).  Generator only => first order."""

    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, eps, decay, act, alpha, moving_updates=1):
        x = _c(x)
        C = x.shape[-1]
        n = x.numel() // C
        # statistics (the producing conv's epilogue partials when ops.conv2d(..., stats=True) left any, else a pass over x;
        # numerically stable either way) and the finalize step in one chain of launches
        # round 5: one entry point — [first stage unless the conv left tile partials] -> [second stage + finalize] -> [normalise], the
        # middle launch folded into the last one's prologue for the small tensors (t2i_bn_train_fwd_grouped with groups = 1); the
        # separate statistics / normalise calls of rounds 1-4 remain for what that entry point refuses (C % 4 != 0, misaligned tensors)
        if C % 4 == 0 and x.data_ptr() % 16 == 0 and gamma.data_ptr() % 4 == 0:
            y, mean, rstd = K.bn_train_fwd_grouped(x, gamma, beta, eps, decay, 1, act, alpha, moving_mean, moving_var, moving_updates)
            mean, rstd = mean[0], rstd[0]
        else:
            for _ in range(moving_updates - 1 if moving_mean is not None else 0):      # (rare path: the statistics pass again per extra update)
                K.bn_train_stats(x, gamma, beta, eps, decay, moving_mean, moving_var)
            mean, rstd, scale, shift = K.bn_train_stats(x, gamma, beta, eps, decay, moving_mean, moving_var)
            y = K.bn_apply(x, scale, shift, act, alpha)
        ctx.save_for_backward(x, gamma, mean, rstd, y if act != K.ACT_NONE else None)
        ctx.act, ctx.alpha = act, alpha
        ctx.gamma_ref, ctx.beta_ref = gamma, beta
        ctx.mark_non_differentiable(mean, rstd)
        ctx.set_materialize_grads(False)     # else the engine zero-fills a gradient for mean and rstd on every backward
        return y, mean, rstd

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gm, _gr):
        if gy is None:
            return (None,) * 10
        x, gamma, mean, rstd, y = ctx.saved_tensors
        gy = _c(gy)
        fused = gy.shape[-1] % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (gy, x, mean))
        if not fused:
            if ctx.act != K.ACT_NONE:
                gy = K.act_bwd(gy, y, ctx.act, ctx.alpha)
            sum_dy, sum_dy_x = K.col_reduce(gy, x, True, center=mean)     # sum dy, sum dy * (x - mean)
        # gamma / beta that do not require a gradient (a critic with batch norm run under store.frozen() in the generator
        # step: detached views that share the real parameters' addresses) must neither reach the sinks nor be announced
        want_g, want_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gsink = _sink_of(ctx.gamma_ref) if want_g else None
        bsink = _sink_of(ctx.beta_ref) if want_b else None
        sunk = gsink is not None and bsink is not None
        if fused:      # [act backward + both reductions] -> [second stage + coefficients + dx]: two launches when the partials are few
            dx, dgamma, dbeta = K.bn_bwd_grouped(gy, y if ctx.act != K.ACT_NONE else None, x, mean, rstd, gamma, 1, ctx.act, ctx.alpha,
                                                 dgamma_out=gsink if sunk else None, dbeta_out=bsink if sunk else None)
        else:
            dx, dgamma, dbeta = K.bn_bwd(gy, x, mean, rstd, gamma, sum_dy, sum_dy_x, dgamma_out=gsink if sunk else None,
                                         dbeta_out=bsink if sunk else None)
        if sunk:
            _notify(ctx.gamma_ref); _notify(ctx.beta_ref)
            return dx, None, None, None, None, None, None, None, None, None
        return dx, (dgamma if want_g else None), (dbeta if want_b else None), None, None, None, None, None, None, None


class BatchNormTrainGroupedFn(Function):
    """Training-mode batch norm of a BATCHED pass whose `groups` equal slices along the batch axis are separate passes of the
    reference graph (models/gancls/model.py:48-51: the critic on fake / match / mismatch images, each with its own batch statistics):
    statistics, normalisation and backward per slice, while every convolution around it runs once on the whole batch.  Moving averages
    move once per slice, in slice order (what three sequential passes did); dgamma / dbeta are summed over the slices.  Three launches
    forward, three backward for all slices (t2i_bn_train_fwd_grouped / t2i_bn_bwd_grouped; C % 4 == 0 and 16-byte alignment — otherwise
    the slices go through the ordinary kernels one by one, forward AND backward: tests/test_kernels_gpu.py::
    test_grouped_batch_norm_odd_channels).  First order only."""

    @staticmethod
    def _fast(x, groups):
        b = x.shape[0] // groups
        return x.shape[-1] % 4 == 0 and x.data_ptr() % 16 == 0 and (x[:b].numel() * x.element_size()) % 16 == 0

    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, eps, decay, act, alpha, groups):
        x = _c(x)
        Bt = x.shape[0]
        assert Bt % groups == 0, (Bt, groups)
        b = Bt // groups
        ctx.fast = BatchNormTrainGroupedFn._fast(x, groups)
        if ctx.fast:
            y, mean, rstd = K.bn_train_fwd_grouped(x, gamma, beta, eps, decay, groups, act, alpha, moving_mean, moving_var)
            stats = [mean, rstd]
        else:
            stats, scales, shifts = [], [], []
            for g in range(groups):
                mean, rstd, scale, shift = K.bn_train_stats(x[g * b:(g + 1) * b], gamma, beta, eps, decay, moving_mean, moving_var)
                stats += [mean, rstd]
                scales.append(scale); shifts.append(shift)
            y = K.bn_apply_groups(x, scales, shifts, act, alpha)
        ctx.save_for_backward(x, gamma, y if act != K.ACT_NONE else None, *stats)
        ctx.act, ctx.alpha, ctx.groups = act, alpha, groups
        ctx.gamma_ref, ctx.beta_ref = gamma, beta
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        if gy is None:
            return (None,) * 10
        x, gamma, y = ctx.saved_tensors[:3]
        stats = ctx.saved_tensors[3:]
        gy = _c(gy)
        groups = ctx.groups
        b = x.shape[0] // groups
        want_g, want_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gsink = _sink_of(ctx.gamma_ref) if want_g else None
        bsink = _sink_of(ctx.beta_ref) if want_b else None
        sunk = gsink is not None and bsink is not None
        if ctx.fast and gy.data_ptr() % 16 == 0:
            dx, dgamma, dbeta = K.bn_bwd_grouped(gy, y if ctx.act != K.ACT_NONE else None, x, stats[0], stats[1], gamma, groups, ctx.act, ctx.alpha,
                                                 dgamma_out=gsink if sunk else None, dbeta_out=bsink if sunk else None)
        else:
            if ctx.fast:                 # per-group views of the [groups, C] statistics
                stats = [t[g] for g in range(groups) for t in (stats[0], stats[1])]
            vec = gy.shape[-1] % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (gy, x)) and (x[:b].numel() * x.element_size()) % 16 == 0
            dx = torch.empty_like(x)
            dgamma = dbeta = None
            for g in range(groups):
                sl = slice(g * b, (g + 1) * b)
                if vec:
                    _, dg, db = K.bn_bwd_fused(gy[sl], y[sl] if ctx.act != K.ACT_NONE else None, x[sl], stats[2 * g], stats[2 * g + 1], gamma, ctx.act,
                                               ctx.alpha, dgamma_out=gsink if sunk else None, dbeta_out=bsink if sunk else None, out=dx[sl])
                else:
                    # a channel count that is not a multiple of 4 (an odd DF_DIM), or unaligned slices: the scalar kernels, slice by slice
                    # — activation backward, the two column reductions about the slice's mean, then the batch-norm backward itself
                    gs = K.act_bwd(_c(gy[sl]), _c(y[sl]), ctx.act, ctx.alpha) if ctx.act != K.ACT_NONE else _c(gy[sl])
                    xs = _c(x[sl])
                    sum_dy, sum_dy_x = K.col_reduce(gs, xs, True, center=stats[2 * g])
                    dxs, dg, db = K.bn_bwd(gs, xs, stats[2 * g], stats[2 * g + 1], gamma, sum_dy, sum_dy_x,
                                           dgamma_out=gsink if sunk else None, dbeta_out=bsink if sunk else None)
                    dx[sl].copy_(dxs)
                if not sunk:
                    dgamma = dg if dgamma is None else dgamma + dg
                    dbeta = db if dbeta is None else dbeta + db
        if sunk:
            _notify(ctx.gamma_ref); _notify(ctx.beta_ref)
            return (dx,) + (None,) * 9
        return (dx, dgamma if want_g else None, dbeta if want_b else None) + (None,) * 7


class GpSlopesFn(Function):
    """slopes[b] = ||g[b]||_2 (reference models/wgancls/model.py:64,69).  Its backward feeds the double backward of the
    critic; it is itself only differentiated once."""

    @staticmethod
    def forward(ctx, g):
        g = _c(g)
        s = K.gp_slopes(g)
        ctx.save_for_backward(g, s)
        return s

    @staticmethod
    @once_differentiable
    def backward(ctx, ds):
        g, s = ctx.saved_tensors
        # coef_b = where(s > 0, ds / clamp_min(s, 1e-30), 0), formed inside the kernel (five tensor-library launches per term before)
        return K.row_scale_div(g, _c(ds), s)


# ---- PGGAN operators (reference utils/ops.py:74-81,100-101,109-111) ------------------------------------------------------
class Pool2Fn(Function):
    """scale * 2x2 window sum, stride 2 (scale = 1/4: tf.nn.pool AVG SAME on even extents).  Linear; its adjoint is the
    nearest-neighbour replication with the same scale, so the pair is closed under differentiation of any order (the
    critic of PGGAN is differentiated twice by the gradient penalty)."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        ctx.set_materialize_grads(False)
        return K.pool2_sum(_c(x), scale)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        return Upscale2Fn.apply(g, ctx.scale), None


class Upscale2Fn(Function):
    """scale * nearest-neighbour x2 (scale = 1: ops.upscale)."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        ctx.set_materialize_grads(False)
        return K.upscale2(_c(x), scale)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        return Pool2Fn.apply(g, ctx.scale), None


class AxpbyFn(Function):
    """alpha*a + beta*b with host scalars: the fade-in mix of a new resolution (reference models/pggan/pggan.py:267,314)."""

    @staticmethod
    def forward(ctx, a, alpha, b, beta):
        ctx.alpha, ctx.beta, ctx.has_b = alpha, beta, b is not None
        ctx.set_materialize_grads(False)
        return K.axpby(_c(a), alpha, _c(b) if b is not None else None, beta)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        ga = AxpbyFn.apply(g, ctx.alpha, None, 0.0) if ctx.needs_input_grad[0] else None
        gb = AxpbyFn.apply(g, ctx.beta, None, 0.0) if (ctx.has_b and ctx.needs_input_grad[2]) else None
        return ga, None, gb, None


class LayerNormFn(Function):
    """tf.contrib.layers.layer_norm(x, begin_norm_axis=1, begin_params_axis=-1) + activation (reference utils/ops.py:74-81):
    each sample is normalised over all of its elements (biased variance, eps = 1e-12), then scaled and shifted per
    last-axis channel.  The backward is LayerNormBwdFn, which has a backward of its own: usable in a critic under the gradient
    penalty.  x itself is saved only as the graph handle through which d2L/dx reaches the input."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, act, alpha):
        x_in = x
        x = _c(x)
        B = x.shape[0]
        n = x.numel() // B
        s1, s2 = K.row_moments(x)
        mean = s1 / n
        var = torch.clamp(s2 / n - mean * mean, min=0.0)
        rstd = torch.rsqrt(var + eps)
        xhat = K.row_fma2(x, rstd, delta=-mean * rstd)
        y = K.bn_apply(xhat, gamma, beta, act, alpha)               # per-channel affine + activation
        ctx.save_for_backward(x_in, xhat, rstd, gamma, y if act != K.ACT_NONE else None)
        ctx.act, ctx.alpha, ctx.n = act, alpha, n
        return y

    @staticmethod
    def backward(ctx, gy):
        x, xhat, rstd, gamma, y = ctx.saved_tensors
        dx, dgamma, dbeta = LayerNormBwdFn.apply(gy, x, gamma, xhat, rstd, y.detach() if y is not None else None, ctx.act, ctx.alpha, ctx.n,
                                                 not _INPUTS_ONLY[0])
        return dx, dgamma, dbeta, None, None, None


class LayerNormBwdFn(Function):
    """(dx, dgamma, dbeta) of LayerNormFn from gy; x is only the handle that carries this Function's own gradient to the forward's
    input (xhat and rstd are kernel outputs without a graph).  want_params = False (the first-order pass of the gradient penalty,
    input_grads_only): the dgamma / dbeta column reductions are not launched and None is returned for them.
    backward = the double backward, for the cotangent v of dx: the five per-sample sums (two launches), one elementwise launch that
    writes dL/dgy and dL/dx, and the column reduction for dL/dgamma when gamma asks for it.  The penalty differentiates a gradient
    once => once_differentiable; cotangents for dgamma / dbeta (the gradient of a parameter gradient) are refused."""

    @staticmethod
    def forward(ctx, gy, x, gamma, xhat, rstd, y, act, alpha, n, want_params):
        gy = _c(gy)
        gz = K.act_bwd(gy, y, act, alpha) if act != K.ACT_NONE else gy
        dbeta = dgamma = None
        if want_params:
            dbeta, dgamma = K.col_reduce(gz, xhat, True)                # sum gz, sum gz * xhat over rows of [*, C]
        g = K.bn_apply(gz, gamma, torch.zeros_like(gamma), K.ACT_NONE, 0.0)
        t1, t2 = K.row_moments(g, xhat)
        dx = K.row_fma2(g, rstd, xhat, -rstd * t2 / n, -rstd * t1 / n)
        ctx.save_for_backward(gy, xhat, rstd, gamma, y)
        ctx.act, ctx.alpha = act, alpha
        ctx.set_materialize_grads(False)
        return dx, dgamma, dbeta

    @staticmethod
    @once_differentiable
    def backward(ctx, v, v_dgamma, v_dbeta):
        if v_dgamma is not None or v_dbeta is not None:
            raise NotImplementedError('layer_norm: the gradient of a parameter gradient (dgamma / dbeta) is not implemented; the second '
                                      'order covers the input gradient dx, which is what a gradient penalty differentiates')
        if v is None:
            return (None,) * 10
        if ctx.act == K.ACT_TANH:
            raise NotImplementedError('layer_norm: second order through a fused tanh is not implemented (lrelu, relu or no activation)')
        gy, xhat, rstd, gamma, y = ctx.saved_tensors
        want_gamma = ctx.needs_input_grad[2]
        dgy, dx, hgz = K.layer_norm_bwd2(_c(v), gy, xhat, y, gamma, rstd, ctx.act, ctx.alpha, want_hgz=want_gamma)
        dgamma = K.col_reduce(hgz)[0] if want_gamma else None
        return (dgy if ctx.needs_input_grad[0] else None, dx if ctx.needs_input_grad[1] else None, dgamma) + (None,) * 7


class CaSampleKlFn(Function):
    """(code, kl) = (mean + exp(log_sigma)*eps, KL(N(mean, sigma) || N(0,1)) averaged over all elements): the conditioning
    augmentation of reference models/wgancls/model.py:117-127 as one forward and one backward launch."""

    @staticmethod
    def forward(ctx, mean, log_sigma, eps):
        mean, log_sigma, eps = _c(mean), _c(log_sigma), _c(eps)
        ctx.save_for_backward(mean, log_sigma, eps)
        ctx.set_materialize_grads(False)
        code, kl = K.ca_kl_fwd(mean, log_sigma, eps)
        return code, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, dcode, dkl):
        mean, log_sigma, eps = ctx.saved_tensors
        if dcode is None and dkl is None:
            return None, None, None
        dmean, dls = K.ca_kl_bwd(mean, log_sigma, eps, _c(dcode) if dcode is not None else None,
                                 _c(dkl).reshape(1) if dkl is not None else None)
        return dmean, dls, None


class LerpDevFn(Function):
    """mode 0: (1-t)*a + t*b;  1: t*a;  2: (1-t)*a, t in device memory (graph-replayable fade-in).  Closed under
    differentiation: the gradients are modes 2 and 1 of the incoming gradient."""

    @staticmethod
    def forward(ctx, a, b, t_dev, mode):
        ctx.t_dev, ctx.mode = t_dev, mode
        ctx.set_materialize_grads(False)
        return K.lerp_dev(_c(a), _c(b) if b is not None else None, t_dev, mode)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        if ctx.mode == 0:
            ga = LerpDevFn.apply(g, None, ctx.t_dev, 2) if ctx.needs_input_grad[0] else None
            gb = LerpDevFn.apply(g, None, ctx.t_dev, 1) if ctx.needs_input_grad[1] else None
            return ga, gb, None, None
        return (LerpDevFn.apply(g, None, ctx.t_dev, ctx.mode) if ctx.needs_input_grad[0] else None), None, None, None


# ---- the rest of the operator surface (reference utils/ops.py:94-116,145-148) ---------------------------------------------
class PixelNormFn(Function):
    """y = u / sqrt(mean_c(u^2) + eps), u = act(x), over the last axis (reference utils/ops.py:94-97): one launch forward, one backward.
    The backward (PixelNormBwdFn) works from y and the saved per-pixel 1 / norm alone (u = y * norm) and has a backward of its own: usable
    in a critic under the gradient penalty.  x is saved only as the graph handle for d2L/dx."""

    @staticmethod
    def forward(ctx, x, eps, act, alpha):
        y, rnorm = K.pixel_norm_fwd(x, eps, act, alpha)
        ctx.save_for_backward(x, y, rnorm)
        ctx.act, ctx.alpha = act, alpha
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, gy):
        if gy is None:
            return None, None, None, None
        x, y, rnorm = ctx.saved_tensors
        return PixelNormBwdFn.apply(gy, x, y.detach(), rnorm, ctx.act, ctx.alpha), None, None, None


class PixelNormBwdFn(Function):
    """dx of PixelNormFn from gy (one launch); x is only the handle that carries this Function's own gradient to the forward's input.
    backward = the double backward, one launch: dL/dgy and dL/dx for the cotangent v of dx, from v, gy, y and rnorm."""

    @staticmethod
    def forward(ctx, gy, x, y, rnorm, act, alpha):
        gy = _c(gy)
        ctx.save_for_backward(gy, y, rnorm)
        ctx.act, ctx.alpha = act, alpha
        ctx.set_materialize_grads(False)
        return K.pixel_norm_bwd(gy, y, rnorm, act, alpha)

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        if v is None:
            return (None,) * 6
        if ctx.act == K.ACT_TANH:
            raise NotImplementedError('pixel_norm: second order through a fused tanh is not implemented (lrelu, relu or no activation)')
        gy, y, rnorm = ctx.saved_tensors
        dgy, dx = K.pixel_norm_bwd2(_c(v), gy, y, rnorm, ctx.act, ctx.alpha)
        return (dgy if ctx.needs_input_grad[0] else None, dx if ctx.needs_input_grad[1] else None) + (None,) * 4


class MinibatchStddevFn(Function):
    """x [B,H,W,C] -> [B,F]: the minibatch standard deviation of the progressive-growing paper's critic —
    per group of G contiguous samples and chunk of C/F channels, the mean over the chunk's columns of the standard deviation across
    the group.  Only x is saved: the backward (MinibatchStddevBwdFn) recomputes mean and deviation from it, and has a backward of its
    own, so the layer may sit in a critic under the gradient penalty."""

    @staticmethod
    def forward(ctx, x, group, features, eps):
        ctx.save_for_backward(x)
        ctx.group, ctx.features, ctx.eps = group, features, eps
        ctx.set_materialize_grads(False)
        return K.minibatch_stddev_fwd(_c(x), group, features, eps)

    @staticmethod
    def backward(ctx, gs):
        if gs is None:
            return None, None, None, None
        x, = ctx.saved_tensors
        return MinibatchStddevBwdFn.apply(gs, x, ctx.group, ctx.features, ctx.eps), None, None, None


class MinibatchStddevBwdFn(Function):
    """dx of MinibatchStddevFn from gs [B,F] (one launch).  backward = the double backward for the cotangent v of dx: dL/dgs and
    dL/dx from v, x and gs (two launches).  The penalty differentiates a gradient once => once_differentiable."""

    @staticmethod
    def forward(ctx, gs, x, group, features, eps):
        gs, x = _c(gs), _c(x)
        ctx.save_for_backward(gs, x)
        ctx.group, ctx.features, ctx.eps = group, features, eps
        ctx.set_materialize_grads(False)
        return K.minibatch_stddev_bwd(gs, x, group, features, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        if v is None:
            return (None,) * 5
        gs, x = ctx.saved_tensors
        dxx, dgs = K.minibatch_stddev_bwd2(_c(v), x, gs, ctx.group, ctx.features, ctx.eps)
        return (dgs if ctx.needs_input_grad[0] else None, dxx if ctx.needs_input_grad[1] else None, None, None, None)


class ResizeNearestFn(Function):
    """tf.image.resize_nearest_neighbor (reference utils/ops.py:104-116), [B,H,W,C] -> [B,Ho,Wo,C].  Linear; its backward is
    ResizeNearestAdjFn, whose backward is this Function again: closed under differentiation of any order (usable inside the critic
    under the gradient penalty, like Pool2Fn / Upscale2Fn)."""

    @staticmethod
    def forward(ctx, x, Ho, Wo):
        ctx.hw = (x.shape[1], x.shape[2])
        ctx.set_materialize_grads(False)
        return K.resize_nearest(_c(x), Ho, Wo)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        return ResizeNearestAdjFn.apply(g, ctx.hw[0], ctx.hw[1]), None, None


class ResizeNearestAdjFn(Function):
    """The adjoint of the nearest resize from an [B,H,W,C] map: every input pixel gathers the sum of its block of output pixels."""

    @staticmethod
    def forward(ctx, g, H, W):
        ctx.out_hw = (g.shape[1], g.shape[2])
        ctx.set_materialize_grads(False)
        return K.resize_nearest_adj(_c(g), H, W)

    @staticmethod
    def backward(ctx, gg):
        if gg is None:
            return None, None, None
        return ResizeNearestFn.apply(gg, ctx.out_hw[0], ctx.out_hw[1]), None, None


class DiffAugmentFn(Function):
    """y = T(x): the differentiable augmentation of DESIGN.md section 4.35 (colour / translation / cutout, one row of the device table P
    [B,9] per sample).  Affine in x; its backward is DiffAugmentAdjFn, whose backward is this Function again without the brightness
    offset: closed under differentiation of any order (usable in front of a critic under the gradient penalty).  P carries no gradient."""

    @staticmethod
    def forward(ctx, x, P, policy, offset):
        ctx.save_for_backward(P)
        ctx.policy = policy
        ctx.set_materialize_grads(False)
        return K.diff_augment_fwd(_c(x), P, policy, offset)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        P, = ctx.saved_tensors
        return DiffAugmentAdjFn.apply(g, P, ctx.policy), None, None, None


class DiffAugmentAdjFn(Function):
    """dx = A^T g, the adjoint of the linear part A of DiffAugmentFn; backward: A itself (DiffAugmentFn with offset=False)."""

    @staticmethod
    def forward(ctx, g, P, policy):
        ctx.save_for_backward(P)
        ctx.policy = policy
        ctx.set_materialize_grads(False)
        return K.diff_augment_adj(_c(g), P, policy)

    @staticmethod
    def backward(ctx, gg):
        if gg is None:
            return None, None, None
        P, = ctx.saved_tensors
        return DiffAugmentFn.apply(gg, P, ctx.policy, False), None, None


class UpFirDn2dFn(Function):
    """Anti-aliased resampling: zero insertion by u, pads (p0, p1), FIR filter with the host floats `taps`
    (reversed when flip), decimation by d, along H and W of [B,H,W,C].  Linear, and its adjoint is the same operator with
    K.upfirdn2d_adjoint's parameters: the backward applies this Function itself, so it is differentiable to any order with one kernel
    family (usable under the gradient penalty).  p1 is a pair (along H, along W).  No gradient flows to the taps."""

    @staticmethod
    def forward(ctx, x, taps, u, d, p0, p1, flip):
        ctx.args = (taps, u, d, p0, flip)
        ctx.hw = (x.shape[1], x.shape[2])
        ctx.set_materialize_grads(False)
        return K.upfirdn2d(_c(x), taps, u, d, p0, p1, flip)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None, None
        taps, u, d, p0, flip = ctx.args
        ua, da, p0a, p1h, fa = K.upfirdn2d_adjoint(ctx.hw[0], g.shape[1], len(taps), u, d, p0, flip)
        p1w = K.upfirdn2d_adjoint(ctx.hw[1], g.shape[2], len(taps), u, d, p0, flip)[3]
        return UpFirDn2dFn.apply(g, taps, ua, da, p0a, (p1h, p1w), fa), None, None, None, None, None, None


class PoolAvgFn(Function):
    """tf.nn.pool AVG, window = stride = s, SAME, any extents (the mean of the taps inside the image).  Linear; adjoint: PoolAvgAdjFn."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s, ctx.hw = s, (x.shape[1], x.shape[2])
        ctx.set_materialize_grads(False)
        return K.pool_same_fwd(_c(x), s, K.POOL_AVG)[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        return PoolAvgAdjFn.apply(g, ctx.hw[0], ctx.hw[1], ctx.s), None


class PoolAvgAdjFn(Function):
    """dx[pixel] = g[its window] / count(its window); its backward is the average pool again."""

    @staticmethod
    def forward(ctx, g, H, W, s):
        ctx.s = s
        ctx.set_materialize_grads(False)
        return K.pool_same_bwd(_c(g), None, H, W, s, K.POOL_AVG)

    @staticmethod
    def backward(ctx, gg):
        if gg is None:
            return None, None, None, None
        return PoolAvgFn.apply(gg, ctx.s), None, None, None


class PoolMaxFn(Function):
    """tf.nn.pool MAX, window = stride = s, SAME (padding ignored).  The forward records the window offset of each first maximum;
    with those fixed the pool is the linear map PoolMaxTakeFn, and the derivatives are that map's (PoolMaxPutFn <-> PoolMaxTakeFn).
    The offsets are written only when x asks for a gradient (nothing produced under no_grad does): inference pays for y alone."""

    @staticmethod
    def forward(ctx, x, s):
        y, idx = K.pool_same_fwd(_c(x), s, K.POOL_MAX, want_idx=ctx.needs_input_grad[0])
        ctx.s, ctx.hw, ctx.idx = s, (x.shape[1], x.shape[2]), idx
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        return PoolMaxPutFn.apply(g, ctx.idx, ctx.hw[0], ctx.hw[1], ctx.s), None


class PoolMaxPutFn(Function):
    """dx[pixel] = g[its window] where the window's recorded offset is this pixel's, else 0."""

    @staticmethod
    def forward(ctx, g, idx, H, W, s):
        ctx.s, ctx.idx = s, idx
        ctx.set_materialize_grads(False)
        return K.pool_same_bwd(_c(g), idx, H, W, s, K.POOL_MAX)

    @staticmethod
    def backward(ctx, gg):
        if gg is None:
            return None, None, None, None, None
        return PoolMaxTakeFn.apply(gg, ctx.idx, ctx.s), None, None, None, None


class PoolMaxTakeFn(Function):
    """y[window] = x at the window's recorded offset."""

    @staticmethod
    def forward(ctx, x, idx, s):
        ctx.s, ctx.idx, ctx.hw = s, idx, (x.shape[1], x.shape[2])
        ctx.set_materialize_grads(False)
        return K.pool_same_take(_c(x), idx, s)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        return PoolMaxPutFn.apply(g, ctx.idx, ctx.hw[0], ctx.hw[1], ctx.s), None, None


class MulFn(Function):
    """a * f with a constant factor tensor f (no gradient to f): its own adjoint, so differentiable to any order."""

    @staticmethod
    def forward(ctx, a, f):
        ctx.f = f
        ctx.set_materialize_grads(False)
        return K.mul(_c(a), f)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        return MulFn.apply(g, ctx.f), None


class GnFn(Function):
    """y = x * m^n, n ~ N(0, 1) per element (reference utils/ops.py:145-148): one launch writes y and the factor f = m^n; the
    backward is g * f (MulFn), which is its own adjoint.  f is written only when x asks for a gradient; the draw is the same either way."""

    @staticmethod
    def forward(ctx, x, log_m):
        y, f = K.gn_fwd(_c(x), log_m, want_f=ctx.needs_input_grad[0])
        ctx.f = f
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        return MulFn.apply(g, ctx.f), None


class BatchRenormTrainFn(Function):
    """Training-mode batch renormalisation (tf.contrib.layers.batch_norm(renorm=True), non-fused path; reference utils/ops.py:32-55):
    y = act(((x - mu) / sigma * r + d) * gamma + beta) with r, d [C] constants for the gradient.  Built from the batch-norm kernels:
    the caller supplies mu and rstd = 1 / sigma (kernels.bn_stats); the forward is one bn_apply with scale = gamma r / sigma, the
    backward is the batch-norm backward with gamma r in place of gamma for dx, dbeta = sum g, dgamma = r sum g xhat + d sum g.
    First order, like BatchNormTrainFn."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean, rstd, r, d, act, alpha):
        x = _c(x)
        scale = gamma * r * rstd
        shift = beta + gamma * d - mean * scale
        y = K.bn_apply(x, scale.contiguous(), shift.contiguous(), act, alpha)
        ctx.save_for_backward(x, gamma, mean, rstd, r, d, y if act != K.ACT_NONE else None)
        ctx.act, ctx.alpha = act, alpha
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        if gy is None:
            return (None,) * 9
        x, gamma, mean, rstd, r, d, y = ctx.saved_tensors
        gy = _c(gy)
        if ctx.act != K.ACT_NONE:
            gy = K.act_bwd(gy, y, ctx.act, ctx.alpha)
        sum_dy, sum_dy_x = K.col_reduce(gy, x, True, center=mean)         # sum g, sum g * (x - mu)
        dx, g_xhat, dbeta = K.bn_bwd(gy, x, mean, rstd, (gamma * r).contiguous(), sum_dy, sum_dy_x)      # g_xhat = sum g * xhat
        dgamma = r * g_xhat + d * dbeta
        return (dx, dgamma if ctx.needs_input_grad[1] else None, dbeta if ctx.needs_input_grad[2] else None) + (None,) * 6


class AdaINFn(Function):
    """The style-based generator's layer epilogue (Karras et al. 2019; not in the reference):
    u = act(x + strength[c] noise[b,h,w]) (u = act(x) without noise), instance norm over (h, w), y = uhat (1 + ys) + yb.  Saves x, noise,
    strength, ys, mean and rstd only: the backward recomputes u.  noise gets no gradient.  First order: the generator is never under
    the gradient penalty, so the backward of the backward (AdaINBwdFn.backward) raises NotImplementedError."""

    @staticmethod
    def forward(ctx, x, ys, yb, noise, strength, act, alpha, eps):
        y, mean, rstd = K.adain_fwd(x, ys, yb, noise, strength, act, alpha, eps)
        ctx.save_for_backward(x, ys, noise, strength, mean, rstd)
        ctx.act, ctx.alpha = act, alpha
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, gy):
        if gy is None:
            return (None,) * 8
        x, ys, noise, strength, mean, rstd = ctx.saved_tensors
        want_strength = strength is not None and ctx.needs_input_grad[4] and not _INPUTS_ONLY[0]
        dx, dstrength, dys, dyb = AdaINBwdFn.apply(gy, x, ys, noise, strength, mean, rstd, ctx.act, ctx.alpha, want_strength)
        return dx, dys, dyb, None, dstrength, None, None, None


class AdaINBwdFn(Function):
    """(dx, dstrength, dys, dyb) of AdaINFn from gy: three launches, four with dstrength (want_strength = False under
    input_grads_only: its reduction is not launched and None is returned).  Not differentiable."""

    @staticmethod
    def forward(ctx, gy, x, ys, noise, strength, mean, rstd, act, alpha, want_strength):
        ctx.set_materialize_grads(False)
        return K.adain_bwd(_c(gy), x, ys, mean, rstd, noise, strength, act, alpha, want_strength)

    @staticmethod
    def backward(ctx, *v):
        raise NotImplementedError('adain: a second differentiation is not implemented - the layer belongs to the generator, which no '
                                  'gradient penalty differentiates (the penalty is a gradient of the critic with respect to images); '
                                  'a critic that needs a twice-differentiable norm has layer_norm and pixel_norm')


_MODCONV_SECOND = ('%s: a second differentiation is not implemented - the layer belongs to the generator, which no '
                   'gradient penalty differentiates (the penalty is a gradient of the critic with respect to images); '
                   'a critic that needs a twice-differentiable norm has layer_norm and pixel_norm')


class _FirstOrder(Function):
    """The backward piece of a weight-demodulated convolution's functions: runs `fn(*args)` (tensors and plain values), not differentiable."""

    @staticmethod
    def forward(ctx, op, fn, *args):
        ctx.op = op
        ctx.set_materialize_grads(False)
        return fn(*args)

    @staticmethod
    def backward(ctx, *v):
        raise NotImplementedError(_MODCONV_SECOND % ctx.op)


class ModulateFn(Function):
    """xs[b,h,w,c] = x[b,h,w,c] s[b,c]: the per-sample channel scale in front of a weight-demodulated convolution (Karras et al. 2020; not
    in the reference).  Saves x and s.  dx is the same launch on the cotangent; ds [B,C] = sum over (h, w) of g x,
    two launches.  First order, like AdaINFn."""

    @staticmethod
    def forward(ctx, x, s):
        x = _c(x)
        ctx.save_for_backward(x, s)
        ctx.set_materialize_grads(False)
        return K.modulate(x, s)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        x, s = ctx.saved_tensors
        need = ctx.needs_input_grad

        def piece(g, x, s):
            g = _c(g)
            return (K.modulate(g, s) if need[0] else None), (K.modulate_bwd_scale(g, x) if need[1] else None)
        return _FirstOrder.apply('modulate', piece, g, x, s)


class DemodCoefFn(Function):
    """d[b,o] = rsqrt(sum_i s[b,i]^2 q[i,o] + eps), q[i,o] = the sum over the taps of w[.,.,i,o]^2: the demodulation coefficients of a
    modulated filter w [kh,kw,Cin,Cout] under the style scales s [B,Cin].  Two launches; saves w, s, q and d.
    Backward: ds (one launch) and dw (one launch; not under input_grads_only).  In the final backward dw goes straight into the
    weight's gradient-arena slot, which the convolution's filter gradient shares: added, or stored when it is the slot's first
    contribution of the step, on the filter-gradient stream when there is one (the slot's contributions keep their order)."""

    @staticmethod
    def forward(ctx, w, s, eps):
        d, q = K.demod_coef(w, s, eps)
        ctx.save_for_backward(w, s, q, d)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(q)
        return d, q

    @staticmethod
    def backward(ctx, gd, _gq):
        if gd is None:
            return None, None, None
        w, s, q, d = ctx.saved_tensors
        want_w = ctx.needs_input_grad[0] and not _INPUTS_ONLY[0]
        want_s = ctx.needs_input_grad[1]
        sink = _sink_of(w) if want_w else None

        def piece(gd, d, w, s, q):
            gd = _c(gd)
            if sink is None:
                return K.demod_coef_bwd(gd, d, w, s, q, want_s, want_w)
            ds = K.demod_coef_bwd(gd, d, w, s, q, want_s, False)[0]
            acc = sink_accumulate(w.data_ptr())
            sunk_launch(lambda: K.demod_coef_bwd(gd, d, w, s, q, False, True, out=sink, accumulate=acc), (gd, d, w, s, q))
            _notify(w)
            return ds, None
        ds, dw = _FirstOrder.apply('modulated_conv2d', piece, gd, d, w, s, q)
        return dw, ds, None


class DemodActFn(Function):
    """out = act(d[b,o] c + bias[o] + strength[o] noise[b,h,w]): the epilogue behind a weight-demodulated convolution's plain convolution
    c; d, bias and the noise pair are each optional.  One launch.  Saves c, d, bias, noise and strength: the
    backward recomputes the pre-activation, no plane of it or of a mask is kept.  Backward: dc and, unless under input_grads_only, dbias
    and dstrength, with dd in one or two launches; noise gets no gradient.  First order, like AdaINFn."""

    @staticmethod
    def forward(ctx, c, d, bias, noise, strength, act, alpha):
        c = _c(c)
        ctx.save_for_backward(c, d, bias, noise, strength)
        ctx.act, ctx.alpha = act, alpha
        ctx.set_materialize_grads(False)
        return K.demod_act(c, d, bias, noise, strength, act, alpha)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 7
        c, d, bias, noise, strength = ctx.saved_tensors
        need, params = ctx.needs_input_grad, not _INPUTS_ONLY[0]
        want = (d is not None and need[1], bias is not None and need[2] and params, strength is not None and need[4] and params)
        act, alpha = ctx.act, ctx.alpha

        def piece(g, c, d, bias, noise, strength):
            return K.demod_act_bwd(_c(g), c, d, bias, noise, strength, act, alpha, *want)
        dc, dd, dbias, dstrength = _FirstOrder.apply('modulated_conv2d', piece, g, c, d, bias, noise, strength)
        return dc, dd, dbias, None, dstrength, None, None


# ---- the same three functions, differentiable twice (path-length regularisation) ----------------------------------
# ops.modulated_conv2d(second_order=True) uses the subclasses below: the forward and the first-order backward are the parents' launches
# (the values are theirs bit for bit); under create_graph the backward is a Function whose own backward is csrc/t2i_modconv.hip's second-order
# entry points.  In a final backward (no graph is being recorded) the parents' backward runs as it is, arena sinks included.
_MODCONV_THIRD = ('%s: a third differentiation is not implemented - second_order=True makes the layer differentiable twice (the path-length '
                  'regulariser is the gradient of a gradient norm), and nothing in the package differentiates it again')
_MODCONV_PARAM = ('%s: a cotangent for the gradient of %s is the gradient of a parameter gradient, which is not implemented (layer_norm '
                  'refuses it likewise) - take the first backward under autograd.input_grads_only(), which does not form it')


class _SecondOrder(Function):
    """The second-order piece of a weight-demodulated convolution's functions: runs `fn(*args)`, not differentiable again."""

    @staticmethod
    def forward(ctx, op, fn, *args):
        ctx.op = op
        ctx.set_materialize_grads(False)
        return fn(*args)

    @staticmethod
    def backward(ctx, *v):
        raise NotImplementedError(_MODCONV_THIRD % ctx.op)


class ModulateBwdFn(Function):
    """(dx, ds) of ModulateFn from g: dx = g s, ds = sum over (h, w) of g x (the launches of ModulateFn.backward).  Backward, for the
    cotangents vx and vs: to g, s vx + x vs (one launch, t2i_modulate2); to x, g vs (t2i_modulate); to s, sum over (h, w) of vx g
    (t2i_modulate_bwd_scale)."""

    @staticmethod
    def forward(ctx, g, x, s, want_x, want_s):
        g = _c(g)
        ctx.save_for_backward(g, x, s)
        ctx.set_materialize_grads(False)
        return (K.modulate(g, s) if want_x else None), (K.modulate_bwd_scale(g, x) if want_s else None)

    @staticmethod
    def backward(ctx, vx, vs):
        if vx is None and vs is None:
            return (None,) * 5
        g, x, s = ctx.saved_tensors
        need = ctx.needs_input_grad

        def piece(g, x, s, vx, vs):
            vx, vs = (None if v is None else _c(v) for v in (vx, vs))
            return (K.modulate2(s, vx, x, vs) if need[0] else None, K.modulate(g, vs) if (need[1] and vs is not None) else None,
                    K.modulate_bwd_scale(vx, g) if (need[2] and vx is not None) else None)
        return _SecondOrder.apply('modulated_conv2d', piece, g, x, s, vx, vs) + (None, None)


class ModulateFn2(ModulateFn):
    """ModulateFn, differentiable twice."""

    @staticmethod
    def backward(ctx, g):
        if g is None or not torch.is_grad_enabled():
            return ModulateFn.backward(ctx, g)
        x, s = ctx.saved_tensors
        return ModulateBwdFn.apply(g, x, s, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


class DemodCoefBwdFn(Function):
    """(ds, dw) of DemodCoefFn from gd (the launches of DemodCoefFn.backward).  Backward, for the cotangent vs of ds, with
    e = -d^3 gd / 2 and r = sum_i vs s q: to gd, -d^3 r and to d, -3 d^2 gd r (one launch); to s, 2 vs sum_o q e (t2i_demod_coef_bwd with vs
    in place of s); to w, 4 w sum_b vs s e (one launch; into the weight's gradient-arena slot in a final backward, like dw).  d is
    DemodCoefFn's output, so its cotangent runs DemodCoefFn's backward once more.  A cotangent for dw is refused."""

    @staticmethod
    def forward(ctx, gd, d, w, s, q, want_s, want_w):
        gd = _c(gd)
        ctx.save_for_backward(gd, d, w, s, q)
        ctx.set_materialize_grads(False)
        return K.demod_coef_bwd(gd, d, w, s, q, want_s, want_w)

    @staticmethod
    def backward(ctx, vs, vdw):
        if vdw is not None:
            raise NotImplementedError(_MODCONV_PARAM % ('modulated_conv2d', 'weights'))
        if vs is None:
            return (None,) * 7
        gd, d, w, s, q = ctx.saved_tensors
        need = ctx.needs_input_grad
        want_w = need[2] and not _INPUTS_ONLY[0]
        sink = _sink_of(w) if want_w else None

        def piece(gd, d, w, s, q, vs):
            vs = _c(vs)
            gs = K.demod_coef_bwd(gd, d, w, vs, q, True, False)[0] if need[3] else None
            if sink is None:
                return K.demod_coef_bwd2(vs, gd, d, w, s, q, need[0], need[1], want_w) + (gs,)
            ggd, gdd, _ = K.demod_coef_bwd2(vs, gd, d, w, s, q, need[0], need[1], False)
            acc = sink_accumulate(w.data_ptr())
            sunk_launch(lambda: K.demod_coef_bwd2(vs, gd, d, w, s, q, False, False, True, out=sink, accumulate=acc), (vs, gd, d, w, s, q))
            _notify(w)
            return ggd, gdd, None, gs
        ggd, gdd, gw, gs = _SecondOrder.apply('modulated_conv2d', piece, gd, d, w, s, q, vs)
        return ggd, gdd, gw, gs, None, None, None


class DemodCoefFn2(DemodCoefFn):
    """DemodCoefFn, differentiable twice."""

    @staticmethod
    def backward(ctx, gd, _gq):
        if gd is None or not torch.is_grad_enabled():
            return DemodCoefFn.backward(ctx, gd, _gq)
        w, s, q, d = ctx.saved_tensors
        want_w = ctx.needs_input_grad[0] and not _INPUTS_ONLY[0]
        ds, dw = DemodCoefBwdFn.apply(gd, d, w, s, q, ctx.needs_input_grad[1], want_w)
        return dw, ds, None


class DemodActBwdFn(Function):
    """(dc, dd, dbias, dstrength) of DemodActFn from g (the launch pair of DemodActFn.backward).  Backward, for the cotangents vc of dc and
    vd of dd, with m = act'(the recomputed pre-activation): to g, m (d vc + c vd); to c, m g vd; to d, sum over (h, w) of m g vc - one
    launch, two with the last (t2i_demod_act_bwd2).  bias, strength and noise get nothing: act'' is zero almost everywhere.  A cotangent
    for dbias or dstrength is refused."""

    @staticmethod
    def forward(ctx, g, c, d, bias, noise, strength, act, alpha, want):
        g = _c(g)
        ctx.save_for_backward(g, c, d, bias, noise, strength)
        ctx.act, ctx.alpha = act, alpha
        ctx.set_materialize_grads(False)
        return K.demod_act_bwd(g, c, d, bias, noise, strength, act, alpha, *want)

    @staticmethod
    def backward(ctx, vc, vd, vbias, vstrength):
        for v, name in ((vbias, 'biases'), (vstrength, 'noise_strength')):
            if v is not None:
                raise NotImplementedError(_MODCONV_PARAM % ('modulated_conv2d', name))
        if vc is None and vd is None:
            return (None,) * 9
        g, c, d, bias, noise, strength = ctx.saved_tensors
        need, act, alpha = ctx.needs_input_grad, ctx.act, ctx.alpha

        def piece(g, c, d, bias, noise, strength, vc, vd):
            vc, vd = (None if v is None else _c(v) for v in (vc, vd))
            return K.demod_act_bwd2(g, c, d, bias, noise, strength, vc, vd, act, alpha, need[0], need[1], d is not None and need[2])
        gg, gc, gd = _SecondOrder.apply('modulated_conv2d', piece, g, c, d, bias, noise, strength, vc, vd)
        return gg, gc, gd, None, None, None, None, None, None


class DemodActFn2(DemodActFn):
    """DemodActFn, differentiable twice."""

    @staticmethod
    def backward(ctx, g):
        if g is None or not torch.is_grad_enabled():
            return DemodActFn.backward(ctx, g)
        c, d, bias, noise, strength = ctx.saved_tensors
        need, params = ctx.needs_input_grad, not _INPUTS_ONLY[0]
        want = (d is not None and need[1], bias is not None and need[2] and params, strength is not None and need[4] and params)
        dc, dd, dbias, dstrength = DemodActBwdFn.apply(g, c, d, bias, noise, strength, ctx.act, ctx.alpha, want)
        return dc, dd, dbias, None, dstrength, None, None
