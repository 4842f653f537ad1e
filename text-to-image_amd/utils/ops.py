"""The reference's operator surface (reference utils/ops.py:1-148), eager and MI355X-native.

Same names, parameters, defaults and error behaviour as the reference wrappers; below them sit libt2i_hip.so kernels
instead of tf.contrib.layers.  Differences that follow from "eager torch instead of a TF-1 graph":
  * parameters are created/looked up in a TF-style variable scope (``scope.py``) with TF's automatic names
    (``Conv``, ``Conv_1``, ``Conv2d_transpose``, ``dense``, ``BatchNorm``), so ``reuse=True`` and
    ``trainable_variables('d_net')`` mean what they mean in the reference (models/wgancls/model.py:59-60,134,167);
  * ``act`` is an ``Activation`` (``lrelu_act(0.2)``, ``relu``, ``tanh``) which the conv / BN epilogues fuse; any other
    callable is applied after the op, unfused;
  * data is physically NHWC always.  ``df=NCHW`` tensors are *logical* NCHW views (a permute of NHWC storage), so
    ``to_nchw`` / ``to_nhwc`` cost nothing and the result is layout-independent (SURVEY.md §7 last bullet).
north_star's ``deconv2d / linear / bn`` do not exist in the reference; they are exported as aliases.
Every public name of the reference's utils/ops.py exists here with its signature and defaults.  What remains different:
  * ``pixel_norm``, ``resize_nearest_neighbor``, ``upscale`` (s != 2), ``downscale``, ``pool`` (anything but the 2x2 average on even
    extents), ``gn`` and ``batch_renorm`` take fp32 tensors only: a bf16 tensor (bf16 storage) is refused with ValueError and a
    stacked pass (``stacked.Stacked``) with NotImplementedError, both before any launch and naming the operator;
  * ``batch_renorm`` and ``gn`` restate TF 1.4 as read from its sources; like the rest of the oracle they are not pinned against TF.
``layer_norm``, ``pixel_norm`` and ``minibatch_stddev`` (not in the reference: the PGGAN paper's critic layer) are differentiable twice
(what a critic under the gradient penalty needs),
like ``pool``, ``resize_nearest_neighbor``, ``gn``, ``lerp``, ``add`` and the convolutions; ``batch_norm`` / ``batch_renorm`` are first order.
``diff_augment`` / ``diff_augment_params`` (not in the reference either: the differentiable augmentation of Zhao et al. 2020, DESIGN.md
section 4.35) take fp32 tensors only, with the same refusals, and are differentiable to any order.  ``DiffAugmentSampler`` (DESIGN.md section
4.39) draws those tables on the device with a probability ``p`` per transform and can steer ``p`` from a critic's outputs.
``adain`` / ``style_block`` (not in the reference: the layer of a style-based generator) take fp32 tensors only,
with the same refusals, and are first order: the generator is never under the gradient penalty.
``modulated_conv2d`` (not in the reference: the weight-demodulated convolution of Karras et al. 2020) likewise.
"""
import math
import struct

import torch

from .. import autograd as A
from .. import kernels as K
from .. import scope as S
from .. import stacked as ST

NHWC = 'NHWC'
NCHW = 'NCHW'


class Activation(object):
    """A fusable activation (what the reference passes as a python callable: tf.nn.relu, a leaky_relu lambda, tf.nn.tanh)."""

    def __init__(self, kind, alpha=0.0):
        self.kind, self.alpha = kind, float(alpha)

    def __call__(self, x):
        shape = x.shape
        return A.ActFn.apply(x.contiguous(), self.kind, self.alpha).view(shape)

    def __repr__(self):
        return 'Activation(%s, %g)' % ({K.ACT_LRELU: 'lrelu', K.ACT_RELU: 'relu', K.ACT_TANH: 'tanh'}[self.kind], self.alpha)


relu = Activation(K.ACT_RELU)
tanh = Activation(K.ACT_TANH)


def lrelu_act(alpha=0.2):
    """reference utils/ops.py:90-91"""
    return Activation(K.ACT_LRELU, alpha)


def _split_act(act):
    """-> (fused kind, alpha, post-callable)"""
    if act is None:
        return K.ACT_NONE, 0.0, None
    if isinstance(act, Activation):
        return act.kind, act.alpha, None
    if callable(act):
        return K.ACT_NONE, 0.0, act
    raise TypeError('act must be None, an ops.Activation or a callable')


def _check_df(df):
    if df not in (NHWC, NCHW):
        raise ValueError('Invalid data format %s' % df)


def _phys(x, df):
    """logical tensor -> physically-NHWC 4-D tensor"""
    _check_df(df)
    if x.dim() != 4:
        raise ValueError('expected a rank-4 tensor, got shape %s' % (tuple(x.shape),))
    return x.permute(0, 2, 3, 1) if df == NCHW else x


def _logical(y, df):
    return y.permute(0, 3, 1, 2) if df == NCHW else y


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def conv2d(x, f, ks=(4, 4), s=(2, 2), padding='SAME', act=None, init=None, name=None, df=NHWC, stats=False):
    """reference utils/ops.py:58-63.  Variables: <scope>/Conv[_k]/{weights [kh,kw,Cin,f] (He), biases [f] (zeros)}.
    stats=True (not in the reference; a hint, results are unchanged): a batch_norm consumes this output next, so the GEMM
    epilogue also emits the per-tile column sums the normalisation needs and batch_norm skips its own pass over the tensor."""
    st = S.default_store()
    xp = _phys(x, df)
    B, H, W, Cin = xp.shape
    (kh, kw), (sh, sw) = _pair(ks), _pair(s)
    kind, alpha, post = _split_act(act)
    with st.variable_scope(name or st.unique_op_name('Conv'), reuse=st.reuse()):
        w = st.get_variable('weights', (kh, kw, Cin, f), init or S.he_init(kh * kw * Cin))
        b = st.get_variable('biases', (f,), S.constant_init(0.0))
    geom = K.conv_desc(B, H, W, Cin, f, kh, kw, sh, sw, padding)
    if isinstance(xp, ST.Stacked):        # a stacked pass (stacked.py): one launch for both parts
        y = ST.conv2d(xp, w, b, geom, kind, alpha, bool(stats) and kind == K.ACT_NONE and post is None)
    else:
        y = A.Conv2dFn.apply(xp, w, b, geom, kind, alpha, bool(stats) and kind == K.ACT_NONE and post is None)
    y = _logical(y, df)
    return post(y) if post else y


def conv2d_transpose(x, f, ks=(4, 4), s=(2, 2), padding='SAME', act=None, init=None, name=None, df=NHWC):
    """reference utils/ops.py:66-71.  Variables: <scope>/Conv2d_transpose[_k]/{weights [kh,kw,f,Cin], biases [f]}.
    He fan_in follows TF's variance_scaling on that layout: kh*kw*shape[-2] = kh*kw*f."""
    st = S.default_store()
    xp = _phys(x, df)
    B, H, W, Cin = xp.shape
    (kh, kw), (sh, sw) = _pair(ks), _pair(s)
    kind, alpha, post = _split_act(act)
    with st.variable_scope(name or st.unique_op_name('Conv2d_transpose'), reuse=st.reuse()):
        w = st.get_variable('weights', (kh, kw, f, Cin), init or S.he_init(kh * kw * f))
        b = st.get_variable('biases', (f,), S.constant_init(0.0))
    geom = K.deconv_desc(B, H, W, Cin, f, kh, kw, sh, sw, padding)
    if isinstance(xp, ST.Stacked):
        y = ST.conv2d_transpose(xp, w, b, geom, kind, alpha)
    else:
        y = A.ConvBwdDataFn.apply(xp, w, b, geom, kind, alpha)
    y = _logical(y, df)
    return post(y) if post else y


def fc(x, units, act=None, init=None, bias=True, name=None):
    """reference utils/ops.py:84-87 (tf.layers.dense).  Variables: <scope>/dense[_k]/{kernel [in,units], bias [units]}.
    Runs as a 1x1 convolution on a [B,1,1,in] view (the same MFMA GEMM kernel)."""
    st = S.default_store()
    if x.dim() != 2:
        raise ValueError('fc expects a rank-2 tensor, got shape %s' % (tuple(x.shape),))
    B, I = x.shape
    kind, alpha, post = _split_act(act)
    with st.variable_scope(name or st.unique_op_name('dense'), reuse=st.reuse()):
        w = st.get_variable('kernel', (I, units), init or S.he_init(I))
        b = st.get_variable('bias', (units,), S.constant_init(0.0)) if bias else None
    geom = K.conv_desc(B, 1, 1, I, units, 1, 1, 1, 1, 'VALID')
    if isinstance(x, ST.Stacked):
        Bm, Bh = x.main.shape[0], x.hat.shape[0]
        y = ST.conv2d(ST.Stacked(x.main.reshape(Bm, 1, 1, I), x.hat.reshape(Bh, 1, 1, I)), w.view(1, 1, I, units), b, geom, kind, alpha)
        y = ST.Stacked(y.main.view(Bm, units), y.hat.view(Bh, units))
    else:
        y = A.Conv2dFn.apply(x.reshape(B, 1, 1, I), w.view(1, 1, I, units), b, geom, kind, alpha).view(B, units)
    return post(y) if post else y


# TF collects the moving-average assignments of batch_norm in GraphKeys.UPDATE_OPS and runs them only under ops that
# depend on them (reference models/wgancls/model.py:98,102: G_optim yes, D_optim no).  Eager equivalent: the moving
# statistics are updated by the BN kernel itself iff the caller is inside `update_ops()`.
_UPDATE_OPS = [False]          # False, or how many times the moving averages take each batch norm's statistics (True == 1)


class update_ops(object):
    """times = 2: one evaluation stands for two identical evaluations of the reference graph, each of which would run the update op
    (models/gancls/trainer.py: the generator in the D run and in the G run of one iteration)."""

    def __init__(self, times=1):
        self.times = int(times)

    def __enter__(self):
        self.prev = _UPDATE_OPS[0]
        _UPDATE_OPS[0] = self.times

    def __exit__(self, *a):
        _UPDATE_OPS[0] = self.prev


def batch_norm(x, train, init=None, act=None, name=None, eps=1e-5, decay=0.9, df=NHWC, groups=1, fused_infer=False, residual=None, res_act=None):
    """reference utils/ops.py:7-29 (tf.contrib.layers.batch_norm, fused, scale=True).  Rank-4 (per channel) or rank-2
    (per feature).  Variables: <scope>/BatchNorm[_k]/{beta, gamma, moving_mean, moving_variance}.
    groups > 1 (not in the reference; training mode): x is a batched pass whose `groups` equal slices along the batch axis are separate
    passes of the reference graph — each slice is normalised with its own batch statistics (autograd.BatchNormTrainGroupedFn).
    fused_infer (not in the reference; inference only, no gradient): the whole norm is ONE launch (kernels.bn_infer: scale / shift are formed
    in the kernel), and with `residual` (a tensor of x's shape) the result is res_act(residual + act(norm(x))) — a residual block's closing
    add(residual, ·, res_act) in the same launch."""
    st = S.default_store()
    _check_df(df)
    if fused_infer and (train or groups > 1):
        raise ValueError('fused_infer is the inference path: train must be False and groups 1')
    if residual is not None and not fused_infer:
        raise ValueError('residual needs fused_infer=True')
    if x.dim() == 4:
        xp = _phys(x, df)
    elif x.dim() == 2:
        xp = x
    else:
        raise ValueError('batch_norm expects rank 2 or 4, got shape %s' % (tuple(x.shape),))
    C = xp.shape[-1]
    kind, alpha, post = _split_act(act)
    init = init or {}
    with st.variable_scope(name or st.unique_op_name('BatchNorm'), reuse=st.reuse()):
        beta = st.get_variable('beta', (C,), init.get('beta', S.constant_init(0.0)))
        gamma = st.get_variable('gamma', (C,), init.get('gamma', S.constant_init(1.0)))
        mm = st.get_variable('moving_mean', (C,), S.constant_init(0.0), trainable=False)
        mv = st.get_variable('moving_variance', (C,), S.constant_init(1.0), trainable=False)
    if train and isinstance(xp, ST.Stacked):
        # two evaluations of the reference graph stacked along the batch axis (the generator pair): per-part statistics; only the leading
        # part — the evaluation that runs under UPDATE_OPS — moves the moving averages
        total = int(groups) if groups > 1 else 2          # groups = 1: each part is one evaluation (the paired generator)
        upd = _UPDATE_OPS[0]
        if not ST.batch_norm_ok(xp, total):
            raise NotImplementedError('stacked batch norm needs C % 4 == 0, whole evaluations per part and 16-byte aligned evaluations')
        y = ST.batch_norm(xp, gamma, beta, mm if upd else None, mv if upd else None, eps, decay, kind, alpha, max(int(upd), 1), total)
    elif train and groups > 1:
        upd = _UPDATE_OPS[0]
        if int(upd) > 1:
            raise NotImplementedError('update_ops(times > 1) with a stacked batch')
        y = A.BatchNormTrainGroupedFn.apply(xp, gamma, beta, mm if upd else None, mv if upd else None, eps, decay, kind, alpha, int(groups))
    elif train:
        upd = _UPDATE_OPS[0]
        y, _, _ = A.BatchNormTrainFn.apply(xp, gamma, beta, mm if upd else None, mv if upd else None, eps, decay, kind, alpha, max(int(upd), 1))
    elif fused_infer:
        if isinstance(xp, ST.Stacked) or post is not None:
            raise NotImplementedError('fused_infer takes a plain tensor and a fusable activation')
        rkind, ralpha, rpost = _split_act(res_act)
        if rpost is not None:
            raise NotImplementedError('fused_infer: res_act must be None or an ops.Activation')
        res = None
        if residual is not None:
            res = (_phys(residual, df) if x.dim() == 4 else residual).detach().contiguous()
        y = K.bn_infer(xp.detach().contiguous(), gamma.detach(), beta.detach(), mm, mv, eps, kind, alpha, res, rkind, ralpha)
    else:
        # inference: y = act(x*scale + shift) with the moving statistics; [C]-sized host-side vector math
        with torch.no_grad():
            scale = gamma / torch.sqrt(mv + eps)
            shift = beta - mm * scale
        y = K.bn_apply(xp.contiguous(), scale.contiguous(), shift.contiguous(), kind, alpha)
    if x.dim() == 4:
        y = _logical(y, df)
    return post(y) if post else y


RENORM_DECAY = 0.99          # tf.contrib.layers.batch_norm's renorm_decay default, which the reference leaves alone


def batch_renorm(x, train, init=None, act=None, name=None, eps=1e-5, decay=0.9, df=NHWC):
    """reference utils/ops.py:32-55 (tf.contrib.layers.batch_norm(renorm=True), renorm_clipping=None, renorm_decay=0.99; TF takes
    its non-fused path).  Rank 4 or rank 2, fp32, no groups / fused_infer / stacked passes.  Variables: <scope>/BatchNorm[_k]/{beta,
    gamma, moving_mean, moving_variance} as batch_norm, and the non-trainable renorm_mean [C], renorm_stddev [C], renorm_mean_weight (),
    renorm_stddev_weight (), all starting at zero as in TF 1.4 (the zero-debiased averages need that: renorm_stddev / weight is the
    running sigma, and the first step has r = 1, d = 0).
    Training: mu, sigma = sqrt(biased variance + eps) of the batch; mixed = renorm + (1 - weight) * batch value; r = sigma / mixed_std,
    d = (mu - mixed_mean) / mixed_std, both from the variables as they are before this call and constants for the gradient;
    y = act(((x - mu) / sigma * r + d) * gamma + beta).  Inside update_ops() (times times): renorm <- renorm * 0.99 + value * 0.01,
    weight <- weight * 0.99 + 0.01 for mean and stddev, and the moving statistics move with `decay` towards renorm_mean / weight
    and (renorm_stddev / weight)^2 - eps.  Inference is batch_norm's.  Restated from TF 1.4's sources; not pinned against TF."""
    st = S.default_store()
    _check_df(df)
    _fp32_plain(x, 'batch_renorm', rank=None)
    if x.dim() == 4:
        xp = _phys(x, df)
    elif x.dim() == 2:
        xp = x
    else:
        raise ValueError('batch_renorm expects rank 2 or 4, got shape %s' % (tuple(x.shape),))
    C = xp.shape[-1]
    kind, alpha, post = _split_act(act)
    init = init or {}
    with st.variable_scope(name or st.unique_op_name('BatchNorm'), reuse=st.reuse()):
        beta = st.get_variable('beta', (C,), init.get('beta', S.constant_init(0.0)))
        gamma = st.get_variable('gamma', (C,), init.get('gamma', S.constant_init(1.0)))
        mm = st.get_variable('moving_mean', (C,), S.constant_init(0.0), trainable=False)
        mv = st.get_variable('moving_variance', (C,), S.constant_init(1.0), trainable=False)
        rm = st.get_variable('renorm_mean', (C,), S.constant_init(0.0), trainable=False)
        rmw = st.get_variable('renorm_mean_weight', (), S.constant_init(0.0), trainable=False)
        rs = st.get_variable('renorm_stddev', (C,), S.constant_init(0.0), trainable=False)
        rsw = st.get_variable('renorm_stddev_weight', (), S.constant_init(0.0), trainable=False)
    if train:
        xc = xp.contiguous()
        rows = xc.numel() // C
        s0, m2 = K.bn_stats(xc)                      # sum, centred second moment: [C]-sized vector math from here on
        with torch.no_grad():
            mu = s0 / rows
            sigma = torch.sqrt(m2 / rows + eps)
            mixed_mean = rm + (1.0 - rmw) * mu
            mixed_std = rs + (1.0 - rsw) * sigma
            r = sigma / mixed_std
            d = (mu - mixed_mean) / mixed_std
            rstd = 1.0 / sigma
            for _ in range(0 if K.is_dry() else int(_UPDATE_OPS[0])):       # (a dry pass holds no values)
                rm.mul_(RENORM_DECAY).add_(mu, alpha=1.0 - RENORM_DECAY)
                rmw.mul_(RENORM_DECAY).add_(1.0 - RENORM_DECAY)
                rs.mul_(RENORM_DECAY).add_(sigma, alpha=1.0 - RENORM_DECAY)
                rsw.mul_(RENORM_DECAY).add_(1.0 - RENORM_DECAY)
                new_std = rs / rsw
                mm.mul_(decay).add_(rm / rmw, alpha=1.0 - decay)
                mv.mul_(decay).add_(new_std * new_std - eps, alpha=1.0 - decay)
        y = A.BatchRenormTrainFn.apply(xc, gamma, beta, mu, rstd, r, d, kind, alpha)
    else:
        with torch.no_grad():
            scale = gamma / torch.sqrt(mv + eps)
            shift = beta - mm * scale
        y = K.bn_apply(xp.contiguous(), scale.contiguous(), shift.contiguous(), kind, alpha)
    if x.dim() == 4:
        y = _logical(y, df)
    return post(y) if post else y


def layer_norm(x, act=None, scope=None, df=NHWC):
    """reference utils/ops.py:74-81 (tf.contrib.layers.layer_norm, begin_params_axis = channel axis).  Rank-4 NHWC or
    rank-2.  Variables: <scope>/LayerNorm[_k]/{beta [C] zeros, gamma [C] ones}.  Differentiable twice with respect to its input
    (no activation, relu or lrelu; reaching the second order through a fused tanh raises NotImplementedError), so it may sit in a
    critic under the gradient penalty; under autograd.input_grads_only() the first-order pass returns no gamma / beta gradients."""
    st = S.default_store()
    _check_df(df)
    if x.dim() == 4:
        xp = _phys(x, df)
    elif x.dim() == 2:
        xp = x
    else:
        raise ValueError('layer_norm expects rank 2 or 4, got shape %s' % (tuple(x.shape),))
    C = xp.shape[-1]
    kind, alpha, post = _split_act(act)
    with st.variable_scope(scope or st.unique_op_name('LayerNorm'), reuse=st.reuse()):
        beta = st.get_variable('beta', (C,), S.constant_init(0.0))
        gamma = st.get_variable('gamma', (C,), S.constant_init(1.0))
    y = A.LayerNormFn.apply(xp, gamma, beta, 1e-12, kind, alpha)
    if x.dim() == 4:
        y = _logical(y, df)
    return post(y) if post else y


def _fp32_plain(x, op, rank=4):
    """The refusals shared by the operators of csrc/t2i_ops.hip, all before any launch."""
    if isinstance(x, ST.Stacked):
        raise NotImplementedError('%s: a stacked pass (stacked.Stacked) is not supported' % op)
    if x.dtype != torch.float32:
        raise ValueError('%s: expected a float32 tensor, got %s (bf16 storage is not supported here)' % (op, x.dtype))
    if rank is not None and x.dim() != rank:
        raise ValueError('%s: expected a rank-%d tensor, got shape %s' % (op, rank, tuple(x.shape)))


def pixel_norm(x, eps=1e-8, act=None):
    """reference utils/ops.py:94-97: u = act(x), then u / sqrt(mean(u^2, axis=3) + eps) — the PGGAN paper's pixelwise feature
    normalisation.  Rank 4, normalised over axis 3 of the tensor as given, which must be contiguous (a logical NCHW view is not:
    pass to_nhwc(x)).  An ops.Activation is fused into the kernel; any other callable is applied first, unfused.  One launch forward,
    one backward, one for the backward of the backward: differentiable twice, so it may sit in a critic under the gradient penalty
    (no activation, relu or lrelu; reaching the second order through a fused tanh raises NotImplementedError).
    The backward reads the derivative of lrelu / relu from the sign of y (as every Activation's backward in this package does), which
    is the sign of x only for a slope >= 0: an lrelu_act with a negative slope is refused with ValueError."""
    _fp32_plain(x, 'pixel_norm')
    kind, alpha, pre = _split_act(act)
    if kind == K.ACT_LRELU and alpha < 0.0:
        raise ValueError('pixel_norm: lrelu_act(%g) has a negative slope; the backward takes the derivative from the sign of the output, '
                         'which needs a slope >= 0' % alpha)
    if pre is not None:
        x = pre(x)
        _fp32_plain(x, 'pixel_norm')
    if not x.is_contiguous():
        raise ValueError('pixel_norm normalises over the last axis of physically NHWC data; got a non-contiguous tensor (shape %s, strides %s) '
                         '- convert a logical NCHW view with to_nhwc first' % (tuple(x.shape), x.stride()))
    return A.PixelNormFn.apply(x, float(eps), kind, alpha)


def adain(x, ys, yb, noise=None, strength=None, act=None, eps=1e-8):
    """The layer epilogue of a style-based generator (Karras et al. 2019; not in the reference).  x [B,H,W,C]
    (contiguous NHWC, fp32), ys and yb [B,C], optionally noise [B,H,W] with strength [C] (both or neither):
      u = act(x + strength[c] * noise[b,h,w])         act: None, relu or lrelu_act(slope >= 0), fused
      mu, var = the biased moments of u over (h, w), per sample and channel (never E[u^2] - mu^2)
      y = (u - mu) / sqrt(var + eps) * (1 + ys[b,c]) + yb[b,c]
    Three launches forward; three backward, four with strength.  Gradients reach x, ys, yb and strength (not under
    autograd.input_grads_only()); noise gets none and must not require one.  First order only: a second differentiation raises
    NotImplementedError.  ys and yb may be the two halves of one [B,2C] tensor (no copy).  bf16 tensors, a stacked pass, another rank, a
    non-contiguous x or noise, wrong shapes, noise without strength or the reverse and a negative lrelu slope are refused before any
    launch.  A sample's result does not depend on its batch, bit for bit."""
    op = 'adain'
    _fp32_plain(x, op)
    kind, alpha, post = _split_act(act)
    if post is not None or kind == K.ACT_TANH:
        raise ValueError('%s: act must be None, relu or an lrelu_act (it is fused between the noise and the normalisation), got %r' % (op, act))
    if kind == K.ACT_LRELU and alpha < 0.0:
        raise ValueError('%s: lrelu_act(%g) has a negative slope; the backward takes the derivative from the sign, which needs a slope >= 0' % (op, alpha))
    if not x.is_contiguous():
        raise ValueError('%s works on physically NHWC data; got a non-contiguous tensor (shape %s, strides %s) - convert a logical NCHW '
                         'view with to_nhwc first' % (op, tuple(x.shape), x.stride()))
    B, H, W, C = (int(s) for s in x.shape)
    if min(B, H, W, C) < 1 or x.numel() >= 1 << 31:
        raise ValueError('%s: every size of x must be at least 1 and x must have fewer than 2^31 elements, got %s' % (op, tuple(x.shape)))
    for name, t in (('ys', ys), ('yb', yb)):
        if not isinstance(t, torch.Tensor) or isinstance(t, ST.Stacked) or t.dtype != torch.float32 or tuple(t.shape) != (B, C) or t.device != x.device:
            raise ValueError('%s: %s must be a float32 tensor of shape [%d, %d] on %s, got %s' % (
                op, name, B, C, x.device, '%s %s on %s' % (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t).__name__))
    if ys.stride(1) != 1 or yb.stride(1) != 1 or (B > 1 and (ys.stride(0) != yb.stride(0) or ys.stride(0) < C)):
        ys, yb = ys.contiguous(), yb.contiguous()
    if (noise is None) != (strength is None):
        raise ValueError('%s: noise and strength come together or not at all (got %s without %s)' % (
            (op, 'noise', 'strength') if strength is None else (op, 'strength', 'noise')))
    if noise is not None:
        for name, t, shape in (('noise', noise, (B, H, W)), ('strength', strength, (C,))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != x.device:
                raise ValueError('%s: %s must be a float32 tensor of shape %s on %s, got %s' % (
                    op, name, list(shape), x.device, '%s %s on %s' % (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t).__name__))
            if not t.is_contiguous():
                raise ValueError('%s: %s must be contiguous (strides %s)' % (op, name, t.stride()))
        if noise.requires_grad:
            raise ValueError('%s: noise requires a gradient, and the operator gives it none (detach it)' % op)
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError('%s: eps must be a finite number >= 0, got %r' % (op, eps))
    return A.AdaINFn.apply(x, ys, yb, noise, strength, kind, alpha, float(eps))


def style_block(x, w, noise=None, act=None, name=None, init=None):
    """The layer a style-based generator puts behind every convolution: x [B,H,W,C] is the convolution's output
    (bias included, no activation), w [B, w_dim] the style vector, noise [B,H,W] a standard-normal image or None.
    Variables: <scope>/StyleMod[_k]/{noise_strength [C] zeros (only with noise), style/kernel [w_dim, 2C], style/bias [2C] zeros}: the
    dense layer is `fc` with the caller's `init` (None: fc's He default), and its rank-2 `kernel` is what an equalized-learning-rate table
    selects.  Its output is split into ys | yb and handed to `adain` without a copy."""
    st = S.default_store()
    _fp32_plain(x, 'style_block')
    if w.dim() != 2 or w.shape[0] != x.shape[0]:
        raise ValueError('style_block: w must be [%d, w_dim], got shape %s' % (x.shape[0], tuple(w.shape)))
    C = int(x.shape[3])
    with st.variable_scope(name or st.unique_op_name('StyleMod'), reuse=st.reuse()):
        strength = st.get_variable('noise_strength', (C,), S.constant_init(0.0)) if noise is not None else None
        s = fc(w, 2 * C, init=init, name='style')
    return adain(x, s[:, :C], s[:, C:], noise=noise, strength=strength, act=act)


def modulated_conv2d(x, w, f, ks=(3, 3), noise=None, act=None, demodulate=True, init=None, style_init=None, name=None, eps=1e-8, second_order=False):
    """A weight-demodulated convolution (Karras et al. 2020; not in the reference): x [B,H,W,Cin] (contiguous NHWC,
    fp32), w [B, w_dim] the style vector, noise [B,H,W] a standard-normal image or None; stride 1, padding 'SAME'.
    Variables: <scope>/ModConv[_k]/{weights [kh,kw,Cin,f] (He, or init), biases [f] zeros, noise_strength [f] zeros (only with noise),
    style/kernel [w_dim,Cin] (fc's He default, or style_init), style/bias [Cin] zeros}.
      s = 1 + fc(w, Cin)                                         the per-sample scale of every input channel
      d[b,o] = rsqrt(sum_{kh,kw,i} (weights[.,.,i,o] s[b,i])^2 + eps)      (demodulate=False: 1)
      y = act(conv(x[b], weights s[b,:] d[b,:]) + biases + noise_strength[o] noise[b,h,w])
    computed as act(d conv(x s, weights) + ...), which is the same function: a scale pass over x, the project's convolution without bias
    or activation, one epilogue.  act: None, relu or lrelu_act(slope >= 0), fused.  Gradients reach x, w and every variable (the
    parameters' not under autograd.input_grads_only()); noise gets none.  First order only, unless second_order=True (DESIGN.md section
    4.46): then the same launches run forward and in the first backward, the values are the same bit for bit, and a gradient taken with
    create_graph=True under autograd.input_grads_only() can be differentiated once more to x, w and every variable (path-length
    regularisation); a cotangent for a parameter's gradient and a third differentiation are refused.  bf16 tensors, a stacked pass, another
    rank, a non-contiguous x or noise, wrong shapes, a negative lrelu slope, tanh and an unfused activation are refused before any launch."""
    op = 'modulated_conv2d'
    st = S.default_store()
    _fp32_plain(x, op)
    kind, alpha, post = _split_act(act)
    if post is not None or kind == K.ACT_TANH:
        raise ValueError('%s: act must be None, relu or an lrelu_act (it is fused into the epilogue behind the convolution), got %r' % (op, act))
    if kind == K.ACT_LRELU and alpha < 0.0:
        raise ValueError('%s: lrelu_act(%g) has a negative slope; the backward takes the derivative from the sign, which needs a slope >= 0' % (op, alpha))
    if not x.is_contiguous():
        raise ValueError('%s: x must be physically NHWC; got a non-contiguous tensor (shape %s, strides %s) - convert a logical NCHW '
                         'view with to_nhwc first' % (op, tuple(x.shape), x.stride()))
    B, H, W, Cin = (int(v) for v in x.shape)
    if min(B, H, W, Cin) < 1 or x.numel() >= 1 << 31:
        raise ValueError('%s: every size of x must be at least 1 and x must have fewer than 2^31 elements, got %s' % (op, tuple(x.shape)))
    if isinstance(w, ST.Stacked):
        raise NotImplementedError('%s: w is a stacked pass (stacked.Stacked), which is not supported' % op)
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 2 or w.shape[0] != B or w.shape[1] < 1 or w.device != x.device:
        raise ValueError('%s: w must be a float32 tensor of shape [%d, w_dim] on %s, got %s' % (
            op, B, x.device, '%s %s on %s' % (w.dtype, tuple(w.shape), w.device) if isinstance(w, torch.Tensor) else type(w).__name__))
    if isinstance(f, bool) or not isinstance(f, int) or f < 1:
        raise ValueError('%s: f must be an integer >= 1 (the output channels), got %r' % (op, f))
    kh, kw = _pair(ks)
    if kh < 1 or kw < 1:
        raise ValueError('%s: ks must be a pair of extents >= 1, got %r' % (op, ks))
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or tuple(noise.shape) != (B, H, W) or noise.device != x.device:
            raise ValueError('%s: noise must be a float32 tensor of shape %s on %s, got %s' % (
                op, [B, H, W], x.device, '%s %s on %s' % (noise.dtype, tuple(noise.shape), noise.device) if isinstance(noise, torch.Tensor)
                else type(noise).__name__))
        if not noise.is_contiguous():
            raise ValueError('%s: noise must be contiguous (strides %s)' % (op, noise.stride()))
        if noise.requires_grad:
            raise ValueError('%s: noise requires a gradient, and the operator gives it none (detach it)' % op)
    if not isinstance(demodulate, bool):
        raise ValueError('%s: demodulate must be True or False, got %r' % (op, demodulate))
    if not isinstance(second_order, bool):
        raise ValueError('%s: second_order must be True or False, got %r' % (op, second_order))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError('%s: eps must be a finite number >= 0, got %r' % (op, eps))
    with st.variable_scope(name or st.unique_op_name('ModConv'), reuse=st.reuse()):
        weights = st.get_variable('weights', (kh, kw, Cin, f), init or S.he_init(kh * kw * Cin))
        biases = st.get_variable('biases', (f,), S.constant_init(0.0))
        strength = st.get_variable('noise_strength', (f,), S.constant_init(0.0)) if noise is not None else None
        s = 1.0 + fc(w, Cin, init=style_init, name='style')
    geom = K.conv_desc(B, H, W, Cin, f, kh, kw, 1, 1, 'SAME')
    coef, scale, epilogue = (A.DemodCoefFn2, A.ModulateFn2, A.DemodActFn2) if second_order else (A.DemodCoefFn, A.ModulateFn, A.DemodActFn)
    d = coef.apply(weights, s, float(eps))[0] if demodulate else None
    c = A.Conv2dFn.apply(scale.apply(x, s), weights, None, geom, K.ACT_NONE, 0.0)
    return epilogue.apply(c, d, biases, noise, strength, kind, alpha)


def minibatch_stddev_stat(x, group_size=4, num_features=1, eps=1e-8):
    """The minibatch standard deviation of the progressive-growing paper's critic, as a statistic: x [B,H,W,C] (contiguous NHWC,
    fp32) -> [B, num_features].  Sample n belongs to group n // group_size — CONTIGUOUS rows (the paper's code strides the groups; for
    i.i.d. rows that is a permutation of this, and contiguous groups stay inside the B-row parts of a concatenated batch) —, channel c to
    chunk c // (C / num_features).  Per column (h, w, c): the biased standard deviation sqrt(var + eps) across the group's samples;
    row n, chunk f = its mean over the chunk's columns, the same in every row of a group.  group_size is taken as given: 1..16 and a
    divisor of B (the caller picks a divisor); num_features divides C.  Differentiable twice; results for a
    batch are bit for bit those of its groups taken separately."""
    op = 'minibatch_stddev'
    _fp32_plain(x, op)
    if int(group_size) != group_size or int(num_features) != num_features:
        raise ValueError('%s: group_size and num_features must be integers, got %r and %r' % (op, group_size, num_features))
    G, F = int(group_size), int(num_features)
    B, C = x.shape[0], x.shape[3]
    if G < 1 or G > 16:
        raise ValueError('%s: group_size must be in 1..16 (a thread keeps the group in registers), got %d' % (op, G))
    if B % G != 0:
        raise ValueError('%s: group_size %d does not divide the batch of %d' % (op, G, B))
    if F < 1 or C % F != 0:
        raise ValueError('%s: num_features %d does not divide the %d channels' % (op, F, C))
    if not float(eps) > 0.0:
        raise ValueError('%s: eps must be positive (the backward divides by sqrt(var + eps)), got %r' % (op, eps))
    if not x.is_contiguous():
        raise ValueError('%s works on physically NHWC data; got a non-contiguous tensor (shape %s, strides %s) - convert a logical NCHW '
                         'view with to_nhwc first' % (op, tuple(x.shape), x.stride()))
    return A.MinibatchStddevFn.apply(x, G, F, float(eps))


def minibatch_stddev(x, group_size=4, num_features=1, eps=1e-8):
    """x [B,H,W,C] -> [B,H,W,C + num_features]: minibatch_stddev_stat tiled over the map and appended as the last channels (concat_tile)."""
    return concat_tile(x, minibatch_stddev_stat(x, group_size, num_features, eps))


DIFFAUG_POLICIES = {'color': K.DIFFAUG_COLOR, 'translation': K.DIFFAUG_TRANSLATION, 'cutout': K.DIFFAUG_CUTOUT}


def diff_augment_policy(policy, op='diff_augment'):
    """'color,translation,cutout' or any non-empty subset, in any order -> the kernels' bit mask; anything else is a ValueError."""
    names = [p.strip() for p in policy.split(',')] if isinstance(policy, str) else None
    if not names or any(p not in DIFFAUG_POLICIES for p in names):
        raise ValueError("%s: policy must be a comma-separated, non-empty subset of 'color,translation,cutout', got %r" % (op, policy))
    mask = 0
    for p in names:
        mask |= DIFFAUG_POLICIES[p]
    return mask


def diff_augment(x, params, policy='color,translation,cutout'):
    """Differentiable augmentation (Zhao et al., NeurIPS 2020; not in the reference): x [B,H,W,C] (contiguous
    NHWC, fp32) -> T(x) of the same shape, sample n transformed by row n of `params` [B,9] = (b, s, c, ty, tx, y0, y1, x0, x1), a float32
    tensor on x's device (diff_augment_params draws one):
      color        u + b, then s u + (1 - s) * (the pixel's channel mean), then c u + (1 - c) * (the sample's mean)
      translation  shift by (ty, tx) pixels, zeros moving in
      cutout       zeros in rows [y0, y1) x columns [x0, x1)
    The columns of a policy that is not named are not read.  At most two launches (one without 'color'); differentiable in x to any
    order — the backward is the adjoint kernel, whose backward is the forward again — so it may sit in front of a critic under the
    gradient penalty.  No gradient flows to `params`.  A sample's result does not depend on the batch it sits in, bit for bit."""
    op = 'diff_augment'
    _fp32_plain(x, op)
    mask = diff_augment_policy(policy, op)
    if not x.is_contiguous():
        raise ValueError('%s works on physically NHWC data; got a non-contiguous tensor (shape %s, strides %s) - convert a logical NCHW '
                         'view with to_nhwc first' % (op, tuple(x.shape), x.stride()))
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or tuple(params.shape) != (x.shape[0], 9):
        raise ValueError('%s: params must be a float32 tensor of shape [%d, 9] (one row per sample), got %s' % (
            op, x.shape[0], '%s %s' % (params.dtype, tuple(params.shape)) if isinstance(params, torch.Tensor) else type(params).__name__))
    if params.device != x.device:
        raise ValueError('%s: params live on %s, x on %s' % (op, params.device, x.device))
    if not params.is_contiguous():
        raise ValueError('%s: params must be contiguous (strides %s)' % (op, params.stride()))
    return A.DiffAugmentFn.apply(x, params.detach(), mask, True)


def diff_augment_params(n, H, W, policy='color,translation,cutout', generator=None, out=None, device=None):
    """One table [n, 9] for diff_augment on H x W images, drawn with the publication's distributions: b ~ U(-0.5, 0.5), s ~ U(0, 2),
    c ~ U(0.5, 1.5); ty, tx uniform integers in [-r, r], r = int(size / 8 + 0.5); a cutout of extent int(size / 2 + 0.5) whose centre
    offset is a uniform integer in [0, size - extent mod 2], clipped to the image (never empty).  A policy that is not named gets its
    identity columns (b 0, s 1, c 1, no shift, an empty rectangle).  Plain tensor-library calls on `out`'s device (or `device`, or
    the generator's, else the CPU); with `out` ([n, 9] float32) the table is written in place — a captured graph's static buffer is
    redrawn this way."""
    op = 'diff_augment_params'
    mask = diff_augment_policy(policy, op)
    n, H, W = int(n), int(H), int(W)
    if n < 1 or H < 1 or W < 1:
        raise ValueError('%s: n, H and W must be positive, got %d, %d, %d' % (op, n, H, W))
    if out is None:
        dev = device if device is not None else (generator.device if generator is not None else 'cpu')
        out = torch.empty((n, 9), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, 9):
        raise ValueError('%s: out must be a float32 tensor of shape [%d, 9], got %s %s' % (op, n, out.dtype, tuple(out.shape)))
    dev = out.device
    with torch.no_grad():
        out.zero_()
        out[:, 1:3].fill_(1.0)
        if mask & K.DIFFAUG_COLOR:
            u = torch.rand((n, 3), generator=generator, device=dev, dtype=torch.float32)
            out[:, 0] = u[:, 0] - 0.5
            out[:, 1] = u[:, 1] * 2.0
            out[:, 2] = u[:, 2] + 0.5
        if mask & K.DIFFAUG_TRANSLATION:
            for col, size in ((3, H), (4, W)):
                r = int(size / 8.0 + 0.5)
                out[:, col] = torch.randint(-r, r + 1, (n,), generator=generator, device=dev).float()
        if mask & K.DIFFAUG_CUTOUT:
            for col, size in ((5, H), (7, W)):
                ext = int(size / 2.0 + 0.5)
                lo = torch.randint(0, size - ext % 2 + 1, (n,), generator=generator, device=dev) - ext // 2
                out[:, col] = lo.clamp(min=0).float()
                out[:, col + 1] = (lo + ext).clamp(max=size).float()
    return out


class DiffAugmentSampler(object):
    """The parameter tables of diff_augment drawn on the device, each transform applied to a row with probability p, and p optionally
    steered from the critic's outputs (Karras et al., "Training Generative Adversarial Networks with Limited Data", NeurIPS 2020;
    DESIGN.md section 4.39).  Owns the sixteen state words of include/t2i_hip.h (t2i_diffaug_state) on `device`: seed, call counter, p and
    the controller's accumulators.  draw() is one launch with no host work, so it may sit in a captured graph, and the table of call k is
    a pure function of (seed, k, row) — Philox4x32-10 — that tests restate in numpy bit for bit.
      adapt=None        p stays what it is; observe() does nothing
      adapt='logit'     the publication's r_t = E[sign(D(real))], for a critic with a logistic loss
      adapt='midpoint'  the same statistic against the midpoint of the batch means of D(real) and D(fake): this project's translation to a
                        Wasserstein critic, whose outputs have no fixed zero (not the publication's; no training run has judged it)
    Every `interval` observations p moves by (real logits seen) / ramp_images, up when the statistic exceeds `target` and down when it
    is below, clamped to [0, 1]; the defaults are the publication's."""
    ADAPT = {None: None, 'logit': K.ADA_LOGIT, 'midpoint': K.ADA_MIDPOINT}

    def __init__(self, policy, p=1.0, seed=0, device=None, adapt=None, target=0.6, interval=4, ramp_images=500000):
        op = 'DiffAugmentSampler'
        self.mask = diff_augment_policy(policy, op)
        self.policy = policy
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:            # (NaN fails both comparisons)
            raise ValueError('%s: p must be a probability in [0, 1], got %r' % (op, p))
        if isinstance(adapt, bool) or adapt not in self.ADAPT:
            raise ValueError("%s: adapt must be None, 'midpoint' or 'logit', got %r" % (op, adapt))
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError('%s: seed must be an integer in [0, 2^64), got %r' % (op, seed))
        if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
            raise ValueError('%s: interval must be an integer >= 1, got %r' % (op, interval))
        if isinstance(target, bool) or not isinstance(target, (int, float)) or not -1.0 < target < 1.0:
            raise ValueError('%s: target must lie in (-1, 1), got %r' % (op, target))
        if isinstance(ramp_images, bool) or not isinstance(ramp_images, (int, float)) or not (math.isfinite(ramp_images) and ramp_images > 0):
            raise ValueError('%s: ramp_images must be positive and finite, got %r' % (op, ramp_images))
        self.adapt, self.mode = adapt, self.ADAPT[adapt]
        self.target, self.interval, self.ramp_images = float(target), interval, float(ramp_images)
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        import numpy as np
        words = np.zeros(16, np.int64)
        words[0], words[1] = seed & 0xffffffff, seed >> 32
        words[4] = int(np.float32(p).view(np.uint32))
        self.state = torch.zeros(16, dtype=torch.int32, device=torch.device(device))
        self.device = self.state.device           # ('cuda' resolved to the current device's index: tensors are compared against it)
        self.load_state_dict(words)

    def draw(self, n, H, W, out=None):
        """The next table [n, 9] for H x W images (into `out`, a contiguous float32 [n, 9] on the state's device, when given); the call
        counter advances by one."""
        op = 'DiffAugmentSampler.draw'
        n, H, W = int(n), int(H), int(W)
        if not (1 <= n <= 65535 and 1 <= H <= 32768 and 1 <= W <= 32768):
            raise ValueError('%s: need 1 <= n <= 65535 and 1 <= H, W <= 32768, got %d, %d, %d' % (op, n, H, W))
        if out is None:
            out = torch.empty((n, 9), dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n, 9) or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError('%s: out must be a contiguous float32 tensor of shape [%d, 9] on %s, got %s' % (
                op, n, self.device, '%s %s on %s' % (out.dtype, tuple(out.shape), out.device) if isinstance(out, torch.Tensor) else type(out).__name__))
        return K.diff_augment_draw(self.state, out, H, W, self.mask)

    def _logits(self, d, name):
        op = 'DiffAugmentSampler.observe'
        if (not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or d.dim() != 1 or not d.is_contiguous() or d.device != self.device
                or not 1 <= d.shape[0] <= 65535):
            raise ValueError('%s: %s must be a contiguous float32 vector of 1..65535 logits on %s, got %s' % (
                op, name, self.device, '%s %s on %s' % (d.dtype, tuple(d.shape), d.device) if isinstance(d, torch.Tensor) else type(d).__name__))
        return d.detach()

    def observe(self, d_real, d_fake=None):
        """One batch of critic outputs for the controller (nothing when adapt is None): d_real, and under 'midpoint' d_fake of the same
        length.  One launch; p changes on every `interval`-th call."""
        if self.mode is None:
            return
        d_real = self._logits(d_real, 'd_real')
        if d_fake is not None or self.mode == K.ADA_MIDPOINT:
            if d_fake is None:
                raise ValueError("DiffAugmentSampler.observe: adapt='midpoint' needs d_fake")
            d_fake = self._logits(d_fake, 'd_fake')
            if d_fake.shape != d_real.shape:
                raise ValueError('DiffAugmentSampler.observe: d_fake has %d logits, d_real %d' % (d_fake.shape[0], d_real.shape[0]))
        K.diffaug_observe(self.state, d_real, d_fake, self.mode, self.target, self.interval, self.ramp_images)

    def p_tensor(self):
        """p as a float32 device scalar that aliases the state: no launch, no synchronisation"""
        return self.state[4:5].view(torch.float32)[0]

    def _word(self, i, as_float):
        w = self.state[i:i + 1]
        return float(w.view(torch.float32).cpu()[0]) if as_float else int(w.cpu()[0]) & 0xffffffff

    @property
    def p(self):
        return self._word(4, True)

    @property
    def last_r(self):
        return self._word(8, True)

    @property
    def updates(self):
        return self._word(9, False)

    @property
    def counter(self):
        return self._word(2, False) | (self._word(3, False) << 32)

    def state_dict(self):
        """The sixteen words as an int64 array of values in [0, 2^32): any checkpoint format holds them."""
        return self.state.cpu().numpy().view('uint32').astype('int64')

    def load_state_dict(self, words):
        import numpy as np
        words = np.asarray(words)
        if words.shape != (16,) or words.dtype.kind not in 'iu' or bool(((words < 0) | (words > 0xffffffff)).any()):
            raise ValueError('DiffAugmentSampler.load_state_dict: expected 16 integer words in [0, 2^32), got %s %s' % (words.dtype, words.shape))
        with torch.no_grad():
            self.state.copy_(torch.from_numpy(words.astype(np.uint32).view(np.int32).copy()))


def pool(x, s=2, p_type='AVG', df=NHWC):
    """reference utils/ops.py:100-101 (tf.nn.pool, window = stride = s, SAME): any integer s >= 1, 'AVG' or 'MAX', any extents.
    The output extent is ceil(H / s); the padding is split with the smaller half in front; AVG divides by the number of taps inside
    the image and MAX ignores the padding.  Differentiable to any order.  pool(x, 2) on even extents — all the reference's models
    use — is the 2x2 kernel pair Pool2Fn / Upscale2Fn as before."""
    if p_type not in ('AVG', 'MAX'):
        raise ValueError("pool: p_type must be 'AVG' or 'MAX', got %r" % (p_type,))
    if int(s) != s or s < 1:
        raise ValueError('pool: s must be an integer >= 1, got %r' % (s,))
    s = int(s)
    _check_df(df)
    xp = _phys(x, df)
    if s == 2 and p_type == 'AVG' and xp.shape[1] % 2 == 0 and xp.shape[2] % 2 == 0:
        return _logical(A.Pool2Fn.apply(xp, 0.25), df)
    _fp32_plain(xp, 'pool')
    # From s = max(H, W) on, one window holds the whole map and the padding only grows, so the result no longer depends on s: clamp it
    # (the kernels bound s).  MAX offsets are then ky * s + kx in the CLAMPED window's coordinates; that is consistent because the
    # clamped s is the one PoolMaxFn keeps in ctx, and every consumer of the offsets (PoolMaxPutFn, PoolMaxTakeFn) gets s from there.
    s = min(s, max(int(xp.shape[1]), int(xp.shape[2]), 1))
    y = A.PoolAvgFn.apply(xp, s) if p_type == 'AVG' else A.PoolMaxFn.apply(xp, s)
    return _logical(y, df)


def resize_nearest_neighbor(x, new_size):
    """reference utils/ops.py:104-106 (tf.image.resize_nearest_neighbor, align_corners=False), NHWC: output row r reads source row
    min(int(floor(r * scale)), H - 1) with scale = float32(H) / float32(H_out), columns alike.  A gather kernel whose adjoint is a
    gather too: differentiable to any order."""
    _fp32_plain(x, 'resize_nearest_neighbor')
    Ho, Wo = int(new_size[0]), int(new_size[1])
    if Ho < 1 or Wo < 1:
        raise ValueError('resize_nearest_neighbor: empty output %dx%d' % (Ho, Wo))
    return A.ResizeNearestFn.apply(x, Ho, Wo)


def upscale(x, s=2):
    """reference utils/ops.py:109-111: nearest-neighbour resize to (h*s, w*s), NHWC, any integer s >= 1."""
    if int(s) != s or s < 1:
        raise ValueError('upscale: s must be an integer >= 1, got %r' % (s,))
    if s == 2:
        return A.Upscale2Fn.apply(x, 1.0)
    _fp32_plain(x, 'upscale')
    return A.ResizeNearestFn.apply(x, int(x.shape[1]) * int(s), int(x.shape[2]) * int(s))


def _fir_taps(f, scale, op):
    """The taps of a resampling filter as float32-exact Python floats: f * scale, refused unless 1..8 finite numbers."""
    try:
        f = [float(t) for t in f]
    except (TypeError, ValueError):
        raise ValueError('%s: the filter must be a sequence of numbers, got %r' % (op, f))
    if not 1 <= len(f) <= K.UPFIRDN_MAX_TAPS:
        raise ValueError('%s: the filter has %d taps, 1..%d are supported' % (op, len(f), K.UPFIRDN_MAX_TAPS))
    taps = tuple(_f32(t * scale) for t in f)
    if not all(math.isfinite(t) for t in taps):
        raise ValueError('%s: the taps must be finite in float32, got %r (times %r)' % (op, f, scale))
    return taps


def _f32(v):
    """v rounded to float32, as a Python float (inf where it overflows)"""
    try:
        return struct.unpack('f', struct.pack('f', v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


def upfirdn2d(x, f, up=1, down=1, pad=(0, 0), flip=False, gain=1.0):
    """Anti-aliased resampling (not in the reference: the `upfirdn2d` of Karras et al. 2019).  x [B,H,W,C]
    (contiguous NHWC, fp32) -> [B,Ho,Wo,C]; along H and along W alike: insert up - 1 zeros after every sample, pad by pad[0] in front
    and pad[1] behind (a negative pad crops), convolve with the taps f (a sequence of 1..8 numbers, used on both axes, reversed first
    when flip; true convolution), keep every down-th sample: Ho = (H up + pad[0] + pad[1] - len(f)) // down + 1.  gain scales the result;
    it is folded into the taps as sqrt(gain) per axis (gain >= 0).  up and down are 1 or 2: other factors are refused, as are bf16
    tensors, a stacked pass, non-finite taps, pads beyond 32768 in magnitude, an empty output and tensors of 2^31 elements or more,
    all with ValueError (NotImplementedError for the stacked pass) before any launch.  One launch of csrc/t2i_resample.hip; the taps
    are host values (no gradient flows to them) and travel as kernel arguments, so the call can be captured.  Differentiable in x to any
    order: the backward is the same kernel with the adjoint's parameters.  A sample's result does not depend on its batch, bit for bit."""
    op = 'upfirdn2d'
    _fp32_plain(x, op)
    if not x.is_contiguous():
        raise ValueError('%s works on physically NHWC data; got a non-contiguous tensor (shape %s, strides %s) - convert a logical NCHW '
                         'view with to_nhwc first' % (op, tuple(x.shape), x.stride()))
    for label, v in (('up', up), ('down', down)):
        if isinstance(v, bool) or not isinstance(v, int) or v not in (1, 2):
            raise ValueError('%s: %s must be 1 or 2, got %r' % (op, label, v))
    if not isinstance(pad, (tuple, list)) or len(pad) != 2 or any(isinstance(p, bool) or not isinstance(p, int) for p in pad):
        raise ValueError('%s: pad must be a pair of integers (front, back), got %r' % (op, pad))
    if isinstance(gain, bool) or not isinstance(gain, (int, float)) or not (math.isfinite(gain) and gain >= 0.0):
        raise ValueError('%s: gain must be a finite number >= 0, got %r' % (op, gain))
    taps = _fir_taps(f, math.sqrt(float(gain)), op)
    p0, p1 = int(pad[0]), int(pad[1])
    if max(abs(p0), abs(p1)) > K.UPFIRDN_MAX_PAD:
        raise ValueError('%s: pads %r exceed %d in magnitude' % (op, tuple(pad), K.UPFIRDN_MAX_PAD))
    B, H, W, C = (int(s) for s in x.shape)
    if min(B, H, W, C) < 1:
        raise ValueError('%s: every size of x must be at least 1, got %s' % (op, tuple(x.shape)))
    Ho, Wo = K.upfirdn2d_extent(H, up, down, p0, p1, len(taps)), K.upfirdn2d_extent(W, up, down, p0, p1, len(taps))
    if Ho < 1 or Wo < 1:
        raise ValueError('%s: a %dx%d map with up %d, down %d, pads %r and %d taps has no output' % (op, H, W, up, down, tuple(pad), len(taps)))
    if x.numel() >= 1 << 31 or B * Ho * Wo * C >= 1 << 31:
        raise ValueError('%s: x %s or the output %s has 2^31 elements or more' % (op, tuple(x.shape), (B, Ho, Wo, C)))
    return A.UpFirDn2dFn.apply(x, taps, up, down, p0, (p1, p1), bool(flip))


def _resample_helper(x, k, factor, gain, op, up):
    if isinstance(factor, bool) or not isinstance(factor, int) or factor not in (1, 2):
        raise ValueError('%s: factor must be 1 or 2, got %r' % (op, factor))
    try:
        total = math.fsum(float(t) for t in k)
    except (TypeError, ValueError):
        raise ValueError('%s: the filter must be a sequence of numbers, got %r' % (op, k))
    if not (math.isfinite(total) and total != 0.0):
        raise ValueError('%s: the taps %r must have a finite, non-zero sum (they are normalised by it)' % (op, k))
    n = len(k)
    p = n - factor
    scale = (factor if up else 1.0) / total                      # per axis: DC gain 1 after the zero insertion
    k = _fir_taps(k, scale, op)
    if up:
        return upfirdn2d(x, k, up=factor, pad=((p + 1) // 2 + factor - 1, p // 2), gain=gain)
    return upfirdn2d(x, k, down=factor, pad=((p + 1) // 2, p // 2), gain=gain)


def upsample_2d(x, k=(1, 3, 3, 1), factor=2, gain=1.0):
    """Low-pass filtered upsampling (Karras et al. 2019, `upsample_2d`; not in the reference): upfirdn2d with up = factor, the taps
    factor * k / sum(k) per axis (DC gain 1) and the publication's pads ((p + 1) // 2 + factor - 1, p // 2), p = len(k) - factor:
    [B,H,W,C] -> [B,factor H,factor W,C].  k = (1, 1) is the nearest-neighbour `upscale(x, 2)` exactly.  factor is 1 or 2 (others are
    refused), fp32 only (bf16 is refused); the other refusals, the launch and the derivatives are upfirdn2d's."""
    return _resample_helper(x, k, factor, gain, 'upsample_2d', True)


def downsample_2d(x, k=(1, 3, 3, 1), factor=2, gain=1.0):
    """Low-pass filtered downsampling (Karras et al. 2019, `downsample_2d`; Zhang 2019's blur pool; not in the reference): upfirdn2d
    with down = factor, the taps k / sum(k) per axis (DC gain 1) and the publication's pads ((p + 1) // 2, p // 2), p = len(k) - factor:
    [B,H,W,C] -> [B,H / factor,W / factor,C] on even extents.  k = (1, 1) is the 2x2 mean `pool(x, 2)` to rounding.  factor is 1 or 2
    (others are refused), fp32 only (bf16 is refused); the other refusals, the launch and the derivatives are upfirdn2d's."""
    return _resample_helper(x, k, factor, gain, 'downsample_2d', False)


def downscale(x, s=2):
    """reference utils/ops.py:114-116: nearest-neighbour resize to (h // s, w // s), NHWC."""
    if int(s) != s or s < 1:
        raise ValueError('downscale: s must be an integer >= 1, got %r' % (s,))
    _fp32_plain(x, 'downscale')
    Ho, Wo = int(x.shape[1]) // int(s), int(x.shape[2]) // int(s)
    if Ho < 1 or Wo < 1:
        raise ValueError('downscale: a %dx%d map scaled down by %d is empty' % (x.shape[1], x.shape[2], s))
    return A.ResizeNearestFn.apply(x, Ho, Wo)


def gn(x, mag):
    """reference utils/ops.py:145-148: x * m^n with m = 1 + 0.2 * max(0, mag - 0.5)^2 and n ~ N(0, 1) drawn per element (the
    multiplicative critic noise of the PGGAN paper).  mag is a Python float or a 0-d tensor that is READ ON THE HOST: no gradient
    flows to mag.  One launch; the draw is keyed by — and advances — the device's torch generator (torch.cuda.manual_seed makes it
    reproducible).  mag <= 0.5 returns x bit for bit.  Differentiable in x to any order.  Raises RuntimeError under graph capture:
    the host-side seed and offset would be baked into the graph and every replay would draw the same noise."""
    _fp32_plain(x, 'gn', rank=None)
    if x.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('gn: cannot be captured into a graph (its Philox seed and offset are host values: every replay would repeat the noise)')
    mag = float(mag.item()) if isinstance(mag, torch.Tensor) else float(mag)
    m = 1.0 + 0.2 * max(0.0, mag - 0.5) ** 2
    return A.GnFn.apply(x, math.log(m))


def lerp(a, b, t):
    """(1 - t)*a + t*b with a host scalar t: the fade-in of a new resolution (tf.multiply / tf.add on the `alpha_tra`
    variable, reference models/pggan/pggan.py:267,314)."""
    if isinstance(t, torch.Tensor):          # weight in device memory: the step can be captured into a hipGraph
        return A.LerpDevFn.apply(a, b, t, 0)
    return A.AxpbyFn.apply(a, 1.0 - float(t), b, float(t))


def to_nchw(x):
    """reference utils/ops.py:129-130.  Logical transpose only: storage stays NHWC."""
    return x.permute(0, 3, 1, 2)


def to_nhwc(x):
    """reference utils/ops.py:133-134"""
    return x.permute(0, 2, 3, 1)


def reshape_to_map(x, C, H, W, df=NHWC):
    """tf.reshape of a rank-2 activation to a feature map (reference models/wgancls/model.py:178-181).  With df=NCHW
    feature index = c*H*W + h*W + w, so the storage is re-tiled to NHWC by one transpose kernel and returned as a
    logical-NCHW view; with df=NHWC the reshape is free."""
    _check_df(df)
    B = x.shape[0]
    if isinstance(x, ST.Stacked):
        if df == NHWC:
            return x.reshape_parts(H, W, C)
        return ST.nchw_to_nhwc(x.reshape_parts(C, H, W)).permute(0, 3, 1, 2)
    if df == NHWC:
        return x.reshape(B, H, W, C)
    return A.NchwToNhwcFn.apply(x.reshape(B, C, H, W)).permute(0, 3, 1, 2)


def add(a, b, act=None, df=NHWC):
    """tf.add followed by an activation (the residual joins, reference models/wgancls/model.py:145-146,190-191)."""
    kind, alpha, post = _split_act(act)
    if isinstance(a, ST.Stacked):
        y = _logical(ST.add_act(_phys(a, df), _phys(b, df), kind, alpha), df)
    elif a.dim() == 4:
        y = _logical(A.AddActFn.apply(_phys(a, df), _phys(b, df), kind, alpha), df)
    else:
        y = A.AddActFn.apply(a, b, kind, alpha)
    return post(y) if post else y


def fork(x, df=NHWC):
    """-> (x, x) for a tensor with two consumers.  Plain tensors: the tensor itself twice (autograd sums the two gradients).  A stacked
    pass (stacked.py): two aliases whose incoming stacked gradients are summed by one launch on the whole buffer."""
    if not isinstance(x, ST.Stacked):
        return x, x
    a, b = ST.fork(_phys(x, df))
    return _logical(a, df), _logical(b, df)


def concat_tile(feat, emb, df=NHWC):
    """expand_dims x2 -> tile over the spatial map -> concat on channels (reference models/wgancls/model.py:153-155)."""
    if isinstance(feat, ST.Stacked):
        return _logical(ST.concat_tile(_phys(feat, df), emb), df)
    return _logical(A.ConcatTileFn.apply(_phys(feat, df), emb), df)


def get_conv_shape(tensor):
    return get_ints_from_shape(tensor)


def get_ints_from_shape(tensor):
    return [int(n) for n in tensor.shape]


def df_to_channel(df):
    """reference utils/ops.py:137-142"""
    if df == NHWC:
        return 'channels_last'
    if df == NCHW:
        return 'channels_first'
    raise RuntimeError('Invalid data format %s' % df)


# aliases named by BASELINE.json:north_star
deconv2d = conv2d_transpose
linear = fc
bn = batch_norm
