"""InceptionV3 inference for the evaluator — the role of reference models/inception/model.py (`load_inception_inference`:
slim `inception_v3(images, num_classes, is_training=False)` restored from the latest checkpoint of INCEP_CHECKPOINT_DIR).

Input [B, 299, 299, 3] float32 in [-1, 1]; output (logits [B, num_classes], PreLogits [B, 2048]).  PreLogits is
`AvgPool_1a_8x8` (dropout is the identity at eval), the logits are the 1x1 `Logits/Conv2d_1c_1x1` with bias and no
activation.  Every other convolution is slim's conv2d + batch_norm(center=True, scale=False, epsilon=0.001) + ReLU, run as
one t2i_conv2d_fwd with the batch norm folded into weights and bias at load time (float64, then cast) and ReLU in the
epilogue.  Pooling, branch concatenation and the head are the evaluator kernels (t2i_eval.hip).  There is no
torch.nn.functional anywhere on this path.

The network is written once (`_inception_v3`) over an `ops` object: `_Spec` traces shapes only (the layer table, parameter
count and multiply-adds), `_Run` executes on the device.  Checkpoints follow utils/saver.py: a `checkpoint` file naming
`<prefix>-<step>.npz`, arrays keyed by slim's TF names (`InceptionV3/Mixed_5b/Branch_1/Conv2d_0b_5x5/weights`, HWIO, and
`.../BatchNorm/{beta, moving_mean, moving_variance}`); other keys (AuxLogits, optimizer slots) are ignored, a missing key
is an error that names it."""
import collections

import numpy as np
import torch

from ... import kernels as K

SCOPE = 'InceptionV3'
BN_EPS = 0.001
IMAGE_SIZE = 299
PRELOGITS_DIM = 2048


def _inception_v3(ops, x, num_classes):
    """slim inception_v3_base (final_endpoint Mixed_7c) + the logits head.  ops.conv(x, name, kh, kw, cout, stride, padding),
    ops.pool(x, name, k, stride, padding, op), ops.concat(parts) where a part is a tensor or ops.pool_into(x, k, stride,
    padding, op) (a pooling branch written straight into the concatenation)."""
    MAX, AVG = K.POOL_MAX, K.POOL_AVG
    c, p = ops.conv, ops.pool
    # stem: VALID unless noted
    x = c(x, 'Conv2d_1a_3x3', 3, 3, 32, 2, 'VALID')
    x = c(x, 'Conv2d_2a_3x3', 3, 3, 32, 1, 'VALID')
    x = c(x, 'Conv2d_2b_3x3', 3, 3, 64, 1, 'SAME')
    x = p(x, 'MaxPool_3a_3x3', 3, 2, 'VALID', MAX)
    x = c(x, 'Conv2d_3b_1x1', 1, 1, 80, 1, 'VALID')
    x = c(x, 'Conv2d_4a_3x3', 3, 3, 192, 1, 'VALID')
    x = p(x, 'MaxPool_5a_3x3', 3, 2, 'VALID', MAX)                    # 35 x 35 x 192
    # 35 x 35 blocks
    for blk, pool_c, b1 in (('Mixed_5b', 32, ('Conv2d_0a_1x1', 'Conv2d_0b_5x5')),
                            ('Mixed_5c', 64, ('Conv2d_0b_1x1', 'Conv_1_0c_5x5')),
                            ('Mixed_5d', 64, ('Conv2d_0a_1x1', 'Conv2d_0b_5x5'))):
        n = lambda br, conv: '%s/%s/%s' % (blk, br, conv)            # noqa: E731
        b0 = c(x, n('Branch_0', 'Conv2d_0a_1x1'), 1, 1, 64)
        t = c(x, n('Branch_1', b1[0]), 1, 1, 48)
        bb1 = c(t, n('Branch_1', b1[1]), 5, 5, 64)
        t = c(x, n('Branch_2', 'Conv2d_0a_1x1'), 1, 1, 64)
        t = c(t, n('Branch_2', 'Conv2d_0b_3x3'), 3, 3, 96)
        bb2 = c(t, n('Branch_2', 'Conv2d_0c_3x3'), 3, 3, 96)
        t = p(x, n('Branch_3', 'AvgPool_0a_3x3'), 3, 1, 'SAME', AVG)
        bb3 = c(t, n('Branch_3', 'Conv2d_0b_1x1'), 1, 1, pool_c)
        x = ops.concat([b0, bb1, bb2, bb3])                          # 256 / 288 / 288
    # Mixed_6a -> 17 x 17 x 768
    b0 = c(x, 'Mixed_6a/Branch_0/Conv2d_1a_1x1', 3, 3, 384, 2, 'VALID')
    t = c(x, 'Mixed_6a/Branch_1/Conv2d_0a_1x1', 1, 1, 64)
    t = c(t, 'Mixed_6a/Branch_1/Conv2d_0b_3x3', 3, 3, 96)
    bb1 = c(t, 'Mixed_6a/Branch_1/Conv2d_1a_1x1', 3, 3, 96, 2, 'VALID')
    x = ops.concat([b0, bb1, ops.pool_into(x, 'Mixed_6a/Branch_2/MaxPool_1a_3x3', 3, 2, 'VALID', MAX)])
    # 17 x 17 blocks
    for blk, w in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
        n = lambda br, conv: '%s/%s/%s' % (blk, br, conv)            # noqa: E731
        b0 = c(x, n('Branch_0', 'Conv2d_0a_1x1'), 1, 1, 192)
        t = c(x, n('Branch_1', 'Conv2d_0a_1x1'), 1, 1, w)
        t = c(t, n('Branch_1', 'Conv2d_0b_1x7'), 1, 7, w)
        bb1 = c(t, n('Branch_1', 'Conv2d_0c_7x1'), 7, 1, 192)
        t = c(x, n('Branch_2', 'Conv2d_0a_1x1'), 1, 1, w)
        t = c(t, n('Branch_2', 'Conv2d_0b_7x1'), 7, 1, w)
        t = c(t, n('Branch_2', 'Conv2d_0c_1x7'), 1, 7, w)
        t = c(t, n('Branch_2', 'Conv2d_0d_7x1'), 7, 1, w)
        bb2 = c(t, n('Branch_2', 'Conv2d_0e_1x7'), 1, 7, 192)
        t = p(x, n('Branch_3', 'AvgPool_0a_3x3'), 3, 1, 'SAME', AVG)
        bb3 = c(t, n('Branch_3', 'Conv2d_0b_1x1'), 1, 1, 192)
        x = ops.concat([b0, bb1, bb2, bb3])                          # 768
    # Mixed_7a -> 8 x 8 x 1280
    t = c(x, 'Mixed_7a/Branch_0/Conv2d_0a_1x1', 1, 1, 192)
    b0 = c(t, 'Mixed_7a/Branch_0/Conv2d_1a_3x3', 3, 3, 320, 2, 'VALID')
    t = c(x, 'Mixed_7a/Branch_1/Conv2d_0a_1x1', 1, 1, 192)
    t = c(t, 'Mixed_7a/Branch_1/Conv2d_0b_1x7', 1, 7, 192)
    t = c(t, 'Mixed_7a/Branch_1/Conv2d_0c_7x1', 7, 1, 192)
    bb1 = c(t, 'Mixed_7a/Branch_1/Conv2d_1a_3x3', 3, 3, 192, 2, 'VALID')
    x = ops.concat([b0, bb1, ops.pool_into(x, 'Mixed_7a/Branch_2/MaxPool_1a_3x3', 3, 2, 'VALID', MAX)])
    # 8 x 8 blocks; the nested concatenations of branches 1 and 2 flatten into the block's channel order
    for blk, b1b in (('Mixed_7b', 'Conv2d_0b_3x1'), ('Mixed_7c', 'Conv2d_0c_3x1')):
        n = lambda br, conv: '%s/%s/%s' % (blk, br, conv)            # noqa: E731
        b0 = c(x, n('Branch_0', 'Conv2d_0a_1x1'), 1, 1, 320)
        t = c(x, n('Branch_1', 'Conv2d_0a_1x1'), 1, 1, 384)
        b1a = c(t, n('Branch_1', 'Conv2d_0b_1x3'), 1, 3, 384)
        b1b_ = c(t, n('Branch_1', b1b), 3, 1, 384)
        t = c(x, n('Branch_2', 'Conv2d_0a_1x1'), 1, 1, 448)
        t = c(t, n('Branch_2', 'Conv2d_0b_3x3'), 3, 3, 384)
        b2a = c(t, n('Branch_2', 'Conv2d_0c_1x3'), 1, 3, 384)
        b2b = c(t, n('Branch_2', 'Conv2d_0d_3x1'), 3, 1, 384)
        t = p(x, n('Branch_3', 'AvgPool_0a_3x3'), 3, 1, 'SAME', AVG)
        bb3 = c(t, n('Branch_3', 'Conv2d_0b_1x1'), 1, 1, 192)
        x = ops.concat([b0, b1a, b1b_, b2a, b2b, bb3])               # 2048
    # head: PreLogits = AvgPool_1a_8x8 (VALID), logits = 1x1 conv with bias, no activation
    pre = p(x, 'Logits/AvgPool_1a_8x8', 8, 2, 'VALID', AVG)
    logits = ops.conv(pre, 'Logits/Conv2d_1c_1x1', 1, 1, num_classes, 1, 'VALID', bn=False)
    return logits, pre


class _Spec(object):
    """Shape-only trace: records every convolution (name, KH, KW, Cin, Cout, stride, padding, Ho, Wo, batch-normed) and every
    pooling window, with tensors stood in for by their shape tuples (B, H, W, C)."""

    def __init__(self):
        self.convs = collections.OrderedDict()
        self.pools = []

    def conv(self, x, name, kh, kw, cout, stride=1, padding='SAME', bn=True):
        B, H, W, cin = x
        Ho, Wo = K.pool_out_size(H, kh, stride, padding), K.pool_out_size(W, kw, stride, padding)
        if name in self.convs:
            raise ValueError('duplicate layer %s' % name)
        self.convs[name] = (kh, kw, cin, cout, stride, padding, Ho, Wo, bn)
        return (B, Ho, Wo, cout)

    def pool(self, x, name, k, stride, padding, op):
        B, H, W, C = x
        self.pools.append((name, k, stride, padding, op, H, W, C))
        return (B, K.pool_out_size(H, k, stride, padding), K.pool_out_size(W, k, stride, padding), C)

    def pool_into(self, x, name, k, stride, padding, op):
        return self.pool(x, name, k, stride, padding, op)

    def concat(self, parts):
        assert len(set(p[:3] for p in parts)) == 1, parts
        return parts[0][:3] + (sum(p[3] for p in parts),)


def layer_table(num_classes=20):
    """-> OrderedDict name (under InceptionV3/) -> (KH, KW, Cin, Cout, stride, padding, Ho, Wo, batch-normed), execution order."""
    spec = _Spec()
    _inception_v3(spec, (1, IMAGE_SIZE, IMAGE_SIZE, 3), num_classes)
    return spec.convs


def variable_shapes(num_classes=20):
    """Checkpoint keys this model reads and their shapes."""
    out = collections.OrderedDict()
    for name, (kh, kw, cin, cout, _, _, _, _, bn) in layer_table(num_classes).items():
        base = '%s/%s/' % (SCOPE, name)
        out[base + 'weights'] = (kh, kw, cin, cout)
        if bn:
            for v in ('beta', 'moving_mean', 'moving_variance'):
                out[base + 'BatchNorm/' + v] = (cout,)
        else:
            out[base + 'biases'] = (cout,)
    return out


def multiply_adds(num_classes=20):
    """Multiply-adds of one image's forward convolutions (padded taps included, as the conv kernels compute them)."""
    return sum(Ho * Wo * kh * kw * cin * cout for kh, kw, cin, cout, _, _, Ho, Wo, _ in layer_table(num_classes).values())


def fold_batch_norm(w, beta, mean, var, eps=BN_EPS):
    """conv + batch_norm(center, no scale) -> (weights, bias) float32: w / sqrt(var + eps), beta - mean / sqrt(var + eps), in
    float64."""
    r = 1.0 / np.sqrt(np.asarray(var, np.float64) + eps)
    return ((np.asarray(w, np.float64) * r).astype(np.float32),
            (np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * r).astype(np.float32))


class _Run(object):
    """Device execution of the network: folded convs through t2i_conv2d_fwd, pooling / concatenation through t2i_eval.hip.
    `timer(kind)` (optional) is called before each launch with 'conv' or 'other' (tools/bench_inception.py)."""

    def __init__(self, params, timer=None):
        self.params, self.timer = params, timer

    def _tick(self, kind):
        if self.timer is not None:
            self.timer(kind)

    def conv(self, x, name, kh, kw, cout, stride=1, padding='SAME', bn=True):
        w, b = self.params[name]
        B, H, W, cin = x.shape
        d, ws = K.conv_desc(B, H, W, cin, cout, kh, kw, stride, stride, padding, math=K.MATH_F32)
        self._tick('conv')
        return K.conv_fwd(x, w, b, d, ws, act=K.ACT_RELU if bn else K.ACT_NONE, out_dtype=torch.float32)

    def pool(self, x, name, k, stride, padding, op):
        self._tick('other')
        return K.pool2d(x, k, k, stride, stride, padding, op)

    def pool_into(self, x, name, k, stride, padding, op):
        return ('pool', x, k, stride, padding, op)

    def concat(self, parts):
        def chans(p):
            return p[1].shape[3] if isinstance(p, tuple) else p.shape[3]
        first = parts[0]
        B, H, W = first.shape[:3]
        out = torch.empty((B, H, W, sum(chans(p) for p in parts)), dtype=torch.float32, device=first.device)
        c0 = 0
        for p in parts:
            self._tick('other')
            if isinstance(p, tuple):
                _, x, k, s, pad, op = p
                K.pool2d(x, k, k, s, s, pad, op, out=out, c0=c0)
            else:
                K.channel_slice_copy(p, out, c0)
            c0 += chans(p)
        return out


class InceptionV3(object):
    """params: name -> (folded weights [KH,KW,Cin,Cout] float32, bias [Cout] float32) on the device."""

    def __init__(self, params, num_classes=20):
        self.params, self.num_classes = params, num_classes

    @classmethod
    def from_arrays(cls, arrays, num_classes=20, device=None, source='checkpoint'):
        """arrays: mapping of TF names to arrays (a checkpoint's contents); BN is folded here."""
        device = device or torch.device('cuda', torch.cuda.current_device())
        shapes = variable_shapes(num_classes)
        for key, shape in shapes.items():
            if key not in arrays:
                raise KeyError('%s has no variable %s' % (source, key))
            if tuple(np.shape(arrays[key])) != shape:
                raise ValueError('%s: %s has shape %s, the model needs %s' % (source, key, np.shape(arrays[key]), shape))
        params = {}
        for name, spec in layer_table(num_classes).items():
            base = '%s/%s/' % (SCOPE, name)
            if spec[-1]:
                w, b = fold_batch_norm(arrays[base + 'weights'], arrays[base + 'BatchNorm/beta'],
                                       arrays[base + 'BatchNorm/moving_mean'], arrays[base + 'BatchNorm/moving_variance'])
            else:
                w, b = np.asarray(arrays[base + 'weights'], np.float32), np.asarray(arrays[base + 'biases'], np.float32)
            params[name] = (torch.from_numpy(np.ascontiguousarray(w)).to(device), torch.from_numpy(np.ascontiguousarray(b)).to(device))
        K.filter_cache_invalidate()
        return cls(params, num_classes)

    def forward(self, images, timer=None):
        """images float32 [B, 299, 299, 3] in [-1, 1] (device) -> (logits [B, num_classes], PreLogits [B, 2048])."""
        if images.dtype != torch.float32 or images.dim() != 4 or tuple(images.shape[1:]) != (IMAGE_SIZE, IMAGE_SIZE, 3):
            raise ValueError('InceptionV3 takes float32 [B, 299, 299, 3], got %s %s' % (images.dtype, tuple(images.shape)))
        with torch.no_grad():
            logits, pre = _inception_v3(_Run(self.params, timer), images.contiguous(), self.num_classes)
        B = images.shape[0]
        return logits.reshape(B, self.num_classes), pre.reshape(B, PRELOGITS_DIM)

    __call__ = forward


def load_inception_inference(num_classes, checkpoint_dir, device=None):
    """reference models/inception/model.py load_inception_inference: the network restored from the latest checkpoint of
    checkpoint_dir (utils/saver.py's `checkpoint` file + npz).  Unlike the reference, a failed load is an error."""
    import os
    import re
    state = os.path.join(checkpoint_dir, 'checkpoint')
    print('Restoring Inception model from %s' % checkpoint_dir)
    m = re.search(r'model_checkpoint_path: "([^"]+)"', open(state).read()) if os.path.exists(state) else None
    path = os.path.join(checkpoint_dir, os.path.basename(m.group(1))) if m else None
    if path is None or not os.path.exists(path):
        print(' [!] Load failed...')
        raise RuntimeError('Could not load the Inception checkpoint from %s' % checkpoint_dir)
    with np.load(path) as z:
        arrays = {k: z[k] for k in variable_shapes(num_classes) if k in z.files}
    net = InceptionV3.from_arrays(arrays, num_classes, device, source='checkpoint %s' % path)
    print(' [*] Load SUCCESS')
    return net
