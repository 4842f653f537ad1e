"""InceptionV3 in training mode for the fine-tuning of reference models/inception/trainer.py: slim
`inception_v3(images, num_classes, dropout_keep_prob=0.8, is_training=True)`, loss = mean sparse softmax cross-entropy, and
RMSProp on `InceptionV3/Mixed_7c/*` and `InceptionV3/Logits/*` only.

The network is the single layer table of model.py (`_inception_v3`) run by a third `ops` executor, `_Train`:
- every batch norm normalises with the BATCH statistics (is_training=True, also in the frozen trunk): conv_fwd_stats ->
  bn_train_stats (moving averages updated in place with decay 0.9997, the variance Bessel-corrected) -> bn_apply + ReLU.  A
  trunk activation is dropped as soon as the next layer has consumed it;
- Mixed_7c's layers keep their input, pre-normalisation output, statistics and ReLU output for the backward;
- AvgPool_1a_8x8 + Dropout_1b are one launch (t2i_pool_dropout, mask drawn on the device from (seed, step));
- Logits/Conv2d_1c_1x1 + the loss + its backward are t2i_softmax_ce_head.
The backward (`InceptionTrainNet.step`) stops at Mixed_7c's input: t2i_pooled_grad_scatter writes each branch output's gradient,
then Mixed_7c's layers are walked in reverse: bn_bwd_fused (ReLU and batch norm; dbeta into the gradient arena), then
conv_bwd_pair (data AND filter gradient) where the layer's input is another Mixed_7c layer's output, conv_bwd_filter alone where it
is the block input or its average pool.  The two data gradients that meet at a fan-out (Branch_1/Conv2d_0a_1x1,
Branch_2/Conv2d_0b_3x3) are summed.  AuxLogits are not built: they touch neither the loss nor the trained variables nor what the
evaluator reads."""
import collections

import numpy as np
import torch

from ... import kernels as K
from ...optim import Arena, RMSPropTF
from .model import BN_EPS, IMAGE_SIZE, PRELOGITS_DIM, SCOPE, _inception_v3, layer_table, variable_shapes

BN_DECAY = 0.9997
KEEP_PROB = 0.8
LOGITS = 'Logits/Conv2d_1c_1x1'
POOL = 'Logits/AvgPool_1a_8x8'
TRAINED_BLOCKS = ('Mixed_7c', 'Logits')          # tf.trainable_variables('InceptionV3/Logits') + ('InceptionV3/Mixed_7c')
NOT_RESTORED = ('Logits', 'AuxLogits')           # not taken from the pretrained checkpoint


def _block(key):
    return key[len(SCOPE) + 1:].split('/', 1)[0]


def variable_partition(num_classes=20):
    """-> (trained, restored, initialised): checkpoint keys of the network (variable_shapes order).  trained: the trainable
    variables of Mixed_7c and Logits (conv weights, BatchNorm/beta, the logits' biases); restored: every variable taken from the
    pretrained checkpoint (all but Logits/*); initialised: Logits/* (truncated normal weights, zero biases)."""
    trained, restored, initialised = [], [], []
    for key in variable_shapes(num_classes):
        if _block(key) in TRAINED_BLOCKS and not key.endswith(('moving_mean', 'moving_variance')):
            trained.append(key)
        (initialised if _block(key) in NOT_RESTORED else restored).append(key)
    return trained, restored, initialised


def checkpoint_keys(num_classes=20):
    """Every key a checkpoint of the fine-tuning holds: the variables plus the RMSProp slots of the trained ones."""
    trained = variable_partition(num_classes)[0]
    return list(variable_shapes(num_classes)) + [RMSPropTF.slot_key('', k, s) for k in trained for s in ('RMSProp', 'RMSProp_1')]


def pretrained_arrays(path, num_classes=20):
    """The restored variables from a pretrained npz keyed by slim's names (`InceptionV3/...`).  Extra keys (the 1001-class
    Logits, AuxLogits, moving-average copies, global_step) are ignored; a missing or mis-shaped variable is an error naming it."""
    shapes = variable_shapes(num_classes)
    out = {}
    with np.load(path) as z:
        files = set(z.files)
        for key in variable_partition(num_classes)[1]:
            if key not in files:
                raise KeyError('pretrained checkpoint %s has no variable %s' % (path, key))
            a = z[key]
            if tuple(a.shape) != shapes[key]:
                raise ValueError('pretrained checkpoint %s: %s has shape %s, the model needs %s' % (path, key, a.shape, shapes[key]))
            out[key] = a
    return out


class _Store(object):
    """What utils/saver.Saver reads: name -> device tensor, in variable_shapes order."""

    def __init__(self, vars_):
        self.vars = vars_


class _Train(object):
    """ops executor: training-mode batch norm everywhere, Mixed_7c's tensors kept for the backward.  update_moving: move the
    moving averages (the optimizer step's forward) or not (the summary's second forward).  mark(name): optional, called with
    'mixed_7c' when the first Mixed_7c layer starts (phase timing)."""

    def __init__(self, net, update_moving, seed, counter, mark=None, mixed_7b=None):
        self.net, self.update_moving, self.seed, self.counter, self.mark = net, update_moving, seed, counter, mark
        self.inject = mixed_7b                        # not None: every layer before Mixed_7c is skipped, Mixed_7c reads this
        self.saved = collections.OrderedDict()        # Mixed_7c layer -> (x, z, y, mean, rstd, desc, ws)
        self.producer = {}                            # id(Mixed_7c layer output) -> layer
        self.branches = None                          # [(layer, channel offset)] of the Mixed_7c concatenation
        self.head_in = None

    def conv(self, x, name, kh, kw, cout, stride=1, padding='SAME', bn=True):
        if not bn:                                    # the logits layer: run by t2i_softmax_ce_head in InceptionTrainNet
            assert name == LOGITS
            return x
        if self.inject is not None:
            if not name.startswith('Mixed_7c/'):
                return self.inject
            x, self.inject = self.inject, None
        net = self.net
        if name.startswith('Mixed_7c/') and not self.saved and self.mark is not None:
            self.mark('mixed_7c')
        B, H, W, cin = x.shape
        d, ws = K.conv_desc(B, H, W, cin, cout, kh, kw, stride, stride, padding, math=K.MATH_F32)
        z = K.conv_fwd_stats(x, net.weights[name], None, d, ws, out_dtype=torch.float32)
        mm, mv = net.moving[name] if self.update_moving else (None, None)
        mean, rstd, scale, shift = K.bn_train_stats(z, net.ones(cout), net.beta[name], BN_EPS, BN_DECAY, mm, mv)
        y = K.bn_apply(z, scale, shift, act=K.ACT_RELU)
        if name.startswith('Mixed_7c/'):
            self.saved[name] = (x, z, y, mean, rstd, d, ws)
            self.producer[id(y)] = name
        return y

    def pool(self, x, name, k, stride, padding, op):
        if self.inject is not None:
            return self.inject
        if name == POOL:
            B = x.shape[0]
            pre, mask, y = K.pool_dropout(x, KEEP_PROB, self.seed, self.counter)
            self.head_in = (pre, mask, y)
            return y.view(B, 1, 1, PRELOGITS_DIM)
        return K.pool2d(x, k, k, stride, stride, padding, op)

    def pool_into(self, x, name, k, stride, padding, op):
        return ('pool', x, k, stride, padding, op)

    def concat(self, parts):
        if self.inject is not None:
            return self.inject
        def chans(p):
            return p[1].shape[3] if isinstance(p, tuple) else p.shape[3]
        first = parts[0]
        B, H, W = first.shape[:3]
        out = torch.empty((B, H, W, sum(chans(p) for p in parts)), dtype=torch.float32, device=first.device)
        c0, branches = 0, []
        for p in parts:
            if isinstance(p, tuple):
                _, x, k, s, pad, op = p
                K.pool2d(x, k, k, s, s, pad, op, out=out, c0=c0)
            else:
                K.channel_slice_copy(p, out, c0)
                if id(p) in self.producer:
                    branches.append((self.producer[id(p)], c0))
            c0 += chans(p)
        if branches:
            assert len(branches) == len(parts)
            self.branches = branches
        return out


class InceptionTrainNet(object):
    """Device state of the fine-tuning: every variable of variable_shapes (trunk weights, betas and moving statistics as plain
    device tensors; the trained variables inside one Arena), the RMSProp optimizer over that arena, and the training step."""

    def __init__(self, arrays, num_classes=20, device=None, lr=5e-5, seed=0):
        self.device = device or torch.device('cuda', torch.cuda.current_device())
        self.num_classes, self.seed = num_classes, int(seed)
        shapes = variable_shapes(num_classes)
        trained = set(variable_partition(num_classes)[0])
        for key, shape in shapes.items():
            if key not in arrays:
                raise KeyError('no value for variable %s' % key)
            if tuple(np.shape(arrays[key])) != shape:
                raise ValueError('%s has shape %s, the model needs %s' % (key, np.shape(arrays[key]), shape))
        t = collections.OrderedDict((k, torch.from_numpy(np.ascontiguousarray(arrays[k], np.float32)).to(self.device)) for k in shapes)
        self.arena = Arena(collections.OrderedDict((k, v) for k, v in t.items() if k in trained))
        self.opt = RMSPropTF(self.arena, lr=lr)
        self.store = _Store(t)
        self.weights, self.beta, self.moving = {}, {}, {}
        for name in layer_table(num_classes):
            base = '%s/%s/' % (SCOPE, name)
            self.weights[name] = t[base + 'weights']
            if name != LOGITS:
                self.beta[name] = t[base + 'BatchNorm/beta']
                self.moving[name] = (t[base + 'BatchNorm/moving_mean'], t[base + 'BatchNorm/moving_variance'])
        self.logits_b = t['%s/%s/biases' % (SCOPE, LOGITS)]
        self._ones = {}
        self._dgamma = torch.zeros(2048, dtype=torch.float32, device=self.device)   # scale=False: the gamma gradient is discarded
        K.filter_cache_invalidate()

    def ones(self, c):
        if c not in self._ones:
            self._ones[c] = torch.ones(c, dtype=torch.float32, device=self.device)
        return self._ones[c]

    def _grad(self, name, var):
        return self.arena.grad_of('%s/%s/%s' % (SCOPE, name, var))

    def forward(self, images, labels, counter, update_moving=True, mark=None, head_grads=True, mixed_7b=None):
        """Training-mode forward + head (loss, accuracy and, with head_grads, the head's gradients into the arena).  -> (ops
        executor, head dict).  mixed_7b: [B, 8, 8, 2048] float32 — start at Mixed_7c with this input (images unused; tests and
        the phase benchmark)."""
        if mixed_7b is not None:
            ops = _Train(self, update_moving, self.seed, counter, mark, mixed_7b=mixed_7b.contiguous())
            with torch.no_grad():
                _inception_v3(ops, mixed_7b, self.num_classes)
            return ops, self._head(ops, labels, head_grads)
        if images.dtype != torch.float32 or images.dim() != 4 or tuple(images.shape[1:]) != (IMAGE_SIZE, IMAGE_SIZE, 3):
            raise ValueError('InceptionV3 takes float32 [B, 299, 299, 3], got %s %s' % (images.dtype, tuple(images.shape)))
        ops = _Train(self, update_moving, self.seed, counter, mark)
        with torch.no_grad():
            _inception_v3(ops, images.contiguous(), self.num_classes)
        return ops, self._head(ops, labels, head_grads)

    def _head(self, ops, labels, head_grads):
        with torch.no_grad():
            pre, mask, y = ops.head_in
            head = K.softmax_ce_head(y, self.weights[LOGITS], self.logits_b, labels,
                                     dW_out=self._grad(LOGITS, 'weights') if head_grads else None,
                                     db_out=self._grad(LOGITS, 'biases') if head_grads else None)
        head.update(pre=pre, mask=mask, dropped=y)
        return head

    def backward(self, ops, head):
        """Gradients of Mixed_7c's variables into the arena (the head's are there already)."""
        B = head['dy'].shape[0]
        saved = ops.saved
        grads = {}
        outs = []
        for name, c0 in ops.branches:
            g = torch.empty_like(saved[name][2])
            grads[name] = g
            outs.append((g, c0))
        K.pooled_grad_scatter(head['dy'], head['mask'], KEEP_PROB, [g for g, _ in outs], [c for _, c in outs], 64)
        for name in reversed(list(saved)):
            x, z, y, mean, rstd, d, ws = saved[name]
            C = z.shape[-1]
            dz, _, _ = K.bn_bwd_fused(grads.pop(name), y, z, mean, rstd, self.ones(C), K.ACT_RELU, dgamma_out=self._dgamma[:C],
                                      dbeta_out=self._grad(name, 'BatchNorm/beta'))
            src = ops.producer.get(id(x))
            dw = self._grad(name, 'weights')
            if src is None:                        # the block input (or its average pool): filter gradient only
                K.conv_bwd_filter(x, dz, d, ws, out=dw)
            else:
                dx = K.conv_bwd_pair(K.PAIR_BWD_DATA, dz, self.weights[name], x, dz, d, ws, dw)
                grads[src] = K.add_act(grads[src], dx) if src in grads else dx
        assert not grads, list(grads)
        return B

    def step(self, images, labels, counter, mark=None, mixed_7b=None):
        """One optimizer step (reference `sess.run([opt_step, loss])`): zero the gradients, training forward with moving-average
        updates, head, Mixed_7c backward, RMSProp.  -> head dict (loss / acc as device tensors)."""
        self.arena.zero_grad()
        ops, head = self.forward(images, labels, counter, True, mark, mixed_7b=mixed_7b)
        if mark is not None:
            mark('backward')
        self.backward(ops, head)
        del ops
        if mark is not None:
            mark('optimizer')
        self.opt.step()
        return head

    def evaluate(self, images, labels, counter):
        """The summary's second training-mode forward after the update: fresh dropout, no moving-average update, no step."""
        _, head = self.forward(images, labels, counter, update_moving=False, head_grads=False)
        return head
