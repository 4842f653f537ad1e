"""InceptionV3 fine-tuning on the GPU: the head, dropout and RMSProp kernels against NumPy float64, the Mixed_7c + head step and
one whole training step against a float64 torch-CPU autograd oracle (training-mode batch norm, fed the kernel's dropout mask),
and `run_incep.py` end to end into `run.py --eval is`."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# ---- kernels -------------------------------------------------------------------------------------------------------------
def _np_head(y, W, b, labels):
    y, W, b = (np.asarray(a, np.float64) for a in (y, W, b))
    B = len(y)
    logits = y @ W + b
    e = np.exp(logits - logits.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    loss = float(np.mean(-np.log(p[np.arange(B), labels])))
    acc = float(np.mean(np.argmax(p, 1) == labels))
    dz = p.copy()
    dz[np.arange(B), labels] -= 1
    dz /= B
    return dict(logits=logits, prob=p, loss=loss, acc=acc, dW=y.T @ dz, db=dz.sum(0), dy=dz @ W.T)


@pytest.mark.parametrize('C', [20, 50])
def test_softmax_ce_head_matches_float64(C):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    rng = np.random.default_rng(C)
    B, D = 64, 2048
    y = rng.standard_normal((B, D)).astype(np.float32)
    W = (0.05 * rng.standard_normal((D, C))).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    labels = rng.integers(0, C, B).astype(np.int32)
    labels[:3] = [0, C - 1, 7]
    out = K.softmax_ce_head(_dev(y), _dev(W), _dev(b), _dev(labels, torch.int32))
    ref = _np_head(y, W, b, labels)
    for k in ('logits', 'prob', 'dW', 'db', 'dy'):
        got = out[k].cpu().numpy().astype(np.float64)
        err = np.abs(got - ref[k]).max() / np.abs(ref[k]).max()
        assert err <= 1e-5, (k, err)
    assert abs(float(out['loss']) - ref['loss']) <= 1e-5 * abs(ref['loss'])
    assert float(out['acc']) == ref['acc']
    again = K.softmax_ce_head(_dev(y), _dev(W), _dev(b), _dev(labels, torch.int32))
    for k in ('dW', 'dy', 'loss'):
        assert torch.equal(out[k], again[k])                 # no atomics: bitwise repeatable


@pytest.mark.parametrize('C', [20, 50])
def test_softmax_ce_head_ties_take_the_first_maximum(C):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    B, D = 4, 2048
    y = np.zeros((B, D), np.float32)
    W = np.zeros((D, C), np.float32)
    b = np.zeros(C, np.float32)
    b[[3, 5]] = 2.0                           # classes 3 and 5 tie for the maximum
    labels = np.array([3, 5, 0, 3], np.int32)
    out = K.softmax_ce_head(_dev(y), _dev(W), _dev(b), _dev(labels, torch.int32))
    assert float(out['acc']) == 0.5           # argmax is 3 for every row: rows 0 and 3 are right
    ref = _np_head(y, W, b, labels)
    assert abs(float(out['loss']) - ref['loss']) <= 1e-6 * ref['loss']


def test_dropout_mask_keep_rate_and_determinism():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    rng = np.random.default_rng(1)
    B, D = 64, 2048
    x = rng.standard_normal((B, 8, 8, D)).astype(np.float32)
    pre, mask, y = K.pool_dropout(_dev(x), 0.8, seed=5, step=10)
    m = mask.cpu().numpy()
    assert set(np.unique(m)) <= {0.0, 1.0}
    assert abs(m.mean() - 0.8) < 0.01, m.mean()
    ref_pre = x.astype(np.float64).reshape(B, 64, D).mean(1)
    assert np.abs(pre.cpu().numpy() - ref_pre).max() <= 1e-6 * np.abs(ref_pre).max()
    assert np.array_equal(y.cpu().numpy(), pre.cpu().numpy() / np.float32(0.8) * m)
    _, mask2, y2 = K.pool_dropout(_dev(x), 0.8, seed=5, step=10)
    assert torch.equal(mask, mask2) and torch.equal(y, y2)
    _, mask3, _ = K.pool_dropout(_dev(x), 0.8, seed=5, step=11)
    _, mask4, _ = K.pool_dropout(_dev(x), 0.8, seed=6, step=10)
    assert not torch.equal(mask, mask3) and not torch.equal(mask, mask4)
    assert abs(float((mask == mask3).float().mean()) - 0.68) < 0.02         # independent draws: P(equal) = .8^2 + .2^2


def test_pooled_grad_scatter_slices_branches():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    rng = np.random.default_rng(2)
    B, D = 3, 2048
    g = rng.standard_normal((B, D)).astype(np.float32)
    m = (rng.random((B, D)) < 0.8).astype(np.float32)
    widths = [320, 384, 384, 384, 384, 192]
    c0s = np.concatenate([[0], np.cumsum(widths)[:-1]])
    outs = [torch.empty((B, 8, 8, w), dtype=torch.float32, device=DEV) for w in widths]
    K.pooled_grad_scatter(_dev(g), _dev(m), 0.8, outs, list(c0s), 64)
    full = g * m / np.float32(0.8) / np.float32(64)
    for o, c0, w in zip(outs, c0s, widths):
        ref = np.broadcast_to(full[:, None, None, c0:c0 + w], (B, 8, 8, w))
        assert np.array_equal(o.cpu().numpy(), ref)


def test_rmsprop_tf_matches_float64():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.optim import Arena, RMSPropTF
    from collections import OrderedDict
    rng = np.random.default_rng(3)
    w0 = rng.standard_normal(1003).astype(np.float32)
    arena = Arena(OrderedDict(w=_dev(w0)))
    opt = RMSPropTF(arena, lr=5e-5)
    w, ms, mom = w0.astype(np.float64), np.ones(1003), np.zeros(1003)
    for step in range(5):
        g = (rng.standard_normal(1003) * 10.0 ** rng.integers(-4, 2, 1003)).astype(np.float32)
        arena.grad_of('w').copy_(_dev(g))
        opt.step()
        ms += (g.astype(np.float64) ** 2 - ms) * (1 - 0.9)
        mom = 5e-5 * g / np.sqrt(ms + 1e-10)
        w -= mom
        for got, ref in ((arena.vars['w'], w), (opt.ms[:1003], ms), (opt.mom[:1003], mom)):
            got = got.detach().cpu().numpy().astype(np.float64)
            assert np.all(np.abs(got - ref) <= 1e-6 * np.abs(ref) + 1e-12), (step, np.abs(got - ref).max())


# ---- oracle ------------------------------------------------------------------------------------------------------------
class _TrainOracle(object):
    """float64 torch-CPU statement of slim inception_v3(is_training=True): batch-statistics batch norm (biased variance to
    normalise, Bessel-corrected into the moving variance), TF SAME padding by explicit pads, dropout with a given mask.  P: name ->
    float64 tensor (the trained ones with requires_grad).  mixed_7b: start at Mixed_7c with this NCHW input."""

    def __init__(self, P, mask, mixed_7b=None, pins=None):
        self.P, self.mask, self.inject, self.pins = P, mask, mixed_7b, pins or {}
        self.moving = {}
        self.flips = 0

    def conv(self, x, name, kh, kw, cout, stride=1, padding='SAME', bn=True):
        import torch.nn.functional as F
        if self.inject is not None:
            if not name.startswith('Mixed_7c/'):
                return self.inject
            x, self.inject = self.inject, None
        base = 'InceptionV3/%s/' % name
        w = self.P[base + 'weights'].permute(3, 2, 0, 1)
        if padding == 'SAME':
            H, W = x.shape[2], x.shape[3]
            ph = max((-(-H // stride) - 1) * stride + kh - H, 0)
            pw = max((-(-W // stride) - 1) * stride + kw - W, 0)
            x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
        z = F.conv2d(x, w, stride=stride)
        if not bn:
            return z + self.P[base + 'biases'][None, :, None, None]
        mean = z.mean((0, 2, 3))
        var = z.var((0, 2, 3), unbiased=False)
        n = z.numel() // z.shape[1]
        d = 0.9997
        mm, mv = self.P[base + 'BatchNorm/moving_mean'], self.P[base + 'BatchNorm/moving_variance']
        self.moving[name] = ((mm * d + mean.detach() * (1 - d)).numpy(), (mv * d + var.detach() * n / (n - 1) * (1 - d)).numpy())
        zn = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + 0.001)
        a = zn + self.P[base + 'BatchNorm/beta'][None, :, None, None]
        if name in self.pins:                 # the device's ReLU branches (tests/branches.py): no kink flips near 0
            pin = self.pins[name].permute(0, 3, 1, 2).to(torch.float64)
            self.flips += int(((a.detach() > 0).to(torch.float64) != pin).sum())
            return a * pin
        return torch.relu(a)

    def pool(self, x, name, k, stride, padding, op):
        import torch.nn.functional as F
        from t2i_amd import kernels as K
        if self.inject is not None:
            return self.inject
        if name == 'Logits/AvgPool_1a_8x8':
            pre = x.mean((2, 3))
            return (pre / 0.8 * self.mask)[:, :, None, None]
        if op == K.POOL_MAX:
            return F.max_pool2d(x, k, stride)
        if padding == 'SAME':
            return F.avg_pool2d(x, 3, 1, padding=1, count_include_pad=False)
        return F.avg_pool2d(x, k, stride)

    pool_into = pool

    def concat(self, parts):
        if self.inject is not None:
            return self.inject
        return torch.cat(parts, 1)


def _oracle_step(arrays, trained, mask, labels, C, images=None, mixed_7b=None, pins=None):
    from t2i_amd.models.inception.model import _inception_v3
    P = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k in trained) for k, v in arrays.items()}
    o = _TrainOracle(P, torch.from_numpy(mask.astype(np.float64)),
                     None if mixed_7b is None else torch.from_numpy(mixed_7b.astype(np.float64)).permute(0, 3, 1, 2), pins)
    x = torch.zeros(1) if images is None else torch.from_numpy(images.astype(np.float64)).permute(0, 3, 1, 2)
    logits, _ = _inception_v3(o, x, C)
    logits = logits.reshape(len(labels), C)
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(labels.astype(np.int64)))
    loss.backward()
    print('oracle: %d ReLU branch flips pinned to the device\'s' % o.flips)
    return float(loss.detach()), {k: P[k].grad.numpy() for k in trained}, o.moving


def _random_arrays(seed, C):
    from t2i_amd.models.inception.model import variable_shapes
    rng = np.random.default_rng(seed)
    arrays = {}
    for k, shape in variable_shapes(C).items():
        if k.endswith('weights'):
            arrays[k] = (rng.standard_normal(shape) / np.sqrt(np.prod(shape[:3]))).astype(np.float32)
        elif k.endswith('beta') or k.endswith('biases'):
            arrays[k] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif k.endswith('moving_mean'):
            arrays[k] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        else:
            arrays[k] = (0.5 + rng.random(shape)).astype(np.float32)
    arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] *= 4
    return arrays


def _check_step(net, arrays, trained, head, loss_ref, grads_ref, moving_ref, grads, layers, tol=1e-4):
    from t2i_amd.models.inception.model import SCOPE
    loss = float(head['loss'])
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    errs = {}
    for k in trained:
        got = grads[k].astype(np.float64)
        ref = grads_ref[k].reshape(got.shape)
        errs[k] = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    print('\n'.join('%.2e  %s' % (e, k) for k, e in errs.items()))
    worst = max(errs.values())
    assert worst <= tol, max(errs, key=errs.get)
    for name in layers:
        mm, mv = net.moving[name]
        rm, rv = moving_ref[name]
        assert np.abs(mm.cpu().numpy() - rm).max() <= 1e-5 * max(np.abs(rm).max(), 1.0), name
        assert np.abs(mv.cpu().numpy() - rv).max() <= 1e-5 * max(np.abs(rv).max(), 1.0), name
        base = '%s/%s/BatchNorm/' % (SCOPE, name)
        assert not np.array_equal(mm.cpu().numpy(), arrays[base + 'moving_mean']), name
        assert not np.array_equal(mv.cpu().numpy(), arrays[base + 'moving_variance']), name
    return worst


def _pinned_step(net, layers, *args, **kw):
    """net.step, recording the sign of every batch-normed ReLU output (tests/branches.py) -> (head, layer -> [B,H,W,C] bool)."""
    from branches import record_branches
    rec = []
    with record_branches(rec):
        head = net.step(*args, **kw)
    assert len(rec) == len(layers), (len(rec), len(layers))
    return head, dict(zip(layers, rec))


def _grads_before_update(net):
    """The step's gradients: the arena keeps them after the update until the next zero_grad."""
    return {k: net.arena.grad_of(k).detach().cpu().numpy() for k in net.arena.names}


@pytest.mark.parametrize('C', [20, 50])
def test_mixed_7c_and_head_step_matches_autograd(C):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception.model import layer_table
    from t2i_amd.models.inception.train_net import InceptionTrainNet, variable_partition
    arrays = _random_arrays(4, C)
    trained = variable_partition(C)[0]
    rng = np.random.default_rng(5)
    B = 8
    x7b = np.maximum(rng.standard_normal((B, 8, 8, 2048)), 0).astype(np.float32)      # a ReLU output
    labels = rng.integers(0, C, B).astype(np.int32)
    net = InceptionTrainNet(arrays, C, DEV, seed=9)
    layers = [n for n in layer_table(C) if n.startswith('Mixed_7c/')]
    head, pins = _pinned_step(net, layers, None, _dev(labels, torch.int32), 0, mixed_7b=_dev(x7b))
    grads = _grads_before_update(net)
    mask = head['mask'].cpu().numpy()
    loss_ref, grads_ref, moving_ref = _oracle_step(arrays, trained, mask, labels, C, mixed_7b=x7b, pins=pins)
    worst = _check_step(net, arrays, trained, head, loss_ref, grads_ref, moving_ref, grads, layers)
    print('Mixed_7c + head C=%d: worst gradient error %.2e of max |ref|' % (C, worst))
    # the update itself: RMSProp from ms = 1 on the step's gradients
    for k in trained:
        g = grads[k].astype(np.float64)
        ms = 1.0 + (g * g - 1.0) * 0.1
        ref = arrays[k].astype(np.float64) - 5e-5 * g / np.sqrt(ms + 1e-10)
        got = net.store.vars[k].detach().cpu().numpy()
        assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max() + 1e-9, k


def test_full_network_training_step_matches_autograd():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception.model import layer_table
    from t2i_amd.models.inception.train_net import InceptionTrainNet, variable_partition
    C = 20
    arrays = _random_arrays(6, C)
    trained = variable_partition(C)[0]
    rng = np.random.default_rng(7)
    B = 2
    images = rng.uniform(-1, 1, (B, 299, 299, 3)).astype(np.float32)
    labels = np.array([3, 17], np.int32)
    net = InceptionTrainNet(arrays, C, DEV, seed=1)
    layers = [n for n in layer_table(C) if n != 'Logits/Conv2d_1c_1x1']
    head, pins = _pinned_step(net, layers, _dev(images), _dev(labels, torch.int32), 2)
    grads = _grads_before_update(net)
    loss_ref, grads_ref, moving_ref = _oracle_step(arrays, trained, head['mask'].cpu().numpy(), labels, C, images=images, pins=pins)
    # Mixed_7c's input carries the fp32 rounding of 85 batch-statistics layers at B = 2 (128 rows per channel in the last
    # blocks): measured on MI355X, 1.1e-4 .. 2.5e-4 of max |ref| on every Mixed_7c gradient, uniformly — the same block fed an
    # exact input agrees within 1.6e-6 (test_mixed_7c_and_head_step_matches_autograd)
    worst = _check_step(net, arrays, trained, head, loss_ref, grads_ref, moving_ref, grads, layers, tol=1e-3)
    print('full training step B=2: loss %.6f, worst gradient error %.2e of max |ref|' % (float(head['loss']), worst))
    for k in arrays:                            # the frozen trunk's variables are untouched, bit for bit
        if k not in trained and not k.endswith(('moving_mean', 'moving_variance')):
            assert np.array_equal(net.store.vars[k].cpu().numpy(), arrays[k]), k


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _make_incep_cfg(tmp_path, data_dir, pretrained, restore=True, steps=6):
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'text-to-image_amd', 'models', 'inception', 'cfg', 'flowers.yaml')))
    d = str(tmp_path)
    cfg.update(DATASET_DIR=data_dir, CHECKPOINT_DIR=d + '/incep_ckpt/', LOGS_DIR=d + '/incep_logs/')
    cfg['MODEL']['CLASSES'] = 20              # the evaluator's EVAL.NUM_CLASSES; the tiny data set uses 5 of them
    cfg['TRAIN'].update(RESTORE_PRETRAIN=restore, PRETRAINED_CHECKPOINT_DIR=pretrained, MAX_STEPS=steps, BATCH_SIZE=4,
                        SUMMARY_PERIOD=2, CHECKPOINTS_TO_KEEP=2)
    path = d + '/incep_%d.yaml' % steps
    yaml.safe_dump(cfg, open(path, 'w'))
    return path


def test_run_incep_end_to_end_into_eval(tmp_path, monkeypatch):
    import joblib
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.models.inception import run_incep, trainer
    from t2i_amd.models.inception.train_net import checkpoint_keys
    from t2i_amd.models.wgancls import run
    from t2i_amd.utils.summary import read_events
    from test_visualize import _make_cfg
    cache_was_on = K.filter_cache_enabled()
    try:
        gan_cfg = _make_cfg(tmp_path)
        np.random.seed(0); random.seed(0)
        run.main(['--cfg', gan_cfg, '--train', '--steps', '3', '--graphs', '0'])
        K.filter_cache(False)
        data_dir = str(tmp_path) + '/data/flowers/'
        n_test = len(joblib.load(data_dir + 'test/76images.pickle'))
        rng = np.random.default_rng(1)
        joblib.dump(list(rng.integers(0, 256, (n_test, 360, 360, 3), dtype=np.uint8)), data_dir + 'test/360images.pickle')
        arrays = _random_arrays(2, 1001)
        del arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'], arrays['InceptionV3/Logits/Conv2d_1c_1x1/biases']
        arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] = np.zeros((1, 1, 2048, 1001), np.float32)   # ImageNet head: ignored
        arrays['InceptionV3/AuxLogits/Conv2d_2b_1x1/weights'] = np.zeros((1, 1, 768, 1001), np.float32)
        arrays['global_step'] = np.array(1000)
        pre = str(tmp_path / 'imagenet.npz')
        np.savez(pre, **arrays)
        monkeypatch.setattr(trainer, 'SAVE_PERIOD', 4)
        np.random.seed(1); random.seed(1)
        last = run_incep.main(['--cfg', _make_incep_cfg(tmp_path, data_dir, pre, steps=6)])
        assert last['step'] == 5 and np.isfinite(last['loss'])
        ck = str(tmp_path / 'incep_ckpt')
        assert os.path.exists(ck + '/model-4.npz') and 'model-4.npz' in open(ck + '/checkpoint').read()
        with np.load(ck + '/model-4.npz') as z:
            assert sorted(z.files) == sorted(checkpoint_keys(20))
            assert np.all(z['InceptionV3/Mixed_7c/Branch_0/Conv2d_0a_1x1/weights/RMSProp'] != 1.0)
            assert not np.array_equal(z['InceptionV3/Mixed_6e/Branch_0/Conv2d_0a_1x1/BatchNorm/moving_mean'],
                                      arrays['InceptionV3/Mixed_6e/Branch_0/Conv2d_0a_1x1/BatchNorm/moving_mean'])
            assert np.array_equal(z['InceptionV3/Mixed_6e/Branch_0/Conv2d_0a_1x1/weights'],
                                  arrays['InceptionV3/Mixed_6e/Branch_0/Conv2d_0a_1x1/weights'])
        logs = [f for f in os.listdir(str(tmp_path / 'incep_logs')) if f.startswith('events.out.tfevents')]
        assert len(logs) == 1
        ev = read_events(str(tmp_path / 'incep_logs' / logs[0]))
        tags = {(e.get('step'), v['tag']) for e in ev for v in e['values']}
        assert {(2, 'loss'), (2, 'train_acc'), (4, 'loss'), (4, 'train_acc')} <= tags, tags
        assert any(t.startswith('image') for _, t in tags), tags
        # resume from the checkpoint: continues at step 5
        np.random.seed(2); random.seed(2)
        out = run_incep.main(['--cfg', _make_incep_cfg(tmp_path, data_dir, pre, restore=False, steps=9)])
        assert out['step'] == 8
        assert 'model-8.npz' in open(ck + '/checkpoint').read() and os.path.exists(ck + '/model-8.npz')
        # the evaluator reads the fine-tuned network unchanged
        cfg = yaml.safe_load(open(gan_cfg))
        cfg['EVAL'].update(INCEP_CHECKPOINT_DIR=ck + '/', SAMPLE_SIZE=8, SIZE=16, INCEP_BATCH_SIZE=4)
        yaml.safe_dump(cfg, open(gan_cfg, 'w'))
        np.random.seed(3); random.seed(3); torch.manual_seed(3)
        r = run.main(['--cfg', gan_cfg, '--eval', 'is'])
        assert np.isfinite(r['mean']) and r['mean'] >= 1.0 - 1e-9
    finally:
        K.filter_cache(cache_was_on)
        K.filter_cache_reset()
