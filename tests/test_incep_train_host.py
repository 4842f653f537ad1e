"""Host side of the InceptionV3 fine-tuning: the trained / restored / initialised partition from the layer table, the checkpoint
key set, pretrained-npz filtering, the configs and the entry point's arguments, and the Saver round trip of RMSProp slots."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_variable_partition_follows_the_layer_table():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception.model import variable_shapes
    from t2i_amd.models.inception.train_net import variable_partition
    for C in (20, 50):
        trained, restored, initialised = variable_partition(C)
        shapes = variable_shapes(C)
        assert set(restored) | set(initialised) == set(shapes) and not set(restored) & set(initialised)
        assert initialised == ['InceptionV3/Logits/Conv2d_1c_1x1/weights', 'InceptionV3/Logits/Conv2d_1c_1x1/biases']
        # Mixed_7c: 9 convolutions, each with weights and BatchNorm/beta; plus the logits' weights and biases
        assert len(trained) == 9 * 2 + 2
        assert all(k.startswith(('InceptionV3/Mixed_7c/', 'InceptionV3/Logits/')) for k in trained)
        assert not any(k.endswith(('moving_mean', 'moving_variance')) for k in trained)
        assert shapes['InceptionV3/Logits/Conv2d_1c_1x1/weights'] == (1, 1, 2048, C)
        n = sum(int(np.prod(shapes[k])) for k in trained)
        assert n == 6070272 + 3264 + 2048 * C + C, n


def test_checkpoint_keys_are_the_variables_plus_rmsprop_slots():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception.model import variable_shapes
    from t2i_amd.models.inception.train_net import checkpoint_keys, variable_partition
    keys = checkpoint_keys(20)
    assert len(keys) == len(set(keys))
    trained = variable_partition(20)[0]
    assert set(keys) == set(variable_shapes(20)) | {k + s for k in trained for s in ('/RMSProp', '/RMSProp_1')}
    assert 'InceptionV3/Mixed_7c/Branch_2/Conv2d_0b_3x3/BatchNorm/beta/RMSProp_1' in keys


def _write_pretrained(path, drop=None, extra=True, C=1001):
    from t2i_amd.models.inception.model import variable_shapes
    arrays = {k: np.full(s, 0.5, np.float32) for k, s in variable_shapes(C).items()}
    if extra:
        arrays['InceptionV3/AuxLogits/Conv2d_2b_1x1/weights'] = np.zeros((1, 1, 768, 1001), np.float32)
        arrays['InceptionV3/Mixed_5b/Branch_0/Conv2d_0a_1x1/weights/ExponentialMovingAverage'] = np.zeros((1, 1, 192, 64), np.float32)
        arrays['global_step'] = np.array(5)
    if drop:
        del arrays[drop]
    np.savez(path, **arrays)


def test_pretrained_npz_filtering_and_missing_keys(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception.train_net import pretrained_arrays, variable_partition
    p = str(tmp_path / 'imagenet.npz')
    _write_pretrained(p)
    got = pretrained_arrays(p, 20)
    assert sorted(got) == sorted(variable_partition(20)[1])          # the 1001-class logits and every extra key are ignored
    _write_pretrained(p, drop='InceptionV3/Mixed_6b/Branch_1/Conv2d_0c_7x1/BatchNorm/moving_variance')
    with pytest.raises(KeyError, match='Mixed_6b/Branch_1/Conv2d_0c_7x1/BatchNorm/moving_variance'):
        pretrained_arrays(p, 20)
    from t2i_amd.models.inception.model import variable_shapes
    arrays = {k: np.zeros(s, np.float32) for k, s in variable_shapes(20).items()}
    arrays['InceptionV3/Conv2d_1a_3x3/weights'] = np.zeros((3, 3, 3, 31), np.float32)
    np.savez(p, **arrays)
    with pytest.raises(ValueError, match='Conv2d_1a_3x3/weights'):
        pretrained_arrays(p, 20)


def test_configs_and_arguments():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception import run_incep
    from t2i_amd.utils.config import config_from_yaml
    for name, C in (('flowers', 20), ('birds', 50)):
        cfg = config_from_yaml(os.path.join(ROOT, 'text-to-image_amd', 'models', 'inception', 'cfg', name + '.yaml'))
        assert cfg.MODEL.CLASSES == C and cfg.TRAIN.BATCH_SIZE == 64 and cfg.TRAIN.FLAG is True
        for k in ('MAX_STEPS', 'RESTORE_PRETRAIN', 'PRETRAINED_CHECKPOINT_DIR', 'CHECKPOINTS_TO_KEEP', 'SUMMARY_PERIOD'):
            assert k in cfg.TRAIN
        for k in ('DATASET_DIR', 'CHECKPOINT_DIR', 'LOGS_DIR'):
            assert k in cfg
    assert run_incep.parse_args([]).cfg.endswith(os.path.join('cfg', 'flowers.yaml'))
    assert run_incep.parse_args(['--cfg', 'x.yaml']).cfg == 'x.yaml'
    with pytest.raises(SystemExit):
        run_incep.parse_args(['--steps', '3'])


def test_train_flag_false_does_nothing(tmp_path):
    import yaml
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception import run_incep
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'text-to-image_amd', 'models', 'inception', 'cfg', 'flowers.yaml')))
    cfg.update(DATASET_DIR=str(tmp_path / 'nodata'), CHECKPOINT_DIR=str(tmp_path / 'ck'), LOGS_DIR=str(tmp_path / 'logs'))
    cfg['TRAIN']['FLAG'] = False
    path = str(tmp_path / 'c.yaml')
    yaml.safe_dump(cfg, open(path, 'w'))
    assert run_incep.main(['--cfg', path]) is None
    assert os.path.isdir(str(tmp_path / 'ck')) and os.path.isdir(str(tmp_path / 'logs'))


class _FakeArena(object):
    def __init__(self, shapes):
        self.names = list(shapes)
        self.vars = OrderedDict((n, torch.zeros(s)) for n, s in shapes.items())
        self.offsets, off = OrderedDict(), 0
        for n, v in self.vars.items():
            self.offsets[n] = (off, v.numel())
            off += (v.numel() + 3) // 4 * 4
        self.flat = torch.zeros(off)


class _Store(object):
    def __init__(self, vars_):
        self.vars = vars_


def test_saver_round_trip_of_rmsprop_slots(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.optim import RMSPropTF
    from t2i_amd.utils.saver import Saver, load, save
    shapes = OrderedDict([('InceptionV3/Mixed_7c/Branch_0/Conv2d_0a_1x1/weights', (1, 1, 3, 5)),
                          ('InceptionV3/Logits/Conv2d_1c_1x1/biases', (7,))])
    arena = _FakeArena(shapes)
    opt = RMSPropTF.__new__(RMSPropTF)
    opt.arena = arena
    opt.ms = torch.ones_like(arena.flat)
    opt.mom = torch.zeros_like(arena.flat)
    rng = np.random.default_rng(0)
    opt.ms.copy_(torch.from_numpy(rng.random(arena.flat.numel()).astype(np.float32)))
    opt.mom.copy_(torch.from_numpy(rng.random(arena.flat.numel()).astype(np.float32)))
    store = _Store(arena.vars)
    for v in store.vars.values():
        v.copy_(torch.from_numpy(rng.random(tuple(v.shape)).astype(np.float32)))
    saver = Saver(store, optimizers={'': opt})
    path = save(saver, None, str(tmp_path), 200)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(list(shapes) + [k + s for k in shapes for s in ('/RMSProp', '/RMSProp_1')])
        o, k = arena.offsets['InceptionV3/Logits/Conv2d_1c_1x1/biases']
        assert np.array_equal(z['InceptionV3/Logits/Conv2d_1c_1x1/biases/RMSProp'], opt.ms[o:o + k].numpy())
    want = (opt.ms.clone(), opt.mom.clone(), {n: v.clone() for n, v in store.vars.items()})
    opt.ms.fill_(1.0); opt.mom.zero_()
    for v in store.vars.values():
        v.zero_()
    ok, counter = load(saver, None, str(tmp_path))
    assert ok and counter == 200
    for n in shapes:                 # the padding between slots is not saved: compare the slots
        o, k = arena.offsets[n]
        assert torch.equal(opt.ms[o:o + k], want[0][o:o + k]) and torch.equal(opt.mom[o:o + k], want[1][o:o + k])
        assert torch.equal(store.vars[n], want[2][n])
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files if not k.endswith('/RMSProp_1')}
    np.savez(str(tmp_path / 'model-300.npz'), **arrays)
    with pytest.raises(KeyError, match='RMSProp_1'):
        saver.restore(str(tmp_path / 'model-300.npz'))
