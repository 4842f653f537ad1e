"""The generator weight EMA without a device: the ABI entry, optim.AdamTF(ema_decay=...) on a CPU arena,
the checkpoint keys `<variable>/ExponentialMovingAverage` and their restore rules, PGGAN(g_ema=...) and the --g-ema flag."""
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_pggan_real_host import no_device  # noqa: E402,F401

EMA = '/ExponentialMovingAverage'
TINY = dict(fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)
BAD = (True, False, 0, 0.0, 1, 1.0, 1.5, -0.1, float('nan'), 'a', [0.5])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_fused_entry_within_v13():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    assert _lib.ABI_VERSION == 13 and _lib.lib.t2i_version() == 13
    res, args = _lib.SIGNATURES['t2i_adam_tf_ema']
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    m = re.search(r'\bint\s+t2i_adam_tf_ema\s*\(([^)]*)\)\s*;', header)
    assert m, 'include/t2i_hip.h does not declare t2i_adam_tf_ema'
    params = [a.strip() for a in m.group(1).split(',')]
    # t2i_adam_tf's twelve plus ema, ema_decay, ema_decay_dev, in the order of the prototype
    assert [a.split()[-1].lstrip('*') for a in params] == ['w', 'g', 'm', 'v', 'ema', 'n', 'lr_t', 'lr_t_dev', 'beta1', 'beta2', 'eps',
                                                          'grad_scale', 'ema_decay', 'ema_decay_dev', 'stream']
    assert len(args) == len(params) == len(_lib.SIGNATURES['t2i_adam_tf'][1]) + 3
    import ctypes
    assert res is ctypes.c_int
    kinds = ['p' if '*' in a or 't2i_stream_t' in a else ('i' if 'int64_t' in a else 'f') for a in params]
    want = {'p': ctypes.c_void_p, 'i': ctypes.c_int64, 'f': ctypes.c_float}
    assert args == [want[k] for k in kinds]
    assert hasattr(_lib.lib, 't2i_adam_tf_ema')


# ---- optim.AdamTF ---------------------------------------------------------------------------------------------------------------
def _arena(names=('g_net/a/w', 'g_net/b/w', 'g_net/c/bias'), shapes=((3, 5), (2, 2, 3), (7,)), seed=0):
    from t2i_amd import optim
    gen = torch.Generator().manual_seed(seed)
    return optim.Arena(OrderedDict((n, torch.randn(s, generator=gen).requires_grad_(True)) for n, s in zip(names, shapes)))


def test_adam_tf_shadow_on_a_cpu_arena():
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    a = _arena()
    plain = optim.AdamTF(a, 0.0, 0.99)
    assert plain.ema is None and plain.ema_decay is None
    opt = optim.AdamTF(a, 0.0, 0.99, ema_decay=0.9)
    assert opt.ema.dtype == torch.float32 and opt.ema.shape == a.flat.shape and opt.ema.data_ptr() != a.flat.data_ptr()
    assert torch.equal(opt.ema, a.flat) and not opt.ema.requires_grad
    assert float(opt.ema_decay_dev[0]) == np.float32(0.9) and opt.ema_decay == 0.9
    opt.set_ema_decay(0.5)
    assert float(opt.ema_decay_dev[0]) == 0.5 and opt.ema_decay == 0.5
    for bad in (True, 'a', -0.1, 1.5):
        with pytest.raises(ValueError):
            opt.set_ema_decay(bad)
    # sync_ema: the named slots, then every slot
    with torch.no_grad():
        a.flat.add_(1.0)
    before = opt.ema.clone()
    opt.sync_ema(['g_net/b/w'])
    o, k = a.offsets['g_net/b/w']
    assert torch.equal(opt.ema[o:o + k], a.flat[o:o + k])
    keep = torch.ones_like(before, dtype=torch.bool); keep[o:o + k] = False
    assert torch.equal(opt.ema[keep], before[keep])
    opt.sync_ema()
    assert torch.equal(opt.ema, a.flat)
    with pytest.raises(RuntimeError):
        plain.sync_ema()
    with pytest.raises(RuntimeError):
        plain.set_ema_decay(0.5)


@pytest.mark.parametrize('bad', BAD, ids=repr)
def test_adam_tf_refuses_a_bad_decay(bad):
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    with pytest.raises(ValueError, match='ema_decay'):
        optim.AdamTF(_arena(), 0.0, 0.99, ema_decay=bad)


# ---- utils/saver.py -------------------------------------------------------------------------------------------------------------
class _Store(object):
    def __init__(self, variables):
        self.vars = variables


def _world(seed):
    """A store with three generator variables in an arena and one critic variable outside it."""
    from t2i_amd import optim
    a = _arena(seed=seed)
    variables = OrderedDict([('d_net/x/w', torch.randn(4, 2, generator=torch.Generator().manual_seed(seed + 100)))])
    variables.update(a.vars)
    opt = optim.AdamTF(a, 0.0, 0.99, ema_decay=0.9)
    with torch.no_grad():
        opt.ema.copy_(torch.randn(opt.ema.shape, generator=torch.Generator().manual_seed(seed + 200)))
    return _Store(variables), a, opt


def _bits(t):
    return t.detach().clone().view(torch.int32)


def _same_slots(a, x, y):
    """Two flat buffers of arena `a` agree bit for bit on every variable's slot (the padding between slots is nobody's)."""
    return all(torch.equal(_bits(x[o:o + k]), _bits(y[o:o + k])) for o, k in a.offsets.values())


def test_saver_writes_and_restores_shadows(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.utils.saver import Saver, load, restore_scopes, save
    store, a, opt = _world(1)
    d = str(tmp_path / 'with')
    path = save(Saver(store, shadows=[opt]), None, d, 3)
    z = np.load(path)
    assert sorted(z.files) == sorted(list(store.vars) + [n + EMA for n in a.names])
    for n in a.names:
        o, k = a.offsets[n]
        assert z[n + EMA].shape == tuple(a.vars[n].shape)
        assert np.array_equal(z[n + EMA].reshape(-1).view(np.int32), opt.ema[o:o + k].numpy().view(np.int32))
        assert np.array_equal(z[n], a.vars[n].detach().numpy())
    # var_list selects: shadow keys for exactly the selected arena variables
    sel = Saver(store, var_list=['g_net/a/', 'd_net'], shadows=[opt]).state()
    assert sorted(sel) == sorted(['d_net/x/w', 'g_net/a/w', 'g_net/a/w' + EMA])
    # round trip into a different world: variable and shadow bits
    store2, a2, opt2 = _world(2)
    assert not torch.equal(opt2.ema, opt.ema)
    assert load(Saver(store2, shadows=[opt2]), None, d) == (True, 3)
    assert _same_slots(a, a2.flat, a.flat) and _same_slots(a, opt2.ema, opt.ema)
    assert torch.equal(store2.vars['d_net/x/w'], store.vars['d_net/x/w'])
    # arena variables outside var_list keep the shadow (and the value) they have
    store3, a3, opt3 = _world(3)
    ema3, flat3 = opt3.ema.clone(), a3.flat.detach().clone()
    load(Saver(store3, var_list=['g_net/b/'], shadows=[opt3]), None, d)
    o, k = a3.offsets['g_net/b/w']
    inside = torch.zeros_like(ema3, dtype=torch.bool); inside[o:o + k] = True
    assert torch.equal(opt3.ema[inside], opt.ema[inside]) and torch.equal(a3.flat[inside], a.flat[inside])
    assert torch.equal(opt3.ema[~inside], ema3[~inside]) and torch.equal(a3.flat[~inside], flat3[~inside])
    # ema=True: the shadow arrays as the variables
    store4, a4, opt4 = _world(4)
    restore_scopes(store4, [('g_net', d)], verbose=False, ema=True)
    for n in a.names:
        o, k = a.offsets[n]
        assert torch.equal(_bits(a4.vars[n]).reshape(-1), _bits(opt.ema[o:o + k])), n
    assert not torch.equal(store4.vars['d_net/x/w'], store.vars['d_net/x/w'])       # outside the scope: untouched
    with pytest.raises(ValueError, match='keeps no moving average'):
        from t2i_amd import optim
        Saver(store, shadows=[optim.AdamTF(a, 0.0, 0.99)])


def test_checkpoint_without_shadows(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.utils.saver import Saver, load, restore_scopes, save
    store, a, opt = _world(5)
    d = str(tmp_path / 'without')
    path = save(Saver(store), None, d, 7)
    assert sorted(np.load(path).files) == sorted(store.vars)                      # shadows=None: today's key set
    other = str(tmp_path / 'again')
    path2 = save(Saver(store, shadows=None), None, other, 7)
    assert open(path, 'rb').read() == open(path2, 'rb').read()
    # a file without shadow keys sets the shadow from the variables it restores
    store2, a2, opt2 = _world(6)
    load(Saver(store2, shadows=[opt2]), None, d)
    assert _same_slots(a, a2.flat, a.flat) and _same_slots(a, opt2.ema, a.flat)
    # ... and cannot be read as averaged weights
    store3, a3, _ = _world(7)
    before = a3.flat.detach().clone()
    with pytest.raises(KeyError) as e:
        restore_scopes(store3, [('g_net', d)], verbose=False, ema=True)
    assert 'g_net/a/w' + EMA in str(e.value) and 'trained without EMA' in str(e.value)
    assert torch.equal(a3.flat, before)


# ---- PGGAN ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [True, 0, 1, 1.5, 'a'], ids=repr)
def test_pggan_refuses_a_bad_g_ema(bad):
    import t2i_amd  # noqa: F401
    from t2i_amd import scope as S
    from t2i_amd.models.pggan.pggan import PGGAN
    store = S.VariableStore(device='cpu')
    with pytest.raises(ValueError, match='g_ema'):
        PGGAN(2, 100, None, None, None, None, None, 1, False, device='cpu', store=store, g_ema=bad, **TINY)
    assert not store.vars                                                          # before anything is built


def test_pggan_g_ema_gives_the_generator_alone_a_shadow():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    m = PGGAN(2, 100, None, None, None, None, None, 2, True, device='cpu', g_ema=0.5, **TINY)
    assert m.g_ema == 0.5 and m.D_optimizer.ema is None
    assert m.G_optimizer.ema_decay == 0.5 and torch.equal(m.G_optimizer.ema, m.g_arena.flat)
    assert m.G_optimizer.ema.data_ptr() != m.g_arena.flat.data_ptr()
    # ema_weights exchanges the two buffers and exchanges them back
    with torch.no_grad():
        m.G_optimizer.ema.mul_(0.5)
    flat, ema = m.g_arena.flat.detach().clone(), m.G_optimizer.ema.clone()
    with m.ema_weights():
        assert torch.equal(m.g_arena.flat, ema) and torch.equal(m.G_optimizer.ema, flat)
        assert torch.equal(next(iter(m.g_vars.values())).reshape(-1), ema[:next(iter(m.g_vars.values())).numel()])
    assert torch.equal(_bits(m.g_arena.flat), _bits(flat)) and torch.equal(_bits(m.G_optimizer.ema), _bits(ema))
    plain = PGGAN(2, 100, None, None, None, None, None, 2, True, device='cpu', **TINY)
    assert plain.g_ema is None and plain.G_optimizer.ema is None and plain.D_optimizer.ema is None
    with pytest.raises(RuntimeError, match='g_ema'):
        with plain.ema_weights():
            pass


# ---- the flags ------------------------------------------------------------------------------------------------------------------
def test_g_ema_flag_errors_before_the_device(tmp_path, no_device, capsys):  # noqa: F811
    TP = no_device
    for bad in ('1.5', '0', '1', '-0.5', 'nan', 'x'):
        with pytest.raises(SystemExit):
            TP.main(['--out', str(tmp_path / 'run'), '--first', '0', '--last', '0', '--iters', '2', '--g-ema', bad])
    assert '--g-ema' in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / 'run'))
    with pytest.raises(AssertionError, match='device work started'):               # a good value passes every check
        TP.main(['--out', str(tmp_path / 'run'), '--first', '0', '--last', '0', '--iters', '2', '--g-ema', '0.999'])


@pytest.mark.parametrize('module', ['eval_pggan', 'visualize_pggan', 'visualize_last_stage'])
def test_readers_take_the_ema_flag(module, capsys):
    import importlib
    import t2i_amd  # noqa: F401
    mod = importlib.import_module('t2i_amd.models.pggan.' + module)
    with pytest.raises(SystemExit):
        mod.main(['--help'])
    assert '--ema' in capsys.readouterr().out
