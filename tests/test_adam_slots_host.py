"""Per-slot multipliers in the Adam launch and the equalized learning rate, without a device: the ABI entry,
the tables optim.AdamTF(slot_scales=...) builds, PGGAN(equalized_lr=..., adam_lr=...)'s initialisation and its unchanged default,
and the --equalized-lr / --lr flags."""
import ctypes
import math
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

TINY = dict(fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_slots_entry_within_v13():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    from t2i_amd import kernels as K
    assert _lib.ABI_VERSION == 13 and _lib.lib.t2i_version() == 13
    res, args = _lib.SIGNATURES['t2i_adam_tf_slots']
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    m = re.search(r'\bint\s+t2i_adam_tf_slots\s*\(([^)]*)\)\s*;', header)
    assert m, 'include/t2i_hip.h does not declare t2i_adam_tf_slots'
    params = [a.strip() for a in m.group(1).split(',')]
    assert [a.split()[-1].lstrip('*') for a in params] == ['w', 'g', 'm', 'v', 'ema', 'n', 'slot_end_dev', 'slot_mult_dev', 'n_slots', 'lr_t',
                                                          'lr_t_dev', 'beta1', 'beta2', 'eps', 'grad_scale', 'ema_decay', 'ema_decay_dev', 'stream']
    kinds = ['p' if '*' in a or 't2i_stream_t' in a else ('l' if 'int64_t' in a else ('i' if 'int32_t' in a else 'f')) for a in params]
    want = {'p': ctypes.c_void_p, 'l': ctypes.c_int64, 'i': ctypes.c_int32, 'f': ctypes.c_float}
    assert res is ctypes.c_int and args == [want[k] for k in kinds]
    assert hasattr(_lib.lib, 't2i_adam_tf_slots')
    cap = re.search(r'#define\s+T2I_ADAM_MAX_SLOTS\s+(\d+)', header)
    assert cap and int(cap.group(1)) == K.ADAM_MAX_SLOTS >= 108          # PGGAN stage 7t: 108 variables over both arenas


# ---- optim.AdamTF ---------------------------------------------------------------------------------------------------------------
NAMES = ('net/a/w', 'net/a/b', 'net/b/w', 'net/b/b')


def _arena(sizes=(5, 1, 4, 7), seed=0):
    from t2i_amd import optim
    gen = torch.Generator().manual_seed(seed)
    return optim.Arena(OrderedDict((n, torch.randn(k, generator=gen).requires_grad_(True)) for n, k in zip(NAMES, sizes)))


def test_slot_tables():
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    a = _arena()
    assert a.numel == 24
    c = math.sqrt(2.0 / 27)
    opt = optim.AdamTF(a, 0.0, 0.99, slot_scales={'net/a/w': c, 'net/b/w': (0.01, 3.0)})
    assert opt.slot_end.dtype == torch.int64 and opt.slot_end.tolist() == [8, 12, 16, 24]
    assert opt.slot_mult.dtype == torch.float32 and tuple(opt.slot_mult.shape) == (4, 2) and opt.slot_mult.is_contiguous()
    want = np.array([[c, c], [1, 1], [0.01, 3.0], [1, 1]], np.float32)
    assert np.array_equal(opt.slot_mult.numpy(), want)
    assert opt.slot_end.device == a.flat.device == opt.slot_mult.device
    assert optim.AdamTF(a, 0.0, 0.99, slot_scales={}).slot_mult.tolist() == [[1.0, 1.0]] * 4       # a mapping: nothing named keeps 1


def test_slot_scales_none_builds_nothing():
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    a = _arena()
    for opt in (optim.AdamTF(a, 0.0, 0.99), optim.AdamTF(a, 0.0, 0.99, slot_scales=None), optim.AdamTF(a, 0.5, 0.99, ema_decay=0.5)):
        assert opt.slot_end is None and opt.slot_mult is None and opt.slot_scales is None
        assert 'slot_end' not in vars(opt) and 'slot_mult' not in vars(opt)


def test_slot_scales_errors():
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    a = _arena()
    with pytest.raises(KeyError, match='net/c/w'):
        optim.AdamTF(a, 0.0, 0.99, slot_scales={'net/c/w': 0.5})
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), True, 'a', None, (1.0,), (1.0, 2.0, 3.0), (1.0, 0.0), (float('nan'), 1.0), (1.0, -2.0)):
        with pytest.raises(ValueError, match='net/a/w'):
            optim.AdamTF(a, 0.0, 0.99, slot_scales={'net/a/w': bad})


# ---- PGGAN ----------------------------------------------------------------------------------------------------------------------
def _c(name, v):
    """c = sqrt(2 / fan_in) of a kernel (kh kw Cin for a convolution, `in` for fc); None for every other variable."""
    if name.endswith('/weights'):
        return math.sqrt(2.0 / (v.shape[0] * v.shape[1] * v.shape[2]))
    if name.endswith('/kernel'):
        return math.sqrt(2.0 / v.shape[0])
    return None


def test_equalized_initialisation():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    off = PGGAN(2, 100, None, None, None, None, None, 4, False, device='cpu')
    on = PGGAN(2, 100, None, None, None, None, None, 4, False, device='cpu', equalized_lr=True)
    assert on.equalized_lr is True and off.equalized_lr is False and on.adam_lr == off.adam_lr == 2e-6
    assert [(n, tuple(v.shape)) for n, v in on.store.vars.items()] == [(n, tuple(v.shape)) for n, v in off.store.vars.items()]
    checked = 0
    for n, v in on.store.vars.items():
        c = _c(n, v)
        if c is None:                          # biases, gamma, beta: what they are without the flag
            assert torch.equal(v, off.store.vars[n]), n
            continue
        N = v.numel()
        if N < 4096:
            continue
        x = v.detach().double()
        std = float(x.std())
        assert abs(std / c - 1.0) <= 5.0 / math.sqrt(2.0 * N), (n, std, c)
        assert float(x.abs().max()) > 2.0 * c, n                 # a truncated normal stops at two standard deviations
        assert float(off.store.vars[n].detach().abs().max()) <= 2.0 * math.sqrt(1.3) * c * (1 + 1e-6), n      # ... as the He default does
        checked += 1
    assert checked >= 20
    # the optimizers: (c, c) for every kernel, (1, 1) for the rest, in arena order
    for arena, opt in ((on.d_arena, on.D_optimizer), (on.g_arena, on.G_optimizer)):
        want = [[_c(n, v) or 1.0] * 2 for n, v in arena.vars.items()]
        assert np.array_equal(opt.slot_mult.numpy(), np.array(want, np.float32))
        assert opt.slot_end.tolist() == [o + (k + 3) // 4 * 4 for o, k in arena.offsets.values()] and opt.slot_end[-1] == arena.numel
        assert any(w[0] != 1.0 for w in want) and any(w[0] == 1.0 for w in want)
    assert off.D_optimizer.slot_end is None and off.G_optimizer.slot_end is None


def test_default_model_is_unchanged():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    a = PGGAN(2, 100, None, None, None, None, None, 2, True, device='cpu', seed=3, **TINY)
    b = PGGAN(2, 100, None, None, None, None, None, 2, True, device='cpu', seed=3, equalized_lr=False, adam_lr=None, **TINY)
    assert list(a.store.vars) == list(b.store.vars)
    for n, v in a.store.vars.items():
        assert torch.equal(v.detach().view(torch.int32), b.store.vars[n].detach().view(torch.int32)), n
    assert a.adam_lr == b.adam_lr == 0.000002
    for m in (a, b):
        assert m.D_optimizer.slot_end is None and m.G_optimizer.slot_end is None
    # the flag changes the kernels' values and nothing about the registry
    c = PGGAN(2, 100, None, None, None, None, None, 2, True, device='cpu', seed=3, equalized_lr=True, adam_lr=1e-3, **TINY)
    assert c.adam_lr == 1e-3 and [(n, tuple(v.shape)) for n, v in c.store.vars.items()] == [(n, tuple(v.shape)) for n, v in a.store.vars.items()]
    assert list(c.d_arena.offsets.items()) == list(a.d_arena.offsets.items()) and list(c.g_arena.offsets.items()) == list(a.g_arena.offsets.items())
    assert any(not torch.equal(v, a.store.vars[n]) for n, v in c.store.vars.items())


@pytest.mark.parametrize('bad', [True, 0, 0.0, -1e-3, float('nan'), float('inf'), 'a', [1e-3]], ids=repr)
def test_pggan_refuses_a_bad_adam_lr(bad):
    import t2i_amd  # noqa: F401
    from t2i_amd import scope as S
    from t2i_amd.models.pggan.pggan import PGGAN
    store = S.VariableStore(device='cpu')
    with pytest.raises(ValueError, match='adam_lr'):
        PGGAN(2, 100, None, None, None, None, None, 1, False, device='cpu', store=store, adam_lr=bad, **TINY)
    assert not store.vars                                                          # before anything is built


def test_pggan_refuses_a_bad_equalized_lr():
    import t2i_amd  # noqa: F401
    from t2i_amd import scope as S
    from t2i_amd.models.pggan.pggan import PGGAN
    store = S.VariableStore(device='cpu')
    for bad in (1, 'yes', None, 0.5):
        with pytest.raises(ValueError, match='equalized_lr'):
            PGGAN(2, 100, None, None, None, None, None, 1, False, device='cpu', store=store, equalized_lr=bad, **TINY)
    assert not store.vars


# ---- the flags ------------------------------------------------------------------------------------------------------------------
def test_lr_flag_errors_before_the_device(tmp_path, no_device, capsys):  # noqa: F811
    TP = no_device
    for bad in ('0', '-1e-3', 'nan', 'inf', 'x'):
        with pytest.raises(SystemExit):
            TP.main(['--out', str(tmp_path / 'run'), '--first', '0', '--last', '0', '--iters', '2', '--equalized-lr', '--lr', bad])
        assert '--lr' in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / 'run'))
    with pytest.raises(AssertionError, match='device work started'):               # good values pass every check
        TP.main(['--out', str(tmp_path / 'run'), '--first', '0', '--last', '0', '--iters', '2', '--equalized-lr', '--lr', '1e-3'])
    with pytest.raises(SystemExit):
        TP.main(['--help'])
    out = capsys.readouterr().out
    assert '--equalized-lr' in out and '--lr' in out


def test_flags_reach_the_model(tmp_path, monkeypatch):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan import train_pggan as TP
    seen = []

    class Stop(Exception):
        pass

    def model(**kw):
        seen.append(kw)
        raise Stop()
    monkeypatch.setattr(TP.K, 'set_math', lambda *a: None)
    monkeypatch.setattr(TP, 'PGGAN', model)
    monkeypatch.setattr(TP, 'dataset_for', lambda size, dev: None)
    for extra in ([], ['--equalized-lr', '--lr', '1e-3'], ['--bench', '--equalized-lr', '--lr', '2e-3']):
        with pytest.raises(Stop):
            TP.main(['--out', str(tmp_path / 'run'), '--first', '0', '--last', '0', '--iters', '2'] + extra)
    assert 'equalized_lr' not in seen[0] and 'adam_lr' not in seen[0]              # without the flags: today's call
    assert seen[1]['equalized_lr'] is True and seen[1]['adam_lr'] == 1e-3
    assert seen[2]['equalized_lr'] is True and seen[2]['adam_lr'] == 2e-3
