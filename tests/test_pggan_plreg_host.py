"""Host-side checks of PGGAN's path-length regularisation, no GPU: the options' validation by keyword and by
flag, the trainer's refusal before a directory is made, the schedule's named forms of the generator half, and what a model built with
pl_weight adds (a device scalar, a checkpoint entry outside g_net/ and d_net/) and does not add (variables)."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.fixture(scope='module')
def t2i():
    lib = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd
    return t2i_amd


def _pggan(**kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    args = dict(fmap_base=64, fmap_max=32, z_dim=16, embed_dim=32, compr_embed_dim=8, device='cpu')
    args.update(kw)
    stage, trans = args.pop('stage', 2), args.pop('trans', True)
    return PGGAN(4, 100, None, None, None, None, None, stage, trans, **args)


MOD = dict(style_dim=16, modulated_conv=True)


def test_option_validation_by_keyword(t2i):
    bad = ((dict(pl_weight=2.0), 'pl_weight needs modulated_conv'), (dict(style_dim=16, pl_weight=2.0), 'pl_weight needs modulated_conv .*AdaIN'),
           (dict(MOD, pl_weight=0.0), 'pl_weight must be'), (dict(MOD, pl_weight=-1.0), 'pl_weight must be'),
           (dict(MOD, pl_weight=float('inf')), 'pl_weight must be'), (dict(MOD, pl_weight=float('nan')), 'pl_weight must be'),
           (dict(MOD, pl_weight=True), 'pl_weight must be'), (dict(MOD, pl_weight='2'), 'pl_weight must be'),
           (dict(MOD, pl_weight=2.0, pl_interval=0), 'pl_interval must be'), (dict(MOD, pl_weight=2.0, pl_interval=2.0), 'pl_interval must be'),
           (dict(MOD, pl_weight=2.0, pl_shrink=0), 'pl_shrink must be'), (dict(MOD, pl_weight=2.0, pl_decay=0.0), 'pl_decay must be'),
           (dict(MOD, pl_weight=2.0, pl_decay=1.5), 'pl_decay must be'), (dict(MOD, pl_weight=2.0, pl_decay=float('nan')), 'pl_decay must be'),
           (dict(MOD, pl_weight=2.0, dp=object()), 'pl_weight under data parallelism is not done'))
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            _pggan(build_model=False, **kw)
    m = _pggan(build_model=False, pl_weight=2, **MOD)
    assert (m.pl_weight, m.pl_interval, m.pl_shrink, m.pl_decay) == (2.0, 4, 2, 0.01) and float(m.pl_mean) == 0.0 and m.pl_mean.shape == ()
    assert _pggan(build_model=False, pl_weight=1, pl_decay=1, **MOD).pl_decay == 1.0
    plain = _pggan(build_model=False, **MOD)
    assert plain.pl_weight is None and plain.pl_mean is None and not plain.pl_due(4)
    assert [m.pl_due(i) for i in range(1, 9)] == [False, False, False, True, False, False, False, True]


def test_flags(t2i):
    from t2i_amd.models.pggan import options as cli
    assert [cli.flag(k) for k in ('pl_weight', 'pl_interval', 'pl_shrink', 'pl_decay')] == ['--pl-weight', '--pl-interval', '--pl-shrink', '--pl-decay']

    def parse(argv, trainer=True):
        ap = argparse.ArgumentParser()
        (cli.add_trainer_arguments if trainer else cli.add_reader_arguments)(ap)
        return cli.kwargs_of(ap, ap.parse_args(argv))
    base = ['--style-dim', '16', '--modulated-conv']
    assert parse(base + ['--pl-weight', '2']) == {'style_dim': 16, 'modulated_conv': True, 'pl_weight': 2.0}
    assert parse(base + ['--pl-weight', '2', '--pl-interval', '8', '--pl-shrink', '4', '--pl-decay', '0.1']) == {
        'style_dim': 16, 'modulated_conv': True, 'pl_weight': 2.0, 'pl_interval': 8, 'pl_shrink': 4, 'pl_decay': 0.1}
    assert parse(base) == {'style_dim': 16, 'modulated_conv': True}
    for argv in (['--pl-weight', '2'], ['--style-dim', '16', '--pl-weight', '2'], base + ['--pl-weight', '0'], base + ['--pl-weight', 'nan'],
                 base + ['--pl-weight', '2', '--pl-interval', '0'], base + ['--pl-weight', '2', '--pl-shrink', '0'],
                 base + ['--pl-weight', '2', '--pl-decay', '0'], base + ['--pl-weight', '2', '--pl-decay', '1.5'], base + ['--pl-interval', '4'],
                 base + ['--pl-decay', '0.1']):
        with pytest.raises(SystemExit) as e:
            parse(argv)
        assert e.value.code == 2, argv
    for argv in (base + ['--pl-weight', '2'], ['--pl-interval', '4']):                    # the readers take none of them
        with pytest.raises(SystemExit) as e:
            parse(argv, trainer=False)
        assert e.value.code == 2


def test_the_trainer_refuses_before_a_directory_is_made(t2i, tmp_path, capsys):
    from t2i_amd.models.pggan import train_pggan as TP
    for argv, word in ((['--style-dim', '16', '--pl-weight', '2'], '--pl-weight needs --modulated-conv'),
                       (['--style-dim', '16', '--modulated-conv', '--pl-weight', '-1'], '--pl-weight must be'),
                       (['--style-dim', '16', '--modulated-conv', '--pl-weight', '2', '--pl-decay', '2'], '--pl-decay must be'),
                       (['--style-dim', '16', '--modulated-conv', '--pl-shrink', '2'], 'are the numbers of --pl-weight')):
        out = str(tmp_path / 'run')
        with pytest.raises(SystemExit) as e:
            TP.main(['--out', out] + argv)
        assert e.value.code == 2 and not os.path.exists(out)
        assert word in capsys.readouterr().err


def test_the_schedule_captures_and_replays_named_forms_of_the_generator_half(t2i):
    from t2i_amd.graphs import DGSchedule

    class Opt(object):
        def __init__(self, log, tag):
            self.log, self.tag = log, tag

        def prepare(self, lr):
            self.log.append((self.tag, 'prepare', lr))

        def apply(self, grad_scale=1.0, refresh=None):
            self.log.append((self.tag, 'apply'))

    class Graphs(object):
        def __init__(self):
            self.graphs, self.log = {}, []

        def capture(self, name, body, **kw):
            self.graphs[name] = body

        def load(self, feed):
            pass

        def replay(self, name):
            self.log.append(name)
            return name
    log = []
    sched = DGSchedule(None, lambda f: ('d', f), None, Opt(log, 'd'), lambda f, pl=False: ('g', f, pl), None, Opt(log, 'g'))
    assert sched.run('feed', 1e-3, 2e-3) == {'d': ('d', 'feed'), 'g': ('g', 'feed', False)}
    assert sched.run('feed', 1e-3, 2e-3, g_form=('g_pl', {'pl': True}))['g'] == ('g', 'feed', True)
    graphs = Graphs()
    sched.capture(graphs, g_forms={'g': {}, 'g_pl': {'pl': True}})
    assert list(graphs.graphs) == ['d', 'g', 'g_pl']
    assert graphs.graphs['g']('f') == ('g', 'f', False) and graphs.graphs['g_pl']('f') == ('g', 'f', True)
    assert sched.run('feed', 1e-3, 2e-3, graphs=graphs) == {'d': 'd', 'g': 'g'}
    assert sched.run('feed', 1e-3, 2e-3, graphs=graphs, g_form=('g_pl', {'pl': True})) == {'d': 'd', 'g': 'g_pl'}
    assert graphs.log == ['d', 'g', 'd', 'g_pl']
    plain = Graphs()
    sched.capture(plain)
    assert list(plain.graphs) == ['d', 'g']                                          # the default: today's two graphs
    with pytest.raises(ValueError, match='g_forms'):
        sched.capture(Graphs(), joint=lambda f: None, g_forms={'g': {}})


def test_the_model_adds_no_variable_and_one_checkpoint_entry(t2i, tmp_path):
    from t2i_amd.models.pggan import options as O
    from t2i_amd.utils.saver import load, save
    plain, reg = _pggan(stage=1, trans=False, seed=3, **MOD), _pggan(stage=1, trans=False, seed=3, pl_weight=2.0, **MOD)
    assert [(n, tuple(v.shape)) for n, v in plain.store.vars.items()] == [(n, tuple(v.shape)) for n, v in reg.store.vars.items()]
    assert all(torch.equal(plain.store.vars[n], reg.store.vars[n]) for n in plain.store.vars)
    files = {}
    for kind, m in (('plain', plain), ('reg', reg)):
        d = str(tmp_path / kind) + '/'
        if kind == 'reg':
            m.pl_mean.fill_(0.75)
        save(m._savers()[0], None, d, 7)
        files[kind] = (d, set(np.load(os.path.join(d, 'model-7.npz')).files))
    assert files['reg'][1] - files['plain'][1] == {O.PL_MEAN_KEY} and files['plain'][1] <= files['reg'][1]
    assert not O.PL_MEAN_KEY.startswith(('g_net/', 'd_net/'))
    z = np.load(os.path.join(files['reg'][0], 'model-7.npz'))
    assert z[O.PL_MEAN_KEY].dtype == np.float32 and z[O.PL_MEAN_KEY].shape == () and float(z[O.PL_MEAN_KEY]) == 0.75
    # resume: the entry is read back; a checkpoint without it leaves 0 and a line
    lines = []
    for kind, want, word in (('reg', 0.75, 'pl_mean 0.750000 restored'), ('plain', 0.0, 'carries no mean path length')):
        m = _pggan(stage=1, trans=False, seed=5, pl_weight=2.0, **MOD)
        m.pl_mean.fill_(0.25)
        m.check_dir_read = files[kind][0]
        _, src = m._savers()
        assert load(src, None, m.check_dir_read)[0]
        m._after_restore(src, lines.append)
        assert float(m.pl_mean) == want and any(word in s for s in lines), (kind, lines)
    with pytest.raises(ValueError, match='needs a model built with pl_weight'):
        plain.g_losses({'cond': torch.zeros(4, 32), 'z': torch.zeros(4, 16)}, pl=True)
