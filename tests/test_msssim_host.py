"""Multi-scale SSIM, host side (no GPU): the float64 restatement (tests/msssim_cases.py) against scipy, the separable window, the
argument checks of t2i_ssim_scale, the wrappers' and the constructor's refusals, the `--eval msssim` / `--msssim-pairs` plumbing of
the entry points and what evaluate_msssim draws from the global np.random stream."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import msssim_cases as MC  # noqa: E402


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', range(1, 12))
def test_separable_window_is_the_2d_gaussian(S):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    g = K.msssim_window(S, S + 3)
    assert g.dtype == np.float64 and g.shape == (S,) and abs(g.sum() - 1) <= 1e-15
    assert np.abs(np.outer(g, g) - MC.fspecial_gauss(S, S * 1.5 / 11)).max() <= 1e-15
    assert np.array_equal(g, g[::-1].copy()) or np.abs(g - g[::-1]).max() <= 1e-17        # symmetric: convolution = correlation
    assert np.array_equal(K.msssim_window(64, 64), K.msssim_window(11, 200)) and K.msssim_window(64, 64).shape == (11,)
    assert np.abs(np.outer(K.msssim_window(S, 40), K.msssim_window(S, 40)) - MC.window_2d(S, 40)).max() <= 1e-15


@pytest.mark.parametrize('h,w', [(5, 7), (16, 16), (37, 53)])
def test_downsample_taps_are_scipys_reflect_box_filter(h, w):
    a, _ = MC.pairs('indep', 3, 2, h, w, 3)
    got = MC.downsample(a)
    assert got.dtype == np.float32 and got.shape == (2, (h + 1) // 2, (w + 1) // 2, 3)
    assert np.array_equal(got.astype(np.float64), MC.downsample_scipy(a))                 # integer levels: the means are exact
    x = np.random.RandomState(4).standard_normal((1, h, w, 2))
    assert np.abs(MC.downsample(x) - MC.downsample_scipy(x)).max() <= 1e-15


def test_msssim_of_a_set_with_itself_is_one_and_the_families_behave():
    a, _ = MC.pairs('near', 1, 2, 32, 32, 3)
    same = MC.msssim(a, a)
    assert np.abs(same['values'] - 1).max() <= 1e-12 and same['clamped'] == 0
    near, flat = MC.msssim_reference('near', 1, (4, 32, 32, 3)), MC.msssim_reference('flat', 1, (4, 32, 32, 3))
    assert near['clamped'] == 0 and flat['clamped'] == 0 and near['cs'].min() >= 0.89 and flat['cs'].min() >= 0.89
    neg = MC.msssim_reference('neg', 1, (4, 32, 32, 3))
    assert neg['clamped'] == 20 and np.all(neg['values'] == 0.0)
    assert MC.msssim_reference('indep', 1, (4, 32, 32, 3))['clamped'] > 0
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation import msssim
    values, clamped = msssim.combine(near['cs'], near['ssim'])
    assert np.array_equal(values, near['values']) and clamped == 0
    assert msssim.WEIGHTS == MC.WEIGHTS and msssim.scale_sides(37, 53, 5) == [(37, 53), (19, 27), (10, 14), (5, 7), (3, 4)]
    x = np.linspace(-1.2, 1.2, 4001).astype(np.float32)
    import torch
    want = np.clip(np.round(x * np.float32(127.5) + np.float32(127.5)), 0, 255)
    assert np.array_equal(msssim.quantize(torch.from_numpy(x)).numpy(), want)


# ---- t2i_ssim_scale refuses bad arguments before any launch -------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    return _lib


P = ctypes.c_void_p
A, B, S_, CS, AH, BH, WS, BIG = P(0x10000000), P(0x20000000), P(0x30000000), P(0x31000000), P(0x40000000), P(0x50000000), P(0x60000000), 1 << 40


def _refused(lib, name, calls, rc=-1, word=b'bad argument'):
    fn = getattr(lib.lib, name)
    for args in calls:
        assert fn(*args, None) == rc, (name, args)
        msg = lib.lib.t2i_last_error()
        assert name.encode() in msg and word in msg, (name, args, msg)


def test_entries_are_declared_and_the_abi_version_stays(lib):
    assert lib.ABI_VERSION == 13 and lib.lib.t2i_version() == 13
    for name, nargs in (('t2i_ssim_scale_workspace_bytes', 4), ('t2i_ssim_scale', 17)):
        assert name in lib.SIGNATURES and hasattr(lib.lib, name) and len(lib.SIGNATURES[name][1]) == nargs, name
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    from t2i_amd import kernels as K
    assert '#define T2I_SSIM_MAX_WINDOW %d' % K.SSIM_MAX_WINDOW in header and K.SSIM_MAX_WINDOW == 11


def test_ssim_scale_refuses_bad_arguments(lib):
    q = lib.lib.t2i_ssim_scale_workspace_bytes
    assert q(2, 64, 64, 3) >= 2 * 16 and q(1, 1, 1, 1) >= 16
    assert q(0, 64, 64, 3) == 0 and q(2, 0, 64, 3) == 0 and q(2, 64, 0, 3) == 0 and q(2, 64, 64, 0) == 0 and q(2, 64, 64, 5) == 0
    assert q(1 << 20, 64, 64, 3) == 0                    # 2^20 * 64 * 64 * 3 >= 2^31
    win = (ctypes.c_double * 11)(*([1.0 / 11] * 11))
    g = ctypes.cast(win, P)
    ok = (A, B, 2, 64, 64, 3, g, 11, 6.5025, 58.5225, S_, CS, AH, BH, WS, BIG)

    def put(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    nan_win = (ctypes.c_double * 11)(*([1.0 / 11] * 10 + [float('nan')]))
    inf_win = (ctypes.c_double * 11)(*([float('inf')] + [1.0 / 11] * 10))
    bad = [put(0, None), put(1, None), put(10, None), put(11, None), put(6, None), put(14, None),       # a NULL tensor
           put(2, 0), put(2, -3), put(3, 0), put(4, 0), put(3, -64),                                     # N, H, W
           put(5, 0), put(5, 5),                                                                         # C
           put(7, 0), put(7, 12), put(7, -1),                                                            # S
           (A, B, 2, 8, 64, 3, g, 11) + ok[8:], (A, B, 2, 64, 10, 3, g, 11) + ok[8:],                    # S > min(H, W)
           put(2, 1 << 19),                                                                              # 2^19 * 64 * 64 * 3 >= 2^31
           (A, B, 1, 32768, 32768, 2) + ok[6:],                                                          # 2^31 exactly
           put(12, None), put(13, None),                                                                 # exactly one half
           put(10, A), put(11, B), put(12, A), put(13, P(0x20000000 + 4096)), put(14, A),                # an output on an input
           put(11, S_), put(13, AH), put(14, P(0x40000000 + 256)),                                       # outputs on each other
           put(15, 0), put(15, q(2, 64, 64, 3) - 1),                                                     # a short workspace
           put(6, ctypes.cast(nan_win, P)), put(6, ctypes.cast(inf_win, P)),                             # the window
           put(8, float('nan')), put(8, float('inf')), put(9, float('nan')), put(9, float('-inf')), put(9, 0.0), put(9, -1.0),
           put(0, P(0x10000002)), put(10, P(0x30000004)), put(12, P(0x40000001))]                        # misaligned
    _refused(lib, 't2i_ssim_scale', bad)
    assert b'S=11' in lib.lib.t2i_last_error() and b'N=2 H=64 W=64 C=3' in lib.lib.t2i_last_error()


def test_wrappers_refuse_cpu_and_bad_shapes(lib):
    import torch
    from t2i_amd import kernels as K
    g = K.msssim_window(16, 16)
    x = torch.zeros(2, 16, 16, 3)
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.ssim_scale(x, x.clone(), g, 6.5025, 58.5225)
    with pytest.raises(ValueError, match='ssim_scale'):
        K.ssim_scale(x.double(), x.double(), g, 6.5025, 58.5225)                       # not float32
    with pytest.raises(ValueError, match='ssim_scale'):
        K.ssim_scale(x.permute(0, 2, 1, 3)[:, :, :8], x.permute(0, 2, 1, 3)[:, :, :8], g, 6.5025, 58.5225)        # not contiguous
    with pytest.raises(ValueError, match='must match'):
        K.ssim_scale(x, torch.zeros(2, 16, 15, 3), g, 6.5025, 58.5225)
    with pytest.raises(ValueError, match='ssim_scale'):
        K.ssim_scale(torch.zeros(2, 16, 16, 5), torch.zeros(2, 16, 16, 5), g, 6.5025, 58.5225)
    with pytest.raises(ValueError, match='ssim_scale'):
        K.ssim_scale(torch.zeros(2, 8, 16, 3), torch.zeros(2, 8, 16, 3), g, 6.5025, 58.5225)          # a window of 11 on 8 rows
    with pytest.raises(ValueError, match='ssim_scale'):
        K.ssim_scale(x, x.clone(), np.ones(12) / 12, 6.5025, 58.5225)
    with pytest.raises(ValueError, match='finite'):
        K.ssim_scale(x, x.clone(), g, 6.5025, 0.0)
    with pytest.raises(ValueError, match='msssim_window'):
        K.msssim_window(0, 16)
    with K.dry_run():                                     # shapes only
        s, c, ah, bh = K.ssim_scale(torch.zeros(2, 37, 53, 3), torch.zeros(2, 37, 53, 3), g, 6.5025, 58.5225)
        assert s.dtype == c.dtype == torch.float64 and tuple(s.shape) == tuple(c.shape) == (2,)
        assert tuple(ah.shape) == tuple(bh.shape) == (2, 19, 27, 3) and ah.dtype == torch.float32
        assert K.ssim_scale(x, x.clone(), g, 6.5025, 58.5225, downsample=False)[2:] == (None, None)


def test_constructor_errors_come_before_any_allocation():
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.msssim import MultiScaleSSIM
    for shape in ((15, 64, 3), (64, 8, 3), (4, 4, 3)):
        with pytest.raises(ValueError, match='at least 16 x 16'):
            MultiScaleSSIM(shape, 'no such device')
    for c in (0, 5):
        with pytest.raises(ValueError, match='channels'):
            MultiScaleSSIM((32, 32, c), 'no such device')
    ms = MultiScaleSSIM((16, 24, 3), 'cpu')               # H != W is allowed
    assert ms.sides == [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)] and [len(w) for w in ms.windows] == [11, 8, 4, 2, 1]
    assert ms.c1 == (0.01 * 255.0) ** 2 and ms.c2 == (0.03 * 255.0) ** 2
    with pytest.raises(ValueError, match='no pairs'):
        ms.finalize()
    import torch
    with pytest.raises(ValueError, match='MS-SSIM.add'):
        ms.add(torch.zeros(2, 16, 24, 3), torch.zeros(2, 16, 16, 3))


# ---- the evaluator's draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pairs,n_pairs', [('random', 3 * 2), ('caption', 3 * 4)])
def test_global_numpy_stream_after_evaluate_msssim_is_that_of_the_inception_score(pairs, n_pairs, capsys):
    """A launch-free run (K.dry_run: the values are uninitialised memory): per batch the reference's draws — z ~ normal(0, 1,
    [bs, z_dim]) and then whatever the test split draws — and nothing else from the global stream; the second z of 'caption'
    comes from RandomState(0)."""
    import torch
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.evaluation.evaluator import GeneratorEval
    from t2i_amd.utils.config import AttrDict

    class Split(object):
        def next_batch(self, bs, k, embeddings=True):
            return None, None, np.random.standard_normal((bs, 8)).astype(np.float32), None, None

    class Data(object):
        test = Split()

    class Model(object):
        device, z_dim, embed_dim = torch.device('cpu'), 4, 8

    seen = []

    class Ev(GeneratorEval):
        def restore(self):
            self.restored = True

        def generate_batch(self, z, cond, is_training):
            assert not is_training and z.dtype == torch.float32 and tuple(z.shape) == (4, 4) and tuple(cond.shape) == (4, 8)
            seen.append((z.numpy().copy(), cond.numpy().copy()))
            return torch.zeros(4, 16, 16, 3)

    ev = Ev(None, Model(), Data(), AttrDict({'EVAL': {'SIZE': 13, 'SAMPLE_SIZE': 4, 'INCEP_BATCH_SIZE': 4}}))
    np.random.seed(11)
    with K.dry_run(), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        out = ev.evaluate_msssim(pairs=pairs)
    after = np.random.get_state()
    assert ev.restored and out['values'].shape == (n_pairs,) and out['sides'][0] == (16, 16) and len(out['cs_levels']) == 5
    text = capsys.readouterr().out
    assert 'MS-SSIM (%s) | mean:' % pairs in text and 'clamped:' in text and text.count('MS-SSIM (') == 2
    np.random.seed(11)                                    # evaluate_inception's draws, batch by batch
    want = []
    for _ in range(3):
        z = np.random.normal(0, 1, size=(4, 4))
        want.append((z.astype(np.float32), np.random.standard_normal((4, 8)).astype(np.float32)))
    expect = np.random.get_state()
    assert expect[0] == after[0] and np.array_equal(expect[1], after[1]) and expect[2:] == after[2:]
    first = seen if pairs == 'random' else seen[0::2]
    assert len(first) == 3 and all(np.array_equal(z, wz) and np.array_equal(c, wc) for (z, c), (wz, wc) in zip(first, want))
    if pairs == 'caption':                                # the regeneration: the same embeddings, z from RandomState(0)
        rs = np.random.RandomState(0)
        for (z, c), (_, wc) in zip(seen[1::2], want):
            assert np.array_equal(c, wc) and np.array_equal(z, rs.normal(0, 1, size=(4, 4)).astype(np.float32))
    with pytest.raises(ValueError, match='pairs'):
        ev.evaluate_msssim(pairs='class')
    ev.bs = 1
    with pytest.raises(ValueError, match='at least 2'):
        ev.evaluate_msssim(pairs='random')


# ---- entry points ---------------------------------------------------------------------------------------------------------------
def _gancls_cfg(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'text-to-image_amd', 'models', 'gancls', 'cfg', 'flowers.yml')))
    d = str(tmp_path / 'gancls')
    cfg.update(DATASET_DIR=d + '/data/', CHECKPOINT_DIR=d + '/ckpt/', LOGS_DIR=d + '/logs/', SAMPLE_DIR=d + '/samples/')
    cfg['TRAIN']['FLAG'] = True
    cfg['EVAL']['FLAG'] = False
    path = str(tmp_path / 'gancls.yml')
    yaml.safe_dump(cfg, open(path, 'w'))
    return path, d


def test_eval_msssim_parses_and_is_dispatched():
    import t2i_amd  # noqa: F401
    from t2i_amd.models import cli
    assert cli.EVAL_MODES == ('is', 'fid', 'imd', 'swd') and cli.PAIR_MODES == ('msssim',)
    ap = cli.make_parser('x.yml')
    args = ap.parse_args(['--eval', 'msssim'])
    assert args.eval == 'msssim' and args.msssim_pairs is None and not args.train and not args.visualize
    assert ap.parse_args(['--eval', 'msssim', '--msssim-pairs', 'caption']).msssim_pairs == 'caption'
    assert ap.parse_args(['--eval', 'swd']).msssim_pairs is None

    class Ev(object):                                     # run_eval looks up the requested mode's method only
        def evaluate_msssim(self, pairs):
            return 'msssim ran on %s pairs' % pairs

        def evaluate_fid(self):
            return 'fid ran'
    assert cli.run_eval(Ev(), 'msssim') == 'msssim ran on random pairs'
    assert cli.run_eval(Ev(), 'msssim', 'caption') == 'msssim ran on caption pairs'
    assert cli.run_eval(Ev(), 'fid') == 'fid ran' and cli.run_eval(Ev(), 'fid', None) == 'fid ran'
    from t2i_amd.evaluation.evaluator import GeneratorEval
    assert callable(GeneratorEval.evaluate_msssim)


def test_eval_msssim_argument_errors_before_any_device_work(tmp_path, capsys):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.gancls import run
    from t2i_amd.models.pggan import eval_pggan
    from t2i_amd.models.stackgan.stageI import run as run1
    from t2i_amd.models.wgancls import run as wrun
    cfg, d = _gancls_cfg(tmp_path)
    none = str(tmp_path / 'none.yml')
    for main in (run.main, run1.main, wrun.main):
        for argv in (['--msssim-pairs', 'caption'], ['--eval', 'swd', '--msssim-pairs', 'random'], ['--train', '--msssim-pairs', 'random']):
            with pytest.raises(SystemExit) as e:
                main(['--cfg', cfg] + argv)
            assert e.value.code == 2 and '--msssim-pairs needs --eval msssim' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            main(['--cfg', cfg, '--eval', 'msssim', '--msssim-pairs', 'class'])
        with pytest.raises(SystemExit):
            main(['--cfg', cfg, '--train', '--eval', 'msssim'])
        assert not os.path.exists(d)
    with pytest.raises(ValueError, match='synthetic'):
        run.main(['--cfg', cfg, '--eval', 'msssim', '--synthetic'])
    assert not os.path.exists(d)
    with pytest.raises(ValueError, match='synthetic'):
        wrun.main(['--cfg', cfg, '--eval', 'msssim', '--msssim-pairs', 'caption', '--synthetic'])
    capsys.readouterr()
    for stage in ('1', '2'):
        with pytest.raises(SystemExit):
            eval_pggan.main(['--cfg', none, '--eval', 'msssim', '--stage', stage])
        assert 'stage 3 or later' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        eval_pggan.main(['--cfg', none, '--eval', 'is', '--msssim-pairs', 'caption'])
    assert '--msssim-pairs needs --eval msssim' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        eval_pggan.main(['--cfg', none, '--eval', 'msssim', '--batch', '1'])
    assert '--batch 2 or more' in capsys.readouterr().err
    for argv in (['--stage', '3', '--ema'], ['--stage', '3', '--msssim-pairs', 'caption', '--batch', '1']):
        with pytest.raises(Exception) as e:               # these pass the argument checks: the missing yml is what stops them
            eval_pggan.main(['--cfg', none, '--eval', 'msssim'] + argv)
        assert not isinstance(e.value, SystemExit)
