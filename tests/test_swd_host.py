"""Sliced Wasserstein distance, host side (no GPU): the float64 restatement (tests/swd_cases.py) against scipy, pyramid_levels,
the argument checks of the seven C entries, the `--eval swd` plumbing of the entry points and the metric's private random stream."""
import ctypes
import os
import sys

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import swd_cases as SC  # noqa: E402


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 7, 7, 1), (1, 8, 16, 3), (2, 9, 5, 2)])
def test_polyphase_upsampling_equals_zero_insert_and_scipy(shape):
    g = np.random.RandomState(1).standard_normal(shape)
    want, got = SC.pyr_up_zero_insert(g), SC.pyr_up_polyphase(g)
    assert got.shape == want.shape == (shape[0], 2 * shape[1], 2 * shape[2], shape[3])
    assert np.abs(got - want).max() <= 1e-14 * np.abs(g).max()


def test_pyramid_restatement_reconstructs_and_halves():
    x = SC.images(0, 2, 64, 64, 3).astype(np.float64)
    lap = SC.laplacian_pyramid(x, 3)
    assert [l.shape for l in lap] == [(2, 64, 64, 3), (2, 32, 32, 3), (2, 16, 16, 3)]
    g = lap[2]                                            # the pyramid is invertible: g_i = lap_i + up(g_{i+1})
    for i in (1, 0):
        g = lap[i] + SC.pyr_up_zero_insert(g)
    assert np.abs(g - x).max() <= 1e-14
    const = SC.laplacian_pyramid(np.full((1, 32, 32, 1), 0.7), 2)           # the filters sum to one, edges included
    assert np.abs(const[0]).max() <= 1e-15 and np.abs(const[1] - 0.7).max() <= 1e-15


def test_descriptor_order_is_channel_then_rows_then_columns():
    level = np.arange(2 * 9 * 10 * 3, dtype=np.float64).reshape(2, 9, 10, 3)
    pos = np.array([[[3, 3], [5, 6]], [[4, 4], [5, 3]]])
    d = SC.descriptors(level, pos)
    assert d.shape == (4, 147)
    for row, (n, y, x) in enumerate([(0, 3, 3), (0, 5, 6), (1, 4, 4), (1, 5, 3)]):
        for c, dy, dx in ((0, 0, 0), (2, 6, 6), (1, 3, 5)):
            assert d[row, c * 49 + dy * 7 + dx] == level[n, y + dy - 3, x + dx - 3, c]


def test_swd_of_a_set_with_itself_is_zero_and_of_a_shifted_copy_is_not():
    rng = np.random.RandomState(2)
    x = SC.images(3, 4, 32, 32, 3)
    lap = SC.laplacian_pyramid(x, 2)
    pos = rng.randint(3, 32 - 3, size=(4, 16, 2))
    A = SC.descriptors(lap[0], pos)
    dirs = [rng.randn(147, 8) for _ in range(2)]
    dirs = [d / np.sqrt((d * d).sum(0, keepdims=True)) for d in dirs]
    assert SC.sliced_distance(A, A.copy(), dirs, 3) == 0.0
    assert SC.sliced_distance(A, 2.5 * A + 1.0, dirs, 3) <= 1e-12          # the scale is irrelevant: the descriptors are standardised
    shifted = SC.descriptors(SC.laplacian_pyramid(np.roll(x, 5, axis=2) * np.linspace(0.2, 1, 32).reshape(1, 1, 32, 1), 2)[0], pos)
    assert SC.sliced_distance(A, shifted, dirs, 3) > 1e-3


def test_pyramid_levels():
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.swd import pyramid_levels
    assert [pyramid_levels(s) for s in (256, 128, 64, 32, 16, 512, 48, 17)] == [5, 4, 3, 2, 1, 6, 2, 1]
    for bad in (15, 8, 4, 0):
        with pytest.raises(ValueError, match='at least 16'):
            pyramid_levels(bad)


# ---- the C entries refuse bad arguments before any launch ---------------------------------------------------------------------
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
X, Y, Z, W_, V, BIG = P(0x10000000), P(0x20000000), P(0x30000000), P(0x40000000), P(0x50000000), 1 << 40


def _refused(lib, name, calls, rc=-1, word=b'bad argument'):
    fn = getattr(lib.lib, name)
    for args in calls:
        assert fn(*args, None) == rc, (name, args)
        msg = lib.lib.t2i_last_error()
        assert name.encode() in msg and word in msg, (name, args, msg)


def test_entries_are_declared_and_the_abi_version_stays(lib):
    assert lib.ABI_VERSION == 13 and lib.lib.t2i_version() == 13
    for name, nargs in (('t2i_laplacian_pyramid_workspace_bytes', 5), ('t2i_laplacian_pyramid', 10), ('t2i_swd_descriptors', 11),
                        ('t2i_swd_channel_stats_workspace_bytes', 2), ('t2i_swd_channel_stats', 8), ('t2i_swd_project', 10),
                        ('t2i_segmented_sort_chunk', 0), ('t2i_segmented_sort_f32', 4), ('t2i_sorted_l1_mean_workspace_bytes', 2),
                        ('t2i_sorted_l1_mean', 9)):
        assert name in lib.SIGNATURES and hasattr(lib.lib, name) and len(lib.SIGNATURES[name][1]) == nargs, name
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    chunk = lib.lib.t2i_segmented_sort_chunk()
    assert chunk >= 4 and chunk & (chunk - 1) == 0 and '#define T2I_SORT_CHUNK %d' % chunk in header


def test_laplacian_pyramid_refuses_bad_arguments(lib):
    q = lib.lib.t2i_laplacian_pyramid_workspace_bytes
    assert q(2, 64, 64, 3, 3) >= 2 * 32 * 32 * 3 * 4 and q(2, 32, 32, 3, 2) == 0 and q(2, 16, 16, 3, 1) == 0      # only g_1 .. g_{L-2}
    assert q(2, 64, 64, 5, 3) == 0 and q(2, 60, 64, 3, 4) == 0 and q(0, 64, 64, 3, 3) == 0
    ok = (X, 2, 64, 64, 3, 3, Y, Z, BIG)
    bad = [(None,) + ok[1:], ok[:6] + (None,) + ok[7:], (X, 0) + ok[2:], (X, 2, 0) + ok[3:], (X, 2, 64, -4) + ok[4:],
           (X, 2, 64, 64, 0) + ok[5:], (X, 2, 64, 64, 5) + ok[5:], (X, 2, 64, 64, 3, 0) + ok[6:],
           (X, 2, 60, 64, 3, 4) + ok[6:],                 # 60 is no multiple of 8
           (X, 2, 16, 16, 3, 3) + ok[6:],                 # coarsest side 4 < 7
           (P(0x10000002),) + ok[1:],                     # misaligned
           ok[:6] + (X,) + ok[7:],                        # out is x
           ok[:6] + (P(0x10000000 + 64),) + ok[7:],       # out overlaps x
           ok[:7] + (P(0x20000000 + 256), BIG)]           # the workspace overlaps out
    _refused(lib, 't2i_laplacian_pyramid', bad)
    _refused(lib, 't2i_laplacian_pyramid', [ok[:7] + (None, BIG), ok[:7] + (Z, 16), ok[:7] + (P(0x30000004), BIG)], rc=-2, word=b'workspace')


def test_swd_descriptors_refuses_bad_arguments(lib):
    ok = (X, 2, 16, 16, 3, Y, 8, Z, 4, 100)
    bad = [(None,) + ok[1:], ok[:5] + (None,) + ok[6:], ok[:7] + (None,) + ok[8:], (X, 0) + ok[2:], (X, 2, 6) + ok[3:],
           (X, 2, 16, 5) + ok[4:], (X, 2, 16, 16, 0) + ok[5:], (X, 2, 16, 16, 5) + ok[5:], ok[:6] + (0,) + ok[7:],
           ok[:8] + (-1, 100), ok[:8] + (90, 100),        # 90 + 2 * 8 rows do not fit in 100
           ok[:8] + (0, 0), ok[:7] + (X, 4, 100), ok[:7] + (Y, 0, 100), (P(0x10000001),) + ok[1:]]
    _refused(lib, 't2i_swd_descriptors', bad)


def test_swd_channel_stats_and_project_refuse_bad_arguments(lib):
    q = lib.lib.t2i_swd_channel_stats_workspace_bytes
    assert q(129, 3) > 0 and q(0, 3) == 0 and q(10, 5) == 0 and q(1 << 40, 3) == 0
    ok = (X, 129, 3, Y, Z, W_, BIG)
    bad = [(None,) + ok[1:], ok[:3] + (None,) + ok[4:], ok[:4] + (None,) + ok[5:], (X, 0) + ok[2:], (X, -5) + ok[2:],
           (X, 129, 0) + ok[3:], (X, 129, 5) + ok[3:], (X, 1 << 40) + ok[2:], ok[:3] + (Y, Y) + ok[5:], ok[:3] + (X, Z) + ok[5:],
           ok[:3] + (P(0x20000004), Z) + ok[5:], ok[:5] + (X, BIG)]
    _refused(lib, 't2i_swd_channel_stats', bad)
    _refused(lib, 't2i_swd_channel_stats', [ok[:5] + (None, BIG), ok[:5] + (W_, 8), ok[:5] + (P(0x40000008), BIG)], rc=-2, word=b'workspace')
    ok = (X, 129, 3, Y, Z, W_, 128, V, 256)
    bad = [(None,) + ok[1:], ok[:3] + (None,) + ok[4:], ok[:4] + (None,) + ok[5:], ok[:5] + (None,) + ok[6:], ok[:7] + (None, 256),
           (X, 0) + ok[2:], (X, 129, 0) + ok[3:], (X, 129, 5) + ok[3:], ok[:6] + (0,) + ok[7:], ok[:8] + (128,),      # rows_pad < rows
           ok[:8] + (384,),                               # no power of two
           ok[:8] + (1 << 30,),                           # S * rows_pad too large
           ok[:7] + (X, 256), ok[:7] + (W_, 256), ok[:7] + (P(0x50000002), 256)]
    _refused(lib, 't2i_swd_project', bad)


def test_sort_and_l1_mean_refuse_bad_arguments(lib):
    bad = [(None, 2, 1024), (X, 0, 1024), (X, -1, 1024), (X, 65536, 1024), (X, 2, 0), (X, 2, -8), (X, 2, 1000), (X, 2, 3),
           (X, 4096, 1 << 20), (P(0x10000004), 2, 1024)]
    _refused(lib, 't2i_segmented_sort_f32', bad)
    q = lib.lib.t2i_sorted_l1_mean_workspace_bytes
    assert q(128, 1000) > 0 and q(0, 1000) == 0 and q(128, 0) == 0
    ok = (X, Y, 128, 1024, 1000, Z, W_, BIG)
    bad = [(None,) + ok[1:], (X, None) + ok[2:], ok[:5] + (None,) + ok[6:], (X, Y, 0) + ok[3:], (X, Y, 128, 0) + ok[4:],
           (X, Y, 128, 1024, 0) + ok[5:], (X, Y, 128, 1024, 1025) + ok[5:], (X, Y, 65536) + ok[3:], ok[:5] + (X,) + ok[6:],
           ok[:5] + (P(0x30000004),) + ok[6:], ok[:6] + (Y, BIG)]
    _refused(lib, 't2i_sorted_l1_mean', bad)
    _refused(lib, 't2i_sorted_l1_mean', [ok[:6] + (None, BIG), ok[:6] + (W_, 8), ok[:6] + (P(0x40000008), BIG)], rc=-2, word=b'workspace')


def test_wrappers_refuse_cpu_and_bad_shapes(lib):
    import torch
    from t2i_amd import kernels as K
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.laplacian_pyramid(torch.zeros(1, 16, 16, 3), 1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.segmented_sort(torch.zeros(2, 8))
    with pytest.raises(ValueError, match='laplacian_pyramid'):
        K.laplacian_pyramid(torch.zeros(1, 16, 16, 3), 3)                 # a coarsest side of 4
    with pytest.raises(ValueError, match='segmented_sort'):
        K.segmented_sort(torch.zeros(2, 12))
    with pytest.raises(ValueError, match='outside'):                     # a centre at side - 3
        K.swd_descriptors(torch.zeros(1, 16, 16, 3), np.array([[[3, 13]]]), torch.zeros(4, 147), 0)
    with pytest.raises(ValueError, match='outside'):
        K.swd_descriptors(torch.zeros(1, 16, 16, 3), np.array([[[2, 5]]]), torch.zeros(4, 147), 0)
    with pytest.raises(ValueError, match='swd_descriptors'):             # the rows do not fit
        K.swd_descriptors(torch.zeros(1, 16, 16, 3), np.array([[[5, 5], [6, 6]]]), torch.zeros(4, 147), 3)
    with pytest.raises(ValueError, match='swd_project'):
        K.swd_project(torch.zeros(5, 147), torch.ones(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64), torch.zeros(147, 4),
                      out=torch.zeros(4, 6))
    assert K.next_pow2(1) == 1 and K.next_pow2(2) == 2 and K.next_pow2(129) == 256 and K.next_pow2(1 << 20) == 1 << 20


# ---- SlicedWasserstein: shapes, the private random stream ----------------------------------------------------------------------
def test_constructor_errors_come_before_any_allocation():
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.swd import SlicedWasserstein
    huge = 1 << 40                                        # an allocation of this many images would fail loudly
    with pytest.raises(ValueError, match='at least 16'):
        SlicedWasserstein((8, 8, 3), huge, 'cpu')
    with pytest.raises(ValueError, match='square'):
        SlicedWasserstein((32, 64, 3), huge, 'cpu')
    with pytest.raises(ValueError, match='channels'):
        SlicedWasserstein((32, 32, 5), huge, 'cpu')


def test_global_numpy_stream_is_untouched_and_the_draw_order_is_stated(capsys):
    import torch
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.evaluation import swd
    np.random.seed(123)
    before = np.random.get_state()
    seen = []
    real_desc = K.swd_descriptors
    try:
        K.swd_descriptors = lambda level, pos, out, row0: seen.append((tuple(level.shape), np.array(pos), row0))
        with K.dry_run():                                 # no launches: shapes and draws only
            sw = swd.SlicedWasserstein((32, 32, 3), 8, 'cpu', seed=7, nhoods=5, repeats=2, dirs=6)
            assert 'bytes' in capsys.readouterr().out and sw.levels == 2 and sw.sides == [32, 16]
            assert [tuple(t.shape) for t in sw.real + sw.gen] == [(40, 147)] * 4
            for _ in range(2):
                sw.add(torch.zeros(4, 32, 32, 3), torch.zeros(4, 32, 32, 3))
            with pytest.raises(ValueError, match='sized for'):
                sw.add(torch.zeros(4, 32, 32, 3), torch.zeros(4, 32, 32, 3))
        dirs = swd.draw_directions(sw.rng, 147, 6)
    finally:
        K.swd_descriptors = real_desc
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    # the order of the draws: per batch, per level, real then generated; then the directions — all from RandomState(seed)
    rs = np.random.RandomState(7)
    want = [(side, rs.randint(3, side - 3, size=(4, 5, 2))) for _ in range(2) for side in (32, 16) for _ in range(2)]
    assert len(seen) == 8 and [s[2] for s in seen] == [0] * 4 + [20] * 4
    for (shape, pos, _), (side, w) in zip(seen, want):
        assert shape == (4, side, side, 3) and pos.dtype == np.int32 and np.array_equal(pos, w)
        assert pos.min() >= 3 and pos.max() < side - 3
    d = rs.randn(147, 6)
    d /= np.sqrt((d * d).sum(0, keepdims=True))
    assert dirs.dtype == np.float32 and np.array_equal(dirs, d.astype(np.float32))
    assert np.abs(np.sqrt((dirs.astype(np.float64) ** 2).sum(0)) - 1).max() <= 1e-6


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


def test_eval_swd_parses_and_is_dispatched():
    import t2i_amd  # noqa: F401
    from t2i_amd.models import cli
    assert cli.EVAL_MODES == ('is', 'fid', 'imd', 'swd')
    args = cli.make_parser('x.yml').parse_args(['--eval', 'swd'])
    assert args.eval == 'swd' and not args.train and not args.visualize

    class Ev(object):
        evaluate_inception = evaluate_fid = evaluate_imd = None

        def evaluate_swd(self):
            return 'swd ran'
    assert cli.run_eval(Ev(), 'swd') == 'swd ran'
    from t2i_amd.evaluation.evaluator import GeneratorEval
    assert callable(GeneratorEval.evaluate_swd)


def test_eval_swd_argument_errors_before_any_device_work(tmp_path, capsys):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.gancls import run
    from t2i_amd.models.pggan import eval_pggan
    from t2i_amd.models.wgancls import run as wrun
    cfg, d = _gancls_cfg(tmp_path)
    with pytest.raises(ValueError, match='synthetic'):
        run.main(['--cfg', cfg, '--eval', 'swd', '--synthetic'])
    with pytest.raises(SystemExit):
        run.main(['--cfg', cfg, '--train', '--eval', 'swd'])
    assert not os.path.exists(d)
    with pytest.raises(ValueError, match='synthetic'):
        wrun.main(['--cfg', cfg, '--eval', 'swd', '--synthetic'])
    capsys.readouterr()
    for stage in ('1', '2'):
        with pytest.raises(SystemExit):
            eval_pggan.main(['--cfg', str(tmp_path / 'none.yml'), '--eval', 'swd', '--stage', stage])
        assert 'stage 3 or later' in capsys.readouterr().err
    with pytest.raises(Exception) as e:                   # stage 3 passes the argument checks: the missing yml is what stops it
        eval_pggan.main(['--cfg', str(tmp_path / 'none.yml'), '--eval', 'swd', '--stage', '3', '--ema'])
    assert not isinstance(e.value, SystemExit)
