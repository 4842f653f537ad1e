"""Precision, recall, density and coverage, host side (no GPU): the float64 restatement (tests/prdc_cases.py) against brute-force
loops, the band condition of its inputs, the argument checks of t2i_knn_dist2 and t2i_ball_counts, the wrappers' and the metric's
refusals, and the `--eval prdc` / `--prdc-k` plumbing of the entry points."""
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

import prdc_cases as PC  # noqa: E402


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_restatement_against_brute_force_loops():
    """The (5, 7, 3, 1) case by Python loops over scalars: a second, independent statement of the four definitions."""
    M, N, D, k = 5, 7, 3, 1
    R, G, ref = PC.case(M, N, D, k)
    r, g = [[float(v) for v in row] for row in R], [[float(v) for v in row] for row in G]

    def d2(a, b):
        return sum((x - y) * (x - y) for x, y in zip(a, b))

    def radius(rows, i):
        return sorted(d2(rows[i], rows[j]) for j in range(len(rows)) if j != i)[k - 1]
    r2_real, r2_gen = [radius(r, n) for n in range(N)], [radius(g, m) for m in range(M)]
    cnt_gen = [sum(d2(g[m], r[n]) <= r2_real[n] for n in range(N)) for m in range(M)]
    cnt_real = [sum(d2(r[n], g[m]) <= r2_gen[m] for m in range(M)) for n in range(N)]
    covered = [min(d2(r[n], g[m]) for m in range(M)) <= r2_real[n] for n in range(N)]
    assert np.allclose(ref['r2_real'], r2_real, rtol=1e-14, atol=0) and np.allclose(ref['r2_gen'], r2_gen, rtol=1e-14, atol=0)
    assert list(ref['cnt_gen']) == cnt_gen and list(ref['cnt_real']) == cnt_real and list(ref['covered']) == covered
    assert ref['precision'] == sum(c > 0 for c in cnt_gen) / M and ref['recall'] == sum(c > 0 for c in cnt_real) / N
    assert ref['density'] == sum(cnt_gen) / (k * M) and ref['coverage'] == sum(covered) / N


def test_knn_restatement_skips_by_index_and_sorts():
    X = np.array([[0.0], [0.0], [3.0], [1.0]], np.float32)
    val, idx = PC.knn(X, X, 2, exclude_self=True)
    assert np.array_equal(val, [[0, 1], [0, 1], [4, 9], [1, 1]]) and idx[0, 0] == 1 and idx[1, 0] == 0        # the duplicate is a neighbour
    val, _ = PC.knn(X, X, 2)
    assert np.array_equal(val, [[0, 0], [0, 0], [0, 4], [0, 1]])
    Q, R = PC.integer_sets(17, 35, 4)
    assert np.array_equal(PC.dist2(Q, R), PC.gram_dist2(Q, R)) and np.array_equal(PC.dist2(Q, R), np.round(PC.dist2(Q, R)))
    assert not np.array_equal(PC.dist2(Q, R)[:17, :17], PC.dist2(Q, R)[:17, :17].T)                            # asymmetric


@pytest.mark.parametrize('shape', PC.SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_inputs_meet_the_band_condition(shape):
    """The condition under which the GPU tests may demand equality: the restatement has no decision within 2 bands of its
    threshold.  (Measured: the closest decision of the seven shapes is 4.75e7 bands away, on (100, 257, 2048, 5); a numpy float64
    Gram form is within 0.43 band of the direct form, the worst on (64, 64, 4, 3).)"""
    M, N, D, k = shape
    R, G, ref = PC.case(*shape)
    assert R.dtype == G.dtype == np.float32 and R.shape == (N, D) and G.shape == (M, D)
    margin = PC.decision_margin(R, G, k, ref)
    gram = float((np.abs(PC.gram_dist2(G, R) - ref['d_gr']) / PC.band(G, R)).max())
    print('%s: closest decision %.3g bands, numpy Gram form %.3g band, precision %.4f recall %.4f density %.4f coverage %.4f' % (
        shape, margin, gram, ref['precision'], ref['recall'], ref['density'], ref['coverage']))
    assert margin > 2.0
    assert gram <= 0.43
    if M > k:                                              # (recall is undefined for the one-query shape: it has no radius)
        assert 0.95 <= ref['precision'] <= 1.0 and 0.655 <= ref['recall'] <= 0.845                            # not trivial
        assert 1.1 <= ref['density'] <= 1.5 and 0.57 <= ref['coverage'] <= 0.98


def test_duplicate_inputs_have_genuine_radii():
    R, G = PC.duplicates()
    ref = PC.restate(R, G, 3)
    own = 4.0 * 48 * 2.0 ** -53 * 2.0 * (R.astype(np.float64) ** 2).sum(1)
    assert (ref['r2_real'] / own).min() >= 2e12                                  # k = 3: beyond the copy, a genuine distance
    assert np.all(ref['dmin_gen'][:10] == 0.0) and np.all(ref['cnt_gen'][:10] >= 2)
    assert np.array_equal(R[30:], R[:30]) and np.array_equal(G[:10], R[:10])


# ---- the entries refuse bad arguments before any launch ---------------------------------------------------------------------------
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
Q_, R_, R2, OUT, CNT, DMIN, WS, BIG = (P(0x10000000), P(0x20000000), P(0x28000000), P(0x30000000), P(0x31000000), P(0x32000000),
                                       P(0x60000000), 1 << 40)


def _refused(lib, name, calls, rc=-1, word=b'bad argument'):
    fn = getattr(lib.lib, name)
    for args in calls:
        assert fn(*args, None) == rc, (name, args)
        msg = lib.lib.t2i_last_error()
        assert name.encode() in msg and word in msg, (name, args, msg)


def test_entries_are_declared_and_the_abi_version_stays(lib):
    assert lib.ABI_VERSION == 13 and lib.lib.t2i_version() == 13
    for name, nargs in (('t2i_knn_dist2_workspace_bytes', 5), ('t2i_knn_dist2', 12), ('t2i_ball_counts_workspace_bytes', 4),
                        ('t2i_ball_counts', 12)):
        assert name in lib.SIGNATURES and hasattr(lib.lib, name) and len(lib.SIGNATURES[name][1]) == nargs, name
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    from t2i_amd import kernels as K
    assert '#define T2I_KNN_MAX_K %d' % K.KNN_MAX_K in header and K.KNN_MAX_K == 8
    build = open(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 'build.sh')).read()
    assert build.count('t2i_knn') == 2                     # the compile list and the link line


def test_workspace_queries_grow_with_the_queries_and_the_segments(lib):
    for q, tail in ((lib.lib.t2i_knn_dist2_workspace_bytes, (5,)), (lib.lib.t2i_ball_counts_workspace_bytes, ())):
        def ws(M, N, D, segments):
            return q(M, N, D, *tail, segments)
        assert ws(1, 2, 1, 1) > 0
        assert ws(100, 300, 64, 1) < ws(1000, 300, 64, 1) < ws(10000, 300, 64, 1)
        assert ws(100, 300, 64, 1) < ws(100, 300, 64, 2) < ws(100, 300, 64, 7) < ws(100, 300, 64, 300)
        assert ws(100, 300, 64, 0) in [ws(100, 300, 64, s) for s in range(1, 6)]          # 0: the library's choice, one per tile at most
        assert ws(0, 300, 64, 1) == 0 and ws(100, 0, 64, 1) == 0 and ws(100, 300, 0, 1) == 0
        assert ws(100, 300, 64, -1) == 0 and ws(100, 300, 64, 301) == 0
        assert ws(1 << 26, 300, 2048, 1) == 0              # 2^26 * 2048 = 2^31 * 64
        assert ws((1 << 26) - 1, 300, 2048, 1) > 0
    assert lib.lib.t2i_knn_dist2_workspace_bytes(100, 300, 64, 0, 1) == 0 and lib.lib.t2i_knn_dist2_workspace_bytes(100, 300, 64, 9, 1) == 0


def test_knn_dist2_refuses_bad_arguments(lib):
    ok = (Q_, 100, R_, 300, 64, 5, 0, 2, OUT, WS, BIG)
    need = lib.lib.t2i_knn_dist2_workspace_bytes(100, 300, 64, 5, 2)

    def put(i, v, base=ok):
        return base[:i] + (v,) + base[i + 1:]
    same = (Q_, 300, Q_, 300, 64, 5, 1, 2, OUT, WS, BIG)                                                 # exclude_self, Q = R
    bad = [put(0, None), put(2, None), put(8, None), put(9, None),                                        # a NULL pointer
           put(1, 0), put(1, -5), put(3, 0), put(3, -1), put(4, 0), put(4, -64),                          # M, N, D
           put(5, 0), put(5, 9), put(5, -1),                                                              # k outside 1..8
           (Q_, 100, R_, 4, 64, 5, 0, 1, OUT, WS, BIG),                                                   # k > N
           (Q_, 5, Q_, 5, 64, 5, 1, 1, OUT, WS, BIG),                                                     # k > N - exclude_self
           put(6, 2), put(6, -1), put(6, 1),                                                              # exclude_self; 1 with M != N
           put(7, -1), put(7, 301),                                                                       # segments
           put(1, 1 << 26, put(4, 2048)), put(3, 1 << 26, put(4, 2048)),                                  # M D, N D = 2^31 * 64
           put(1, 1 << 61, put(4, 1)),                                                                    # M D and M k beyond range
           put(10, 0), put(10, need - 1),                                                                 # a short workspace
           put(8, Q_), put(8, P(0x20000000 + 4096)), put(9, Q_), put(9, R_), put(9, OUT),                 # out / workspace on an input
           put(8, P(0x60000000 + 256)),                                                                   # out inside the workspace
           put(8, Q_, same), put(7, 301, same),
           put(0, P(0x10000002)), put(2, P(0x20000001)), put(8, P(0x30000004)), put(9, P(0x60000004))]    # misaligned
    _refused(lib, 't2i_knn_dist2', bad)
    assert b'k=5' in lib.lib.t2i_last_error() and b'M=100 N=300 D=64' in lib.lib.t2i_last_error()


def test_ball_counts_refuses_bad_arguments(lib):
    ok = (Q_, 100, R_, 300, 64, R2, 2, CNT, DMIN, WS, BIG)
    need = lib.lib.t2i_ball_counts_workspace_bytes(100, 300, 64, 2)

    def put(i, v, base=ok):
        return base[:i] + (v,) + base[i + 1:]
    bad = [put(0, None), put(2, None), put(5, None), put(7, None), put(8, None), put(9, None),            # a NULL pointer
           put(1, 0), put(1, -5), put(3, 0), put(3, -1), put(4, 0), put(4, -64),                          # M, N, D
           put(6, -1), put(6, 301),                                                                       # segments
           put(1, 1 << 26, put(4, 2048)), put(3, 1 << 26, put(4, 2048)),                                  # M D, N D = 2^31 * 64
           put(10, 0), put(10, need - 1),                                                                 # a short workspace
           put(7, Q_), put(7, R_), put(7, R2), put(8, Q_), put(8, P(0x20000000 + 8)), put(8, R2),         # an output on an input
           put(9, Q_), put(9, R_), put(9, R2),                                                            # the workspace on an input
           put(8, CNT), put(9, CNT), put(9, DMIN), put(8, P(0x31000000 + 8)),                             # outputs on each other
           put(0, P(0x10000002)), put(2, P(0x20000001)), put(5, P(0x28000004)), put(7, P(0x31000002)), put(8, P(0x32000004)),
           put(9, P(0x60000004))]                                                                         # misaligned
    _refused(lib, 't2i_ball_counts', bad)
    assert b'M=100 N=300 D=64' in lib.lib.t2i_last_error()


def test_wrappers_refuse_on_the_host(lib):
    import torch
    from t2i_amd import kernels as K
    q, r = torch.zeros(10, 16), torch.zeros(30, 16)
    r2 = torch.zeros(30, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.knn_dist2(q, r, 3)
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.ball_counts(q, r, r2)
    with K.dry_run():
        out = K.knn_dist2(q, r, 3)
        assert out.dtype == torch.float64 and tuple(out.shape) == (10, 3)
        assert K.knn_dist2(q, r, 3, out=out) is out
        assert tuple(K.knn_dist2(r, r, 8, exclude_self=True, segments=30).shape) == (30, 8)
        cnt, dmin = K.ball_counts(q, r, r2, segments=2)
        assert cnt.dtype == torch.int32 and dmin.dtype == torch.float64 and tuple(cnt.shape) == tuple(dmin.shape) == (10,)
        for bad_q, bad_r in ((q.double(), r.double()), (q.t().contiguous().t(), r), (q, torch.zeros(30, 15)), (q[0], r),
                             (torch.zeros(0, 16), r), (q, torch.zeros(0, 16))):
            with pytest.raises(ValueError, match='knn_dist2'):
                K.knn_dist2(bad_q, bad_r, 1)
            with pytest.raises(ValueError, match='ball_counts'):
                K.ball_counts(bad_q, bad_r, r2)
        for k, kw in ((0, {}), (9, {}), (3, dict(exclude_self=True)), (3, dict(segments=-1)), (3, dict(segments=31)),
                      (3, dict(out=torch.zeros(10, 3))), (3, dict(out=torch.zeros(10, 4, dtype=torch.float64)))):
            with pytest.raises(ValueError, match='knn_dist2'):
                K.knn_dist2(q, r, k, **kw)
        with pytest.raises(ValueError, match='knn_dist2'):
            K.knn_dist2(r[:3], r[:3], 3, exclude_self=True)                                               # k > N - 1
        for bad_r2 in (r2.float(), torch.zeros(29, dtype=torch.float64), torch.zeros(60, dtype=torch.float64)[::2]):
            with pytest.raises(ValueError, match='r2'):
                K.ball_counts(q, r, bad_r2)
        with pytest.raises(ValueError, match='ball_counts'):
            K.ball_counts(q, r, r2, segments=31)


def test_manifold_metrics_refusals_and_growth():
    import torch
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.evaluation import prdc
    for k in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match='nearest_k'):
            prdc.ManifoldMetrics(16, 'cpu', nearest_k=k)
    assert prdc.ManifoldMetrics(16, 'cpu').nearest_k == 5
    mm = prdc.ManifoldMetrics(4, 'cpu', nearest_k=3)
    with pytest.raises(ValueError, match='add_real'):
        mm.add_real(torch.zeros(3, 5))
    rows = torch.arange(300 * 4, dtype=torch.float32).reshape(300, 4)
    for a, b in ((0, 7), (7, 260), (260, 300)):                                                           # past the first 256 rows
        mm.add_real(rows[a:b])
    mm.add_gen(rows[:3])
    assert mm.real.n == 300 and torch.equal(mm.real.rows(), rows) and mm.real.rows().is_contiguous() and mm.real.buf.shape[0] >= 512
    with K.dry_run():
        with pytest.raises(ValueError, match='3 generated rows'):
            mm.finalize()
        mm.add_gen(torch.full((1, 4), float('nan')))
        with pytest.raises(ValueError, match='generated feature is not finite'):
            mm.finalize()
    out = prdc.ratios(np.array([0, 2, 5], np.int32), np.array([1, 0, 0, 3], np.int32), np.array([True, False, True, True]), 2)
    assert out == dict(precision=2 / 3, recall=0.5, density=7 / 6, coverage=0.75, nearest_k=2, n_real=4, n_gen=3)


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


def test_eval_prdc_parses_and_is_dispatched():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.models import cli
    assert cli.EVAL_MODES == ('is', 'fid', 'imd', 'swd') and cli.PAIR_MODES == ('msssim',) and cli.FEATURE_MODES == ('prdc',)
    assert cli.KNN_MAX_K == K.KNN_MAX_K
    ap = cli.make_parser('x.yml')
    args = ap.parse_args(['--eval', 'prdc'])
    assert args.eval == 'prdc' and args.prdc_k is None and args.msssim_pairs is None and not args.train and not args.visualize
    assert ap.parse_args(['--eval', 'prdc', '--prdc-k', '3']).prdc_k == 3
    assert ap.parse_args(['--eval', 'fid']).prdc_k is None

    class Ev(object):                                     # run_eval looks up the requested mode's method only
        def evaluate_prdc(self, nearest_k):
            return 'prdc ran with k = %d' % nearest_k

        def evaluate_msssim(self, pairs):
            return 'msssim ran on %s pairs' % pairs

        def evaluate_fid(self):
            return 'fid ran'
    assert cli.run_eval(Ev(), 'prdc') == 'prdc ran with k = 5'
    assert cli.run_eval(Ev(), 'prdc', None, 3) == 'prdc ran with k = 3' and cli.run_eval(Ev(), 'prdc', nearest_k=8) == 'prdc ran with k = 8'
    assert cli.run_eval(Ev(), 'fid') == 'fid ran' and cli.run_eval(Ev(), 'msssim', 'caption') == 'msssim ran on caption pairs'
    from t2i_amd.evaluation.evaluator import GeneratorEval
    assert callable(GeneratorEval.evaluate_prdc)
    with pytest.raises(ValueError, match='nearest_k'):
        GeneratorEval.evaluate_prdc(None, nearest_k=9)    # refused before the Inception net is loaded


def test_eval_prdc_argument_errors_before_any_device_work(tmp_path, capsys):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.gancls import run
    from t2i_amd.models.pggan import eval_pggan
    from t2i_amd.models.stackgan.stageI import run as run1
    from t2i_amd.models.stackgan.stageII import run as run2
    from t2i_amd.models.wgancls import run as wrun
    cfg, d = _gancls_cfg(tmp_path)
    none = str(tmp_path / 'none.yml')
    for main in (run.main, run1.main, run2.main, wrun.main):
        for argv in (['--prdc-k', '3'], ['--eval', 'fid', '--prdc-k', '3'], ['--train', '--prdc-k', '5'], ['--eval', 'msssim', '--prdc-k', '5']):
            with pytest.raises(SystemExit) as e:
                main(['--cfg', cfg] + argv)
            assert e.value.code == 2 and '--prdc-k needs --eval prdc' in capsys.readouterr().err
        for k in ('0', '9', '-2'):
            with pytest.raises(SystemExit) as e:
                main(['--cfg', cfg, '--eval', 'prdc', '--prdc-k', k])
            assert e.value.code == 2 and '--prdc-k must be in 1..8' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            main(['--cfg', cfg, '--eval', 'prdc', '--prdc-k', 'five'])
        with pytest.raises(SystemExit):
            main(['--cfg', cfg, '--train', '--eval', 'prdc'])
        assert not os.path.exists(d)
    with pytest.raises(ValueError, match='synthetic'):
        run.main(['--cfg', cfg, '--eval', 'prdc', '--prdc-k', '3', '--synthetic'])
    assert not os.path.exists(d)
    with pytest.raises(ValueError, match='synthetic'):   # (the wgancls entry point creates its directories first, as the reference does)
        wrun.main(['--cfg', cfg, '--eval', 'prdc', '--synthetic'])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        eval_pggan.main(['--cfg', none, '--eval', 'is', '--prdc-k', '3'])
    assert e.value.code == 2 and '--prdc-k needs --eval prdc' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        eval_pggan.main(['--cfg', none, '--eval', 'prdc', '--prdc-k', '9'])
    assert e.value.code == 2 and '--prdc-k must be in 1..8' in capsys.readouterr().err
    for argv in (['--stage', '1', '--ema'], ['--prdc-k', '3', '--stage', '7']):
        with pytest.raises(Exception) as e:               # these pass the argument checks: the missing yml is what stops them
            eval_pggan.main(['--cfg', none, '--eval', 'prdc'] + argv)
        assert not isinstance(e.value, SystemExit)
