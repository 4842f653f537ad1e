"""The Kernel Inception distance, host side (no GPU): the float64 restatement (tests/mmd_cases.py) against brute-force loops and the
published formulation, the band of its inputs against long double, the argument checks of t2i_poly_mmd_sums, the wrapper's and the
metric's refusals, the index tables and the `--eval mmd` / `--mmd-subsets` / `--mmd-subset-size` plumbing of the entry points."""
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

import mmd_cases as MC  # noqa: E402

IDS = dict(ids=lambda s: 'x'.join(str(v) for v in s))


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', MC.SHAPES[:2], **IDS)
def test_restatement_against_brute_force_loops(shape):
    """Python loops over scalars: a second, independent statement of the three sums and of the estimate."""
    NX, NY, D, S, m = shape
    X, Y, ix, iy, ref, band = MC.case(*shape)
    x, y = [[float(v) for v in row] for row in X], [[float(v) for v in row] for row in Y]

    def k(a, b):
        return (sum(p * q for p, q in zip(a, b)) / D + 1.0) ** 3
    for s in range(S):
        xs, ys = [x[i] for i in ix[s]], [y[i] for i in iy[s]]
        pxx = sum(k(xs[i], xs[j]) for i in range(m) for j in range(m) if i < j)
        pyy = sum(k(ys[i], ys[j]) for i in range(m) for j in range(m) if i < j)
        sxy = sum(k(xs[i], ys[j]) for i in range(m) for j in range(m))
        assert np.all(np.abs(ref[s] - [pxx, pyy, sxy]) <= 2.0 * band[s])
        est = 2 * pxx / (m * (m - 1)) + 2 * pyy / (m * (m - 1)) - 2 * sxy / m ** 2
        assert abs(MC.mmd2(ref, m)[s] - est) <= 2.0 * MC.mmd2_band(band, m)[s]


@pytest.mark.parametrize('shape', MC.SHAPES, **IDS)
def test_the_published_formulation_gives_the_same_estimate(shape):
    NX, NY, D, S, m = shape
    X, Y, ix, iy, ref, band = MC.case(*shape)
    kid = float(np.mean(MC.mmd2(ref, m)))
    assert abs(kid - MC.published(X, Y, ix, iy)) <= 2.0 * float(np.mean(MC.mmd2_band(band, m)))


@pytest.mark.parametrize('shape', MC.SHAPES, **IDS)
def test_inputs_meet_the_band_condition(shape):
    """numpy float64 against long double (64-bit mantissa: its own error is 2^-11 of a band): the restatement lies well inside one
    band, so a GPU result within 2 bands of it is within the derived error of the truth.  Measured: at most 0.06 band."""
    NX, NY, D, S, m = shape
    X, Y, ix, iy, ref, band = MC.case(*shape)
    assert X.dtype == Y.dtype == np.float32 and X.shape == (NX, D) and Y.shape == (NY, D) and ix.shape == iy.shape == (S, m)
    assert np.finfo(np.longdouble).nmant >= 63
    exact = MC.sums(X, Y, ix, iy, dtype=np.longdouble)
    ratio = float((np.abs(ref.astype(np.longdouble) - exact) / band).max())
    print('%s: numpy float64 within %.3g band of long double; KID %.6g' % (shape, ratio, float(np.mean(MC.mmd2(ref, m)))))
    assert ratio <= 0.06
    assert np.all(band > 0) and np.all(band <= 1e-9 * np.abs(ref).clip(1e-300))             # a band is tiny against its sum


def test_the_band_does_not_hide_the_mutations():
    """Each listed mutation of the restatement moves the sums it touches by at least 10^6 bands on a shape of the GPU test."""
    X, Y, ix, iy, ref, band = MC.case(130, 129, 100, 4, 65)
    m = 65

    def far(other, cols, ref=ref, band=band):
        return float((np.abs(other - ref) / band)[:, list(cols)].min())
    assert far(MC.sums(X, Y, ix, iy, upper=np.triu(np.ones((m, m), bool), 0)), (0, 1)) > 1e6          # i <= j in place of i < j
    # padded rows not masked: the 64 x 128 tiles of m = 65 hold 63 zero rows and columns, each pair with one is k = coef0^3 = 1
    pad = ref + np.array([65 * 63 + 63 * 62 // 2, 65 * 63 + 63 * 62 // 2, 128 * 128 - 65 * 65], np.float64)
    assert far(pad, (0, 1, 2)) > 1e6
    assert far(MC.sums(X, Y, iy, iy), (0, 2)) > 1e6                                                    # iy read where ix belongs
    assert far(MC.sums(X, Y, ix, iy, gamma=1.0), (0, 1, 2)) > 1e6                                      # gamma dropped
    assert far(MC.sums(X, Y, ix, iy, degree=2), (0, 1, 2)) > 1e6 and far(MC.sums(X, Y, ix, iy, degree=4), (0, 1, 2)) > 1e6
    # a tile below the diagonal counted (without the position mask, which would make it harmless): m = 200, rows 128..191 x columns 0..127
    X, Y, ix, iy, ref, band = MC.case(200, 200, 64, 5, 200)
    up = np.triu(np.ones((200, 200), bool), 1)
    up[128:192, 0:128] = True
    assert far(MC.sums(X, Y, ix, iy, upper=up), (0, 1), ref, band) > 1e6


# ---- the index tables ----------------------------------------------------------------------------------------------------------
def test_index_tables_are_private_and_without_replacement():
    import torch
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation import mmd

    def fed(seed=0, **kw):
        kd = mmd.KernelDistance(4, 'cpu', num_subsets=7, seed=seed, **kw)
        kd.add_real(torch.zeros(50, 4))
        kd.add_gen(torch.zeros(30, 4))
        return kd
    np.random.seed(11)
    before = np.random.get_state()
    ix, iy, m = fed().tables()
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert m == 30 and ix.shape == iy.shape == (7, 30) and ix.dtype == iy.dtype == np.int32
    for s in range(7):
        assert len(set(ix[s])) == 30 and len(set(iy[s])) == 30 and ix[s].min() >= 0 and ix[s].max() < 50
        assert sorted(iy[s]) == list(range(30))                                            # m = N: a permutation
    ix2, iy2, _ = fed().tables()
    assert np.array_equal(ix, ix2) and np.array_equal(iy, iy2)
    ix3, _, _ = fed(seed=1).tables()
    assert not np.array_equal(ix, ix3)
    want_x, want_y = MC.tables(50, 30, 7, 30)
    assert np.array_equal(ix, want_x) and np.array_equal(iy, want_y)
    assert fed(max_subset_size=8).tables()[2] == 8


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
X_, Y_, IX, IY, SUMS, WS, BIG = P(0x10000000), P(0x20000000), P(0x28000000), P(0x29000000), P(0x30000000), P(0x60000000), 1 << 40


def test_entries_are_declared_and_the_abi_version_stays(lib):
    assert lib.ABI_VERSION == 13 and lib.lib.t2i_version() == 13
    for name, nargs in (('t2i_poly_mmd_sums_workspace_bytes', 5), ('t2i_poly_mmd_sums', 16)):
        assert name in lib.SIGNATURES and hasattr(lib.lib, name) and len(lib.SIGNATURES[name][1]) == nargs, name
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    assert 'size_t t2i_poly_mmd_sums_workspace_bytes(' in header and 'int t2i_poly_mmd_sums(' in header
    build = open(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 'build.sh')).read()
    assert build.count('t2i_mmd') == 2 and ' t2i_mmd ' in build and '"$OUT/t2i_mmd.o"' in build     # the compile list and the link line
    assert os.path.exists(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 't2i_mmd.hip'))


def test_the_workspace_query_grows_with_the_subsets_and_their_size(lib):
    from t2i_amd import kernels as K
    ws = lib.lib.t2i_poly_mmd_sums_workspace_bytes
    assert ws(2, 2, 1, 1, 2) > 0
    assert ws(5000, 5000, 64, 1, 1000) < ws(5000, 5000, 64, 10, 1000) < ws(5000, 5000, 64, 100, 1000)
    assert ws(5000, 5000, 64, 10, 100) < ws(5000, 5000, 64, 10, 500) < ws(5000, 5000, 64, 10, 1000) < ws(5000, 5000, 64, 10, 5000)
    for S, m in ((1, 2), (3, 64), (3, 65), (4, 129), (100, 1000), (7, 4097)):
        assert ws(5000, 5000, 64, S, m) == (8 * K.poly_mmd_items(S, m) + 255) // 256 * 256, (S, m)
    # m = 1000: 16 row tiles x 8 column tiles; the symmetric products keep 72 of the 128, about two thirds of the work in all
    assert K.poly_mmd_items(1, 1000) == 72 + 72 + 128
    assert K.poly_mmd_items(1, 64) == 3 and K.poly_mmd_items(1, 65) == 2 + 2 + 2 and K.poly_mmd_items(1, 129) == 5 + 5 + 6
    for bad in ((0, 5, 64, 1, 2), (5, 0, 64, 1, 2), (5, 5, 0, 1, 2), (5, 5, 64, 0, 2), (5, 5, 64, 1, 1), (5, 5, 64, 1, -3),
                (1 << 26, 5, 2048, 1, 2), (5, 1 << 26, 2048, 1, 2)):
        assert ws(*bad) == 0, bad
    assert ws((1 << 26) - 1, 5, 2048, 1, 2) > 0
    # the cap of 2^30 work items
    assert K.poly_mmd_items(3947580, 1000) <= 1 << 30 < K.poly_mmd_items(3947581, 1000)
    assert ws(5, 5, 64, 3947580, 1000) > 0 and ws(5, 5, 64, 3947581, 1000) == 0
    assert ws(5, 5, 64, 1, (1 << 31) - 1) == 0


def test_poly_mmd_sums_refuses_bad_arguments(lib):
    ok = (X_, 100, Y_, 300, 64, IX, IY, 4, 65, 3, 1.0 / 64, 1.0, SUMS, WS, BIG)
    need = lib.lib.t2i_poly_mmd_sums_workspace_bytes(100, 300, 64, 4, 65)
    assert need > 0
    fn = lib.lib.t2i_poly_mmd_sums

    def put(i, v, base=ok):
        return base[:i] + (v,) + base[i + 1:]
    same = put(2, X_, put(3, 100))                                                                        # X and Y one tensor: allowed
    bad = [put(0, None), put(2, None), put(5, None), put(6, None), put(12, None), put(13, None),          # a NULL pointer
           put(1, 0), put(1, -5), put(3, 0), put(3, -1), put(4, 0), put(4, -64), put(7, 0), put(7, -2),   # NX, NY, D, S
           put(8, 1), put(8, 0), put(8, -4),                                                              # m < 2
           put(9, 0), put(9, 9), put(9, -1),                                                              # degree outside 1..8
           put(10, float('nan')), put(10, float('inf')), put(11, float('nan')), put(11, -float('inf')),   # gamma, coef0
           put(1, 1 << 26, put(4, 2048)), put(3, 1 << 26, put(4, 2048)),                                  # NX D, NY D = 2^31 * 64
           put(7, 3947581, put(8, 1000)), put(8, (1 << 31) - 1),                                          # more than 2^30 work items
           put(14, 0), put(14, need - 1),                                                                 # a short workspace
           put(12, X_), put(12, P(0x20000000 + 4096)), put(12, IX), put(12, P(0x29000000 + 8)),           # sums on an input or a table
           put(12, WS), put(12, P(0x60000000 + need - 8)),                                                   # sums inside the workspace
           put(13, X_), put(13, Y_), put(13, IX), put(13, IY), put(13, SUMS),                             # the workspace on the others
           put(12, X_, same),
           put(0, P(0x10000002)), put(2, P(0x20000001)), put(5, P(0x28000002)), put(6, P(0x29000001)), put(12, P(0x30000004)),
           put(13, P(0x60000004))]                                                                        # misaligned
    for args in bad:
        assert fn(*args, None) == -1, ' '.join(str(getattr(a, 'value', a)) for a in args)
        msg = lib.lib.t2i_last_error()
        assert b't2i_poly_mmd_sums' in msg and b'bad argument' in msg, (args, msg)
    assert b'NX=100 NY=300 D=64 S=4 m=65' in lib.lib.t2i_last_error()


def test_the_wrapper_refuses_on_the_host(lib):
    import torch
    from t2i_amd import kernels as K
    x, y = torch.zeros(10, 16), torch.zeros(30, 16)
    ix, iy = torch.zeros((3, 5), dtype=torch.int32), torch.zeros((3, 5), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.poly_mmd_sums(x, y, ix, iy)
    with K.dry_run():
        out = K.poly_mmd_sums(x, y, ix, iy)
        assert out.dtype == torch.float64 and tuple(out.shape) == (3, 3)
        assert tuple(K.poly_mmd_sums(x, x, ix, ix, degree=8, gamma=0.5, coef0=-1.0, check_indices=False).shape) == (3, 3)
        for bx, by in ((x.double(), y.double()), (x.t().contiguous().t(), y), (x, torch.zeros(30, 15)), (x[0], y), (torch.zeros(0, 16), y),
                       (x, torch.zeros(0, 16)), (torch.zeros(10, 0), torch.zeros(30, 0))):
            with pytest.raises(ValueError, match='poly_mmd_sums'):
                K.poly_mmd_sums(bx, by, ix, iy)
        for bix, biy in ((ix.long(), iy.long()), (ix.float(), iy), (ix, iy.t().contiguous().t()), (ix, iy[:, :4].contiguous()),
                         (ix[:2], iy), (ix[0], iy[0]), (ix[:, :1].contiguous(), iy[:, :1].contiguous()),
                         (torch.zeros((0, 5), dtype=torch.int32), torch.zeros((0, 5), dtype=torch.int32))):
            with pytest.raises(ValueError, match='poly_mmd_sums'):
                K.poly_mmd_sums(x, y, bix, biy)
        for kw in (dict(degree=0), dict(degree=9), dict(gamma=float('nan')), dict(coef0=float('inf'))):
            with pytest.raises(ValueError, match='degree'):
                K.poly_mmd_sums(x, y, ix, iy, **kw)


def test_kernel_distance_refusals_and_growth():
    import torch
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.evaluation import mmd
    for kw, word in ((dict(num_subsets=0), 'num_subsets'), (dict(num_subsets=10001), 'num_subsets'), (dict(num_subsets=2.5), 'num_subsets'),
                     (dict(max_subset_size=1), 'max_subset_size'), (dict(degree=0), 'degree'), (dict(degree=9), 'degree'),
                     (dict(gamma=float('inf')), 'finite'), (dict(coef0=float('nan')), 'finite')):
        with pytest.raises(ValueError, match=word):
            mmd.KernelDistance(16, 'cpu', **kw)
    with pytest.raises(ValueError, match='dim'):
        mmd.KernelDistance(0, 'cpu')
    kd = mmd.KernelDistance(2048, 'cpu')
    assert (kd.num_subsets, kd.max_subset_size, kd.degree, kd.gamma, kd.coef0, kd.seed) == (100, 1000, 3, 1.0 / 2048, 1.0, 0)
    kd = mmd.KernelDistance(4, 'cpu', num_subsets=3)
    with pytest.raises(ValueError, match='KernelDistance.add_real'):
        kd.add_real(torch.zeros(3, 5))
    rows = torch.arange(300 * 4, dtype=torch.float32).reshape(300, 4)
    for a, b in ((0, 7), (7, 260), (260, 300)):                                                           # past the first 256 rows
        kd.add_real(rows[a:b])
    kd.add_gen(rows[:1])
    assert kd.real.n == 300 and torch.equal(kd.real.rows(), rows) and type(kd.real).__module__.endswith('evaluation.prdc')
    with K.dry_run():
        with pytest.raises(ValueError, match='1 generated rows'):
            kd.finalize()
        kd.add_gen(torch.full((1, 4), float('nan')))
        with pytest.raises(ValueError, match='generated feature is not finite'):
            kd.finalize()
    est = mmd.estimates(np.array([[3.0, 6.0, 8.0]]), 2)
    assert est.shape == (1,) and est[0] == 2 * 3.0 / 2 + 2 * 6.0 / 2 - 2 * 8.0 / 4


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


def test_eval_mmd_parses_and_is_dispatched():
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation import mmd
    from t2i_amd.models import cli
    assert cli.EVAL_MODES == ('is', 'fid', 'imd', 'swd') and cli.PAIR_MODES == ('msssim',) and cli.FEATURE_MODES == ('prdc',)
    assert cli.SUBSET_MODES == ('mmd',) and cli.MAX_SUBSETS == mmd.MAX_SUBSETS == 10000
    ap = cli.make_parser('x.yml')
    args = ap.parse_args(['--eval', 'mmd'])
    assert args.eval == 'mmd' and args.mmd_subsets is None and args.mmd_subset_size is None and args.prdc_k is None
    args = ap.parse_args(['--eval', 'mmd', '--mmd-subsets', '10', '--mmd-subset-size', '500'])
    assert cli.subsets_of(args) == (10, 500)
    assert ap.parse_args(['--eval', 'fid']).mmd_subsets is None

    class Ev(object):                                     # run_eval looks up the requested mode's method only
        def evaluate_mmd(self, num_subsets, max_subset_size):
            return 'mmd ran on %d subsets of %d' % (num_subsets, max_subset_size)

        def evaluate_prdc(self, nearest_k):
            return 'prdc ran with k = %d' % nearest_k

        def evaluate_fid(self):
            return 'fid ran'
    assert cli.run_eval(Ev(), 'mmd') == 'mmd ran on 100 subsets of 1000'
    assert cli.run_eval(Ev(), 'mmd', None, None, (10, None)) == 'mmd ran on 10 subsets of 1000'
    assert cli.run_eval(Ev(), 'mmd', subsets=(None, 64)) == 'mmd ran on 100 subsets of 64'
    assert cli.run_eval(Ev(), 'prdc', None, 3) == 'prdc ran with k = 3' and cli.run_eval(Ev(), 'fid') == 'fid ran'
    from t2i_amd.evaluation.evaluator import GeneratorEval
    assert callable(GeneratorEval.evaluate_mmd)
    for kw in (dict(num_subsets=0), dict(num_subsets=10001), dict(max_subset_size=1)):
        with pytest.raises(ValueError, match='evaluate_mmd'):
            GeneratorEval.evaluate_mmd(None, **kw)        # refused before the Inception net is loaded


def test_eval_mmd_argument_errors_before_any_device_work(tmp_path, capsys):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.gancls import run
    from t2i_amd.models.pggan import eval_pggan
    from t2i_amd.models.stackgan.stageI import run as run1
    from t2i_amd.models.stackgan.stageII import run as run2
    from t2i_amd.models.wgancls import run as wrun
    cfg, d = _gancls_cfg(tmp_path)
    none = str(tmp_path / 'none.yml')
    for main in (run.main, run1.main, run2.main, wrun.main):
        for flag, value in (('--mmd-subsets', '10'), ('--mmd-subset-size', '100')):
            for argv in ([flag, value], ['--eval', 'fid', flag, value], ['--train', flag, value], ['--eval', 'prdc', flag, value]):
                with pytest.raises(SystemExit) as e:
                    main(['--cfg', cfg] + argv)
                assert e.value.code == 2 and '%s needs --eval mmd' % flag in capsys.readouterr().err
        for n in ('0', '10001', '-2'):
            with pytest.raises(SystemExit) as e:
                main(['--cfg', cfg, '--eval', 'mmd', '--mmd-subsets', n])
            assert e.value.code == 2 and '--mmd-subsets must be in 1..10000' in capsys.readouterr().err
        for n in ('1', '0', '-7'):
            with pytest.raises(SystemExit) as e:
                main(['--cfg', cfg, '--eval', 'mmd', '--mmd-subset-size', n])
            assert e.value.code == 2 and '--mmd-subset-size must be at least 2' in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            main(['--cfg', cfg, '--eval', 'kid'])                                          # the mode is spelled mmd
        assert e.value.code == 2 and 'invalid choice' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            main(['--cfg', cfg, '--eval', 'mmd', '--mmd-subsets', 'ten'])
        with pytest.raises(SystemExit):
            main(['--cfg', cfg, '--train', '--eval', 'mmd'])
        assert not os.path.exists(d)
    with pytest.raises(ValueError, match='synthetic'):   # --eval mmd is accepted: the next check is what stops the run
        run.main(['--cfg', cfg, '--eval', 'mmd', '--mmd-subsets', '10', '--mmd-subset-size', '2', '--synthetic'])
    for main in (run1.main, run2.main):
        with pytest.raises(ValueError, match='synthetic'):
            main(['--cfg', cfg, '--eval', 'mmd', '--synthetic'])
    assert not os.path.exists(d)
    with pytest.raises(ValueError, match='synthetic'):   # (the wgancls entry point creates its directories first, as the reference does)
        wrun.main(['--cfg', cfg, '--eval', 'mmd', '--synthetic'])
    capsys.readouterr()
    for argv, word in ((['--eval', 'is', '--mmd-subsets', '3'], '--mmd-subsets needs --eval mmd'),
                       (['--eval', 'prdc', '--mmd-subset-size', '30'], '--mmd-subset-size needs --eval mmd'),
                       (['--eval', 'mmd', '--mmd-subsets', '10001'], '--mmd-subsets must be in 1..10000'),
                       (['--eval', 'mmd', '--mmd-subset-size', '1'], '--mmd-subset-size must be at least 2'),
                       (['--eval', 'kid'], 'invalid choice')):
        with pytest.raises(SystemExit) as e:
            eval_pggan.main(['--cfg', none] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
    for argv in (['--stage', '1', '--ema'], ['--mmd-subsets', '3', '--mmd-subset-size', '2', '--stage', '7']):
        with pytest.raises(Exception) as e:               # these pass the argument checks: the missing yml is what stops them
            eval_pggan.main(['--cfg', none, '--eval', 'mmd'] + argv)
        assert not isinstance(e.value, SystemExit)
