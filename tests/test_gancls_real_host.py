"""GAN-CLS on real data, host side (no GPU): the mode errors of models/gancls/run.py, the added C symbol t2i_bn_infer within
ABI version 13, its argument checks, and the float64 NumPy statement of the inference batch norm that tests/test_gancls_real_gpu.py
uses as its oracle."""
import ctypes
import os
import sys

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CFG = os.path.join(ROOT, 'text-to-image_amd', 'models', 'gancls', 'cfg', 'flowers.yml')

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3


# ---- the float64 statement of kernels.bn_infer ---------------------------------------------------------------------------------
def np_act(v, act, alpha):
    if act == ACT_LRELU:
        return np.where(v > 0, v, alpha * v)
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_TANH:
        return np.tanh(v)
    return v


def np_bn_infer(x, gamma, beta, mm, mv, eps=1e-5, act=ACT_NONE, alpha=0.2, residual=None, res_act=ACT_NONE, res_alpha=0.2):
    """y = res_act(residual + act((x - mm) / sqrt(mv + eps) * gamma + beta)) in float64, channels last."""
    x, gamma, beta, mm, mv = (np.asarray(a, np.float64) for a in (x, gamma, beta, mm, mv))
    y = np_act((x - mm) / np.sqrt(mv + eps) * gamma + beta, act, alpha)
    if residual is not None:
        y = np_act(np.asarray(residual, np.float64) + y, res_act, res_alpha)
    return y


def test_np_bn_infer_statement():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 2, 2, 5))
    g, b, mm, mv = rng.standard_normal(5), rng.standard_normal(5), rng.standard_normal(5), rng.uniform(0.5, 2, 5)
    y = np_bn_infer(x, g, b, mm, mv, eps=1e-3)
    for c in range(5):                                   # per channel, spelled out
        np.testing.assert_allclose(y[..., c], (x[..., c] - mm[c]) / np.sqrt(mv[c] + 1e-3) * g[c] + b[c], rtol=1e-14, atol=1e-14)
    # identity statistics: the activation alone
    ones, zeros = np.ones(5), np.zeros(5)
    for act, want in ((ACT_NONE, x), (ACT_RELU, np.maximum(x, 0)), (ACT_LRELU, np.where(x > 0, x, 0.3 * x)), (ACT_TANH, np.tanh(x))):
        np.testing.assert_allclose(np_bn_infer(x, ones, zeros, zeros, ones, eps=0.0, act=act, alpha=0.3), want, rtol=1e-15, atol=0)
    # the residual join: res_act(residual + act(norm)), the activation of the norm applied first
    r = rng.standard_normal(x.shape)
    got = np_bn_infer(x, g, b, mm, mv, act=ACT_RELU, residual=r, res_act=ACT_LRELU, res_alpha=0.1)
    inner = np.maximum(np_bn_infer(x, g, b, mm, mv), 0)
    np.testing.assert_allclose(got, np.where(r + inner > 0, r + inner, 0.1 * (r + inner)), rtol=1e-15, atol=0)
    # rank 2
    x2 = rng.standard_normal((4, 5))
    np.testing.assert_allclose(np_bn_infer(x2, g, b, mm, mv), np_bn_infer(x2.reshape(4, 1, 1, 5), g, b, mm, mv).reshape(4, 5))


# ---- run.py ----------------------------------------------------------------------------------------------------------------------
def _cfg(tmp_path, train_flag=True, eval_flag=False):
    cfg = yaml.safe_load(open(CFG))
    d = str(tmp_path / 'gancls')
    cfg.update(DATASET_DIR=d + '/data/', CHECKPOINT_DIR=d + '/ckpt/', LOGS_DIR=d + '/logs/', SAMPLE_DIR=d + '/samples/')
    cfg['TRAIN']['FLAG'] = train_flag
    cfg['EVAL']['FLAG'] = eval_flag
    path = str(tmp_path / ('gancls_%d%d.yml' % (train_flag, eval_flag)))
    yaml.safe_dump(cfg, open(path, 'w'))
    return path, d


def test_run_mode_errors_before_any_device_work(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.gancls import run
    no_train, d = _cfg(tmp_path, train_flag=False)
    with pytest.raises(NotImplementedError, match='visualize_gancls.py'):
        run.main(['--cfg', no_train])
    with pytest.raises(NotImplementedError, match='EVAL.FLAG'):
        run.main(['--cfg', _cfg(tmp_path, eval_flag=True)[0], '--train'])
    with pytest.raises(NotImplementedError, match='EVAL.FLAG'):
        run.main(['--cfg', _cfg(tmp_path, eval_flag=True)[0], '--visualize'])
    train, _ = _cfg(tmp_path)
    for mode in ('is', 'fid', 'imd'):
        with pytest.raises(ValueError, match='synthetic'):
            run.main(['--cfg', train, '--eval', mode, '--synthetic'])
    with pytest.raises(ValueError, match='synthetic'):
        run.main(['--cfg', train, '--visualize', '--synthetic'])
    with pytest.raises(ValueError, match='incep-batch'):
        run.main(['--cfg', train, '--incep-batch', '8'])
    with pytest.raises(ValueError, match='incep-batch'):
        run.main(['--cfg', train, '--eval', 'is', '--incep-batch', '0'])
    with pytest.raises(ValueError, match='steps'):
        run.main(['--cfg', train, '--train', '--steps', '0'])
    with pytest.raises(ValueError, match='interp'):
        run.main(['--cfg', train, '--train', '--interp', '2'])
    with pytest.raises(ValueError, match='interp'):
        run.main(['--cfg', train, '--visualize', '--interp', '-1'])
    for both in (['--train', '--eval', 'fid'], ['--train', '--visualize'], ['--visualize', '--eval', 'is']):
        with pytest.raises(SystemExit):
            run.main(['--cfg', train] + both)
    with pytest.raises(SystemExit):
        run.main(['--cfg', train, '--eval', 'kid'])
    assert not os.path.exists(d)          # nothing was created: the checks come first


def test_the_three_modules_exist_with_the_reference_class_names():
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.evaluator import GeneratorEval
    from t2i_amd.models.gancls.eval_gancls import GanClsEval
    from t2i_amd.models.gancls.visualize_gancls import SPECIAL_POSITIONS, GanClsVisualizer
    assert issubclass(GanClsEval, GeneratorEval) and all(hasattr(GanClsEval, f) for f in ('evaluate_inception', 'evaluate_fid', 'evaluate_imd'))
    assert tuple(SPECIAL_POSITIONS) == (1126, 908, 398) and hasattr(GanClsVisualizer, 'visualize')


# ---- the C symbol ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    return _lib


def test_bn_infer_is_an_added_symbol_of_abi_13(lib):
    assert lib.ABI_VERSION == 13 and lib.lib.t2i_version() == 13
    assert 't2i_bn_infer' in lib.SIGNATURES and hasattr(lib.lib, 't2i_bn_infer')
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    assert 'int t2i_bn_infer(' in header
    from t2i_amd import kernels as K
    assert callable(K.bn_infer)


def test_bn_infer_rejects_bad_arguments_before_launching(lib):
    """Every call below is invalid, so nothing is launched and no pointer is touched (the pointers are dummies)."""
    P, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)

    def call(x=P, gamma=P, beta=P, mm=P, mv=P, rows=8, C=16, res=None, y=P, dtype=lib.DT_F32):
        return lib.lib.t2i_bn_infer(x, gamma, beta, mm, mv, 1e-5, rows, C, ACT_RELU, 0.0, res, ACT_RELU, 0.0, y, dtype, None)
    for bad in (dict(x=None), dict(gamma=None), dict(beta=None), dict(mm=None), dict(mv=None), dict(y=None), dict(rows=0), dict(C=0)):
        assert call(**bad) == -1, bad
    assert b't2i_bn_infer: bad argument' in lib.lib.t2i_last_error()
    assert call(dtype=7) == -1
    # bf16 storage runs on the vectorised form only
    assert call(dtype=lib.DT_BF16, C=18) == -1
    assert call(dtype=lib.DT_BF16, x=odd) == -1
    assert call(dtype=lib.DT_BF16, res=odd) == -1
    assert b'bf16 tensors need 16-byte aligned pointers' in lib.lib.t2i_last_error()
