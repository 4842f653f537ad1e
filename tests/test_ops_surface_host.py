"""The completed operator surface (reference utils/ops.py) without a GPU: every public name with the reference's defaults, the new
exports in header and binding, batch_renorm's variables, the refusals (all before any device work) and output shapes of a dry pass."""
import contextlib
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the public names of the reference's utils/ops.py with their parameters and defaults, written out (inspect._empty = no default)
_E = inspect.Parameter.empty
REFERENCE_SURFACE = {
    'batch_norm': [('x', _E), ('train', _E), ('init', None), ('act', None), ('name', None), ('eps', 1e-5), ('decay', 0.9), ('df', 'NHWC')],
    'batch_renorm': [('x', _E), ('train', _E), ('init', None), ('act', None), ('name', None), ('eps', 1e-5), ('decay', 0.9), ('df', 'NHWC')],
    'conv2d': [('x', _E), ('f', _E), ('ks', (4, 4)), ('s', (2, 2)), ('padding', 'SAME'), ('act', None), ('init', None), ('name', None),
               ('df', 'NHWC')],
    'conv2d_transpose': [('x', _E), ('f', _E), ('ks', (4, 4)), ('s', (2, 2)), ('padding', 'SAME'), ('act', None), ('init', None),
                         ('name', None), ('df', 'NHWC')],
    'layer_norm': [('x', _E), ('act', None), ('scope', None), ('df', 'NHWC')],
    'fc': [('x', _E), ('units', _E), ('act', None), ('init', None), ('bias', True), ('name', None)],
    'lrelu_act': [('alpha', 0.2)],
    'pixel_norm': [('x', _E), ('eps', 1e-8), ('act', None)],
    'pool': [('x', _E), ('s', 2), ('p_type', 'AVG'), ('df', 'NHWC')],
    'resize_nearest_neighbor': [('x', _E), ('new_size', _E)],
    'upscale': [('x', _E), ('s', 2)],
    'downscale': [('x', _E), ('s', 2)],
    'get_conv_shape': [('tensor', _E)],
    'get_ints_from_shape': [('tensor', _E)],
    'to_nchw': [('x', _E)],
    'to_nhwc': [('x', _E)],
    'df_to_channel': [('df', _E)],
    'gn': [('x', _E), ('mag', _E)],
}
NEW_EXPORTS = ('t2i_pixel_norm_fwd', 't2i_pixel_norm_bwd', 't2i_resize_nearest', 't2i_resize_nearest_adj', 't2i_pool_same_fwd',
               't2i_pool_same_bwd', 't2i_pool_same_take', 't2i_gn_fwd', 't2i_mul')


@contextlib.contextmanager
def _store(st):
    from t2i_amd import scope as S
    prev = S._DEFAULT[0]
    S.set_default_store(st)
    try:
        yield st
    finally:
        S.set_default_store(prev)


@pytest.fixture(scope='module')
def ops():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    return ops


def test_every_reference_name_with_its_defaults(ops):
    assert ops.NHWC == 'NHWC' and ops.NCHW == 'NCHW'
    for name, params in REFERENCE_SURFACE.items():
        fn = getattr(ops, name)
        got = [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
        # this project's wrappers may take further keyword parameters AFTER the reference's (conv2d stats=, batch_norm groups=, ...)
        assert got[:len(params)] == params, (name, got)
        assert all(d is not _E for _, d in got[len(params):]), (name, got)


def test_new_exports_in_header_and_binding():
    from t2i_amd import _lib
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    declared = set(re.findall(r'\b(t2i_[a-z0-9_]+)\s*\(', header))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.lib.t2i_version() == 13 and _lib.ABI_VERSION == 13
    assert 'currently 13' in header


def test_batch_renorm_variables_on_a_cpu_store(ops):
    """Names, shapes, initial values and trainability.  renorm_stddev starts at ZERO, as in TF 1.4 (and as the first training step's
    r = 1, d = 0 requires): renorm_stddev / renorm_stddev_weight is a zero-debiased running sigma."""
    from t2i_amd import kernels as K
    from t2i_amd import scope as S
    st = S.VariableStore(device='cpu')
    expect = {'beta': ((6,), 0.0, True), 'gamma': ((6,), 1.0, True), 'moving_mean': ((6,), 0.0, False),
              'moving_variance': ((6,), 1.0, False), 'renorm_mean': ((6,), 0.0, False), 'renorm_stddev': ((6,), 0.0, False),
              'renorm_mean_weight': ((), 0.0, False), 'renorm_stddev_weight': ((), 0.0, False)}
    with _store(st), K.dry_run():
        with st.variable_scope('g_net'):
            y = ops.batch_renorm(torch.zeros(2, 3, 3, 6), True, act=ops.relu)
            y2 = ops.batch_renorm(torch.zeros(4, 6), True)
        assert tuple(y.shape) == (2, 3, 3, 6) and tuple(y2.shape) == (4, 6)
        assert sorted(st.vars) == sorted(['g_net/BatchNorm/' + n for n in expect] + ['g_net/BatchNorm_1/' + n for n in expect])
        for n, (shape, value, trainable) in expect.items():
            v = st.vars['g_net/BatchNorm/' + n]
            assert tuple(v.shape) == shape and v.dtype == torch.float32, n
            assert bool((v == value).all()), n
            assert st.trainable['g_net/BatchNorm/' + n] is trainable and v.requires_grad is trainable, n
        before = {n: v for n, v in st.vars.items()}
        with st.variable_scope('g_net', reuse=True):
            ops.batch_renorm(torch.zeros(2, 3, 3, 6), False, name='BatchNorm')
        assert list(st.vars) == list(before) and all(st.vars[n] is before[n] for n in before)


def _stacked(t):
    from t2i_amd import stacked as ST
    return ST.Stacked(t, t.clone())


def test_refusals_before_any_device_work(ops):
    """No dry_run here: a CPU tensor that reached a kernel wrapper would raise RuntimeError('... no CPU path'), so the expected
    exception types show that each refusal happens first."""
    from t2i_amd import scope as S
    x = torch.zeros(2, 4, 4, 8)
    h = x.to(torch.bfloat16)
    st = S.VariableStore(device='cpu')
    calls = {'pixel_norm': lambda t: ops.pixel_norm(t), 'resize_nearest_neighbor': lambda t: ops.resize_nearest_neighbor(t, (3, 3)),
             'upscale': lambda t: ops.upscale(t, 3), 'downscale': lambda t: ops.downscale(t, 2), 'pool': lambda t: ops.pool(t, 3, 'MAX'),
             'gn': lambda t: ops.gn(t, 1.0), 'batch_renorm': lambda t: ops.batch_renorm(t, True)}
    with _store(st):
        for name, call in calls.items():
            with pytest.raises(ValueError, match=name):
                call(h)
            with pytest.raises(NotImplementedError, match=name):
                call(_stacked(x))
    assert not st.vars                                                    # refused before a variable was made
    for name in ('pixel_norm', 'resize_nearest_neighbor', 'upscale', 'downscale', 'pool'):
        with pytest.raises(ValueError):
            calls[name](torch.zeros(4, 8))                                # rank != 4
        with pytest.raises(ValueError):
            calls[name](torch.zeros(2, 4, 4, 8, 1))
    with pytest.raises(ValueError, match='to_nhwc'):
        ops.pixel_norm(ops.to_nchw(x))                                    # a logical NCHW view is not contiguous
    with pytest.raises(ValueError, match='to_nhwc'):
        ops.pixel_norm(x[:, :, :, ::2])
    with pytest.raises(ValueError, match='negative slope'):                # the backward reads lrelu's derivative from the sign of y
        ops.pixel_norm(x, act=ops.lrelu_act(-0.5))
    with pytest.raises(ValueError, match='empty'):
        ops.downscale(torch.zeros(1, 3, 8, 4), 4)
    with pytest.raises(ValueError, match='empty'):
        ops.downscale(x, 5)
    with pytest.raises(ValueError, match='p_type'):
        ops.pool(x, 2, 'SUM')
    with pytest.raises(ValueError, match='p_type'):
        ops.pool(x, 3, 'avg')
    with pytest.raises(RuntimeError, match='no CPU path'):                # and an accepted call on a CPU tensor has no fallback
        ops.pixel_norm(x)


def test_output_shapes_of_a_dry_pass(ops):
    from t2i_amd import kernels as K
    with K.dry_run():
        for (H, W) in ((5, 7), (6, 6), (4, 9), (8, 8)):
            x = torch.zeros(2, H, W, 3)
            assert tuple(ops.resize_nearest_neighbor(x, (3, 4)).shape) == (2, 3, 4, 3)
            assert tuple(ops.resize_nearest_neighbor(x, (2 * H + 1, W)).shape) == (2, 2 * H + 1, W, 3)
            for s in (1, 2, 3, 4):
                for p_type in ('AVG', 'MAX'):
                    assert tuple(ops.pool(x, s, p_type).shape) == (2, -(-H // s), -(-W // s), 3)
                    assert tuple(ops.pool(ops.to_nchw(x), s, p_type, df=ops.NCHW).shape) == (2, 3, -(-H // s), -(-W // s))
                assert tuple(ops.upscale(x, s).shape) == (2, H * s, W * s, 3)
                assert tuple(ops.downscale(x, s).shape) == (2, H // s, W // s, 3)
        assert tuple(ops.pool(torch.zeros(1, 3, 5, 2), 9, 'MAX').shape) == (1, 1, 1, 2)
        assert tuple(ops.pixel_norm(torch.zeros(2, 3, 5, 3), act=ops.lrelu_act(0.2)).shape) == (2, 3, 5, 3)
        assert tuple(ops.gn(torch.zeros(2, 3, 5, 3), 1.5).shape) == (2, 3, 5, 3)
