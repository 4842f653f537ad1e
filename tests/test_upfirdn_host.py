"""Host-side checks of the resampling operator, none of which needs a GPU: the float64 restatement of
tests/upfirdn_cases.py against the tensor library's composition, the adjoint identity, the extent function, the ties to nearest
upscaling and the 2x2 mean, the helpers' DC gain, every refusal in Python and (by ctypes, with fabricated pointers) in C before any
launch, PGGAN's argument, the scripts' flag and the readers' refusal of a checkpoint with other taps."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import upfirdn_cases as UC  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import _lib, kernels as K  # noqa: E402
from t2i_amd.utils import ops  # noqa: E402

FILTERS = ((1, 1), (1, 2, 1), (1, 3, 3, 1), (1, 4, 6, 4, 1))
TINY = dict(fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)


def _composition(x, taps, u, d, p0, p1, flip):
    """zero-stuff + F.pad + depthwise F.conv2d + stride, float64 (conv2d correlates: the kernel is the reversed g)"""
    g = np.asarray(taps, dtype=np.float32).astype(np.float64)
    if flip:
        g = g[::-1]
    x = x.double().permute(0, 3, 1, 2)
    B, C, H, W = x.shape
    z = x.new_zeros(B, C, H * u, W * u)
    z[:, :, ::u, ::u] = x
    z = F.pad(z, (p0, p1, p0, p1))
    w = torch.tensor(np.outer(g[::-1], g[::-1]).copy())[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(z, w, groups=C)[:, :, ::d, ::d].permute(0, 2, 3, 1).numpy()


def test_the_table_has_the_six_filters_and_the_kernels_tile():
    assert K.UPFIRDN_TILE == UC.TILE and K.UPFIRDN_MAX_TAPS == 8
    assert len(UC.CASES) == len(UC.PART) and len(UC.CASES) > 300
    assert [len(f) for f in UC.TAPS.values()] == [1, 2, 3, 4, 5, 8] and UC.TAPS['asym5'] != UC.TAPS['asym5'][::-1]


def test_restatement_against_the_tensor_library():
    worst = 0.0
    for i, (shape, name, u, d, p0, p1, flip) in enumerate(UC.CASES):
        x, y = UC.reference(i)[:2]
        want = _composition(x, UC.TAPS[name], u, d, p0, p1, flip)
        assert y.shape == want.shape, UC.case_id(UC.CASES[i])
        worst = max(worst, float(np.abs(y - want).max()))
        t = UC.ref_torch(x.double(), UC.TAPS[name], u, d, p0, p1, flip).numpy()
        worst = max(worst, float(np.abs(t - want).max()))
    print('restatement against zero-stuff + pad + conv2d + stride: largest difference %.2e' % worst)
    assert worst <= 1e-12


def test_adjoint_identity_and_extents():
    worst = 0.0
    for i, (shape, name, u, d, p0, p1, flip) in enumerate(UC.CASES):
        x, y, g, a, adj = UC.reference(i)
        n = len(UC.TAPS[name])
        assert a.shape == tuple(shape)                                      # the adjoint returns H and W exactly
        for H, Ho, q1 in ((shape[1], y.shape[1], adj[3][0]), (shape[2], y.shape[2], adj[3][1])):
            assert K.upfirdn2d_extent(H, u, d, p0, p1, n) == UC.extent(H, u, d, p0, p1, n) == Ho
            assert K.upfirdn2d_adjoint(H, Ho, n, u, d, p0, flip) == UC.adjoint_params(H, Ho, n, u, d, p0, flip) == (adj[0], adj[1], adj[2], q1, adj[4])
            assert K.upfirdn2d_extent(Ho, adj[0], adj[1], adj[2], q1, n) == H
        lhs, rhs = float((y * g.double().numpy()).sum()), float((x.double().numpy() * a).sum())
        worst = max(worst, abs(lhs - rhs))
    print('<A x, g> - <x, A^T g>: largest %.2e' % worst)
    assert worst <= 1e-9


def test_extent_function_refusals():
    assert K.upfirdn2d_extent(4, 2, 1, 2, 1, 4) == 8 and K.upfirdn2d_extent(8, 1, 2, 1, 1, 4) == 4
    for args in ((0, 1, 1, 0, 0, 1), (4, 3, 1, 0, 0, 1), (4, 1, 0, 0, 0, 1), (4, 1, 1, 0, 0, 0), (4, 1, 1, 0, 0, 9), (4, 1, 1, 32769, 0, 1),
                 (4, 1, 1, 0, -32769, 1), (4, 1, 1, -2, -2, 1), (4, 1, 1, 0, 0, 5), (2 ** 31, 1, 1, 0, 0, 1)):
        assert K.upfirdn2d_extent(*args) == 0, args
    assert K.upfirdn2d_extent(2 ** 31 - 1, 2, 1, 0, 0, 1) == 0                 # the extent itself would not fit


def test_box_taps_are_repeat_and_the_2x2_mean():
    x = UC.inputs((2, 6, 4, 3)).double().numpy()
    up = UC.ref_upfirdn2d(x, UC.helper_taps((1, 1), True), 2, 1, *UC.helper_pads(2, 2, 1))
    assert np.array_equal(up, x.repeat(2, 1).repeat(2, 2))
    down = UC.ref_upfirdn2d(x, UC.helper_taps((1, 1), False), 1, 2, *UC.helper_pads(2, 1, 2))
    assert np.abs(down - x.reshape(2, 3, 2, 2, 2, 3).mean((2, 4))).max() <= 1e-15


class _RestatedFn(object):
    """Stands in for autograd.UpFirDn2dFn: what utils.ops hands the kernel, computed by the restatement"""
    calls = []

    @classmethod
    def apply(cls, x, taps, u, d, p0, p1, flip):
        cls.calls.append((taps, u, d, p0, p1, flip))
        return torch.tensor(UC.ref_upfirdn2d(x, taps, u, d, p0, p1, flip))


@pytest.mark.parametrize('k', FILTERS, ids=lambda k: 'x'.join(map(str, k)))
def test_helpers_have_dc_gain_one_and_the_publications_pads(monkeypatch, k):
    monkeypatch.setattr(ops.A, 'UpFirDn2dFn', _RestatedFn)
    del _RestatedFn.calls[:]
    x = torch.ones(1, 8, 6, 2)
    up, down = ops.upsample_2d(x, k), ops.downsample_2d(x, k)
    assert tuple(up.shape) == (1, 16, 12, 2) and tuple(down.shape) == (1, 4, 3, 2)
    n, p = len(k), len(k) - 2
    (tu, uu, du, p0u, p1u, fu), (td, ud, dd, p0d, p1d, fd) = _RestatedFn.calls
    assert (uu, du, p0u, p1u, fu) == (2, 1, (p + 1) // 2 + 1, (p // 2, p // 2), False) and (ud, dd, p0d, p1d, fd) == (1, 2, (p + 1) // 2, (p // 2, p // 2), False)
    assert tu == UC.helper_taps(k, True) and td == UC.helper_taps(k, False)
    # constant input, away from the border: the constant itself (DC gain 1 in both polyphase branches)
    m = n // 2 + 1
    assert float((up[:, m:-m, m:-m] - 1.0).abs().max()) <= 1e-6 and float((down[:, 1:-1, 1:-1] - 1.0).abs().max()) <= 1e-6
    g = ops.upsample_2d(x, k, gain=4.0)
    assert float((g - 4.0 * up).abs().max()) <= 1e-5
    assert tuple(ops.upsample_2d(x, k, factor=1).shape) == tuple(x.shape) == tuple(ops.downsample_2d(x, k, factor=1).shape)


def test_python_refusals(monkeypatch):
    monkeypatch.setattr(ops.A, 'UpFirDn2dFn', _RestatedFn)
    x = torch.zeros(2, 4, 4, 3)
    bad = [dict(f=()), dict(f=(1,) * 9), dict(f=(1.0, float('nan'))), dict(f=(1.0, float('inf'))), dict(f=(1e30, 1.0), gain=1e30), dict(f='ab'),
           dict(f=(1, 1), up=3), dict(f=(1, 1), down=0), dict(f=(1, 1), up=True), dict(f=(1, 1), up=2.0),
           dict(f=(1, 1), pad=(32769, 0)), dict(f=(1, 1), pad=(0, -32769)), dict(f=(1, 1), pad=(0,)), dict(f=(1, 1), pad=(0.5, 0)),
           dict(f=(1, 1), pad=(-2, -2)), dict(f=(1,) * 8, pad=(1, 1)), dict(f=(1, 1), gain=-1.0), dict(f=(1, 1), gain=float('nan'))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.upfirdn2d(x, **kw)
    for t in (x.to(torch.bfloat16), x.double(), x[0], x.permute(0, 3, 1, 2), torch.zeros(0, 4, 4, 3), torch.zeros(2, 4, 4, 0)):
        with pytest.raises(ValueError):
            ops.upfirdn2d(t, (1, 1))
    from t2i_amd import stacked as ST
    with pytest.raises(NotImplementedError):
        ops.upfirdn2d(ST.Stacked.__new__(ST.Stacked), (1, 1))
    for fn in (ops.upsample_2d, ops.downsample_2d):
        for kw in (dict(factor=3), dict(factor=0), dict(factor=2.0), dict(k=(1, -1)), dict(k=()), dict(k=(1, float('inf')))):
            with pytest.raises(ValueError):
                fn(x, **kw)
        with pytest.raises(ValueError):
            fn(x.to(torch.bfloat16))
    with K.dry_run():                                                        # the kernel wrapper's own checks, without a launch
        assert tuple(K.upfirdn2d(x, (1, 3, 3, 1), 2, 1, 2, 1, False).shape) == (2, 8, 8, 3)
        assert tuple(K.upfirdn2d(x, (1, 3, 3, 1), 1, 2, 1, (1, 3), False).shape) == (2, 2, 3, 3)
        for args in ((x, (), 1, 1, 0, 0, False), (x, (1,) * 9, 1, 1, 0, 0, False), (x, (float('nan'),), 1, 1, 0, 0, False), (x, (1, 1), 3, 1, 0, 0, False),
                     (x, (1, 1), 1, 1, 40000, 0, False), (x, (1, 1), 1, 1, 0, -4, False), (x[0], (1, 1), 1, 1, 0, 0, False)):
            with pytest.raises(ValueError):
                K.upfirdn2d(*args)
        with pytest.raises(ValueError):
            K.upfirdn2d(x, (1, 1), 1, 1, 0, 0, False, out=torch.zeros(2, 3, 3, 4))
        with pytest.raises(ValueError):
            K.upfirdn2d(x, (1,), 1, 1, 0, 0, False, out=x)                  # overlapping
        with pytest.raises(TypeError):
            K.upfirdn2d(x.double(), (1, 1), 1, 1, 0, 0, False)


def test_c_refusals_come_before_any_launch():
    """Fabricated device pointers that nothing may dereference: every call must return T2I_ERR_INVALID (-1) from its checks."""
    lib = _lib.lib
    X, Y = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    good = (ctypes.c_float * 4)(1.0, 3.0, 3.0, 1.0)
    nan = (ctypes.c_float * 4)(1.0, float('nan'), 3.0, 1.0)
    inf = (ctypes.c_float * 4)(1.0, 3.0, float('inf'), 1.0)
    T = ctypes.cast(good, ctypes.c_void_p)

    def call(x=X, B=2, H=4, W=4, C=3, taps=T, n=4, u=2, d=1, p0=2, p1=1, flip=0, y=Y):
        return lib.t2i_upfirdn2d(x, B, H, W, C, taps, n, u, d, p0, p1, flip, y, None)

    cases = [dict(x=None), dict(y=None), dict(taps=None), dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(n=0), dict(n=9), dict(u=0), dict(u=3),
             dict(d=0), dict(d=4), dict(p0=32769), dict(p0=-32769), dict(p1=32769), dict(p1=-32769), dict(p0=-8, p1=-8), dict(u=1, p0=0, p1=0, H=3),
             dict(B=2 ** 16, H=2 ** 8, W=2 ** 7, C=1, u=1, p0=2, p1=1), dict(B=2 ** 15, H=2 ** 7, W=2 ** 7, C=1), dict(B=2 ** 30, H=2 ** 30, W=2 ** 30, C=2 ** 30),
             dict(y=ctypes.c_void_p(0x10000000 + 16)), dict(x=ctypes.c_void_p(0x20000000 + 64)),
             dict(taps=ctypes.cast(nan, ctypes.c_void_p)), dict(taps=ctypes.cast(inf, ctypes.c_void_p))]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b't2i_upfirdn2d' in _lib.lib.t2i_last_error(), kw
    assert lib.t2i_upfirdn2d_axes(X, 2, 4, 4, 3, T, 4, 1, 2, 1, 1, 32769, 0, Y, None) == -1
    assert lib.t2i_upfirdn2d_axes(X, 2, 4, 4, 3, T, 4, 1, 2, 1, -9, 1, 0, Y, None) == -1


def test_pggan_argument_validation():
    from t2i_amd.models.pggan.pggan import PGGAN, normalised_taps, same_taps
    mk = lambda **kw: PGGAN(4, 10, None, None, None, None, None, 2, True, build_model=False, device=torch.device('cpu'), **TINY, **kw)
    assert mk().resample_filter is None and mk(resample_filter=None).resample_taps is None
    m = mk(resample_filter=[1, 3, 3, 1])
    assert m.resample_filter == (1.0, 3.0, 3.0, 1.0) and m.resample_taps.dtype == np.float32
    assert np.array_equal(m.resample_taps, np.asarray([0.125, 0.375, 0.375, 0.125], np.float32))
    for bad in ((), (1,), (1,) * 9, (1, -1), (1, -2), (1, float('nan')), (float('inf'), 1), '1,3,3,1', 4, ('a', 'b')):
        with pytest.raises(ValueError):
            mk(resample_filter=bad)
    assert same_taps(None, None) and not same_taps(None, m.resample_taps) and not same_taps(m.resample_taps, None)
    assert same_taps(normalised_taps((2, 6, 6, 2))[1], m.resample_taps) and not same_taps(normalised_taps((1, 2, 1))[1], m.resample_taps)
    # the four sites, launch-free: with taps the model asks for the filtered resampling and builds the same variables
    with K.dry_run(), torch.no_grad():
        names = []
        for kw in ({}, {'resample_filter': (1, 3, 3, 1)}):
            mm = PGGAN(4, 10, None, None, None, None, None, 3, True, device=torch.device('cpu'), **TINY, **kw)
            names.append([(n, tuple(v.shape)) for n, v in mm.store.vars.items()])
        assert names[0] == names[1]


def test_the_model_sites_call_the_filtered_resampling(monkeypatch):
    from t2i_amd.models.pggan import pggan as PM
    seen = []
    monkeypatch.setattr(PM, 'upsample_2d', lambda x, k: (seen.append(('up', tuple(x.shape), k)), ops.upscale(x, 2))[1])
    monkeypatch.setattr(PM, 'downsample_2d', lambda x, k: (seen.append(('down', tuple(x.shape), k)), ops.pool(x, 2))[1])
    with K.dry_run(), torch.no_grad():
        PM.PGGAN(4, 10, None, None, None, None, None, 3, True, device=torch.device('cpu'), **TINY)
        assert seen == []
        PM.PGGAN(4, 10, None, None, None, None, None, 3, True, device=torch.device('cpu'), resample_filter=(1, 3, 3, 1), **TINY)
    k = (1.0, 3.0, 3.0, 1.0)
    # generator: the fade-in's RGB and both blocks; critic: the fade-in's RGB and both blocks
    assert seen == [('up', (4, 4, 4, 16), k), ('up', (4, 8, 8, 3), k), ('up', (4, 8, 8, 16), k),
                    ('down', (4, 16, 16, 3), k), ('down', (4, 16, 16, 16), k), ('down', (4, 8, 8, 16), k)], seen


def _parse_error(main, argv):
    with pytest.raises(SystemExit) as e:
        main(argv)
    return e.value.code


def test_the_scripts_parse_the_flag(capsys):
    import argparse
    from t2i_amd.models.pggan import options as cli
    from t2i_amd.models.pggan import eval_pggan, train_pggan, visualize_last_stage, visualize_pggan
    for reader in (True, False):
        ap = argparse.ArgumentParser()
        cli.add_resample_filter_argument(ap, reader=reader)
        assert cli.resample_filter_of(ap, ap.parse_args([])) is None
        assert cli.resample_filter_of(ap, ap.parse_args(['--resample-filter', '1,3,3,1'])) == (1.0, 3.0, 3.0, 1.0)
        assert cli.resample_filter_of(ap, ap.parse_args(['--resample-filter', '0.25, 0.5,0.25'])) == (0.25, 0.5, 0.25)
        for bad in ('1', '1,-1', '1,x', 'nan,1', '1,inf', ','.join('1' * 9), ''):
            with pytest.raises(SystemExit):
                cli.resample_filter_of(ap, ap.parse_args(['--resample-filter', bad]))
    for mod in (eval_pggan, visualize_pggan, visualize_last_stage):
        assert _parse_error(mod.main, ['--cfg', 'none.yml', '--resample-filter', '1,-1']) == 2
        with pytest.raises(Exception) as e:                                 # a well-formed flag gets past the parser, to the missing config
            mod.main(['--cfg', os.path.join(ROOT, 'no', 'such.yml'), '--resample-filter', '1,3,3,1'])
        assert not isinstance(e.value, SystemExit)
    assert _parse_error(train_pggan.main, ['--resample-filter', '1,x']) == 2
    with pytest.raises(FileNotFoundError):
        train_pggan.main(['--cfg', os.path.join(ROOT, 'no', 'such.yml'), '--resample-filter', '1,3,3,1'])
    capsys.readouterr()


def test_restore_generator_refuses_other_taps(tmp_path):
    from t2i_amd.models.pggan import eval_pggan as E
    from t2i_amd.models.pggan.pggan import RESAMPLE_KEY
    from t2i_amd.utils.config import AttrDict
    from t2i_amd.utils.saver import Saver, restore_scopes, save
    dev = torch.device('cpu')
    taps = np.asarray([0.125, 0.375, 0.375, 0.125], np.float32)
    cfgs = {}
    for tag, extra in (('with', {RESAMPLE_KEY: ((lambda: taps), None)}), ('without', None)):
        cfgs[tag] = AttrDict({'CHECKPOINT_DIR': str(tmp_path / tag)})
        m = E.stage_model(cfgs[tag], 2, 4, None, dev, **TINY)
        with torch.no_grad():
            for v in m.store.vars.values():
                v.fill_(0.5)
        path = save(Saver(m.store, var_list=['g_net'], extra=extra), None, os.path.join(cfgs[tag].CHECKPOINT_DIR, 'stage2/'), 1)
        assert (RESAMPLE_KEY in np.load(path).files) == (extra is not None)
    ok = E.stage_model(cfgs['with'], 2, 4, None, dev, resample_filter=(2, 6, 6, 2), **TINY)     # the same normalised taps
    E.restore_generator(ok)
    assert all(float(v.detach().min()) == 0.5 for v in ok.store.vars.values())
    E.restore_generator(E.stage_model(cfgs['without'], 2, 4, None, dev, **TINY))
    for tag, kw, sides in (('with', {}, ('0.125, 0.375, 0.375, 0.125', 'no filter')),
                           ('with', {'resample_filter': (1, 2, 1)}, ('0.125, 0.375, 0.375, 0.125', '0.25, 0.5, 0.25')),
                           ('without', {'resample_filter': (1, 3, 3, 1)}, ('no filter', '0.125, 0.375, 0.375, 0.125'))):
        with pytest.raises(RuntimeError) as err:
            E.restore_generator(E.stage_model(cfgs[tag], 2, 4, None, dev, **dict(TINY, **kw)))
        assert all(s in str(err.value) for s in sides) and str(tmp_path) in str(err.value), str(err.value)
    # restore_scopes: the default reads no entry; with extra= the setter gets the file's entry
    got = []
    store = E.stage_model(cfgs['with'], 2, 4, None, dev, **TINY).store
    restore_scopes(store, [('g_net', os.path.join(cfgs['with'].CHECKPOINT_DIR, 'stage2/'))], verbose=False)
    restore_scopes(store, [('g_net', os.path.join(cfgs['with'].CHECKPOINT_DIR, 'stage2/'))], verbose=False, extra={RESAMPLE_KEY: (None, got.append)})
    assert len(got) == 1 and np.array_equal(got[0], taps)
