"""Host-side checks of the style layer and the style-based PGGAN generator, no GPU: the float64 restatement's
backward against torch autograd, every refusal of ops.adain and of the C entries (all before any launch), the PGGAN constructor's
validation, the default model's variable list, the mapping network's Adam multipliers, the flags and the readers' refusal message."""
import argparse
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import style_cases as SC  # noqa: E402


@pytest.fixture(scope='module')
def t2i():
    lib = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd
    return t2i_amd


@pytest.mark.parametrize('act', SC.ACTS, ids=lambda a: a or 'none')
@pytest.mark.parametrize('noise', [False, True], ids=['plain', 'noise'])
def test_the_float64_restatement_agrees_with_torch_autograd(act, noise):
    inp = SC.inputs((2, 5, 7, 3), noise, act)
    r = SC.evaluate(inp, act, np.float64)
    T = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    x, ys, yb = T(inp['x']), T(inp['ys']), T(inp['yb'])
    st = T(inp['strength']) if noise else None
    p = x + st * torch.tensor(inp['noise'], dtype=torch.float64)[..., None] if noise else x
    u = p if act is None else torch.where(p > 0, p, (0.0 if act == 'relu' else SC.ALPHA) * p)
    mu = u.mean((1, 2), keepdim=True)
    var = ((u - mu) ** 2).mean((1, 2), keepdim=True)
    y = (u - mu) / torch.sqrt(var + SC.EPS) * (1 + ys[:, None, None, :]) + yb[:, None, None, :]
    y.backward(torch.tensor(inp['g'], dtype=torch.float64))
    assert np.abs(y.detach().numpy() - r['y']).max() <= 1e-9
    for t, k in ((x, 'dx'), (ys, 'dys'), (yb, 'dyb')) + (((st, 'dstrength'),) if noise else ()):
        assert np.abs(t.grad.numpy() - r[k]).max() <= 1e-9 * max(1.0, np.abs(r[k]).max()), k
    assert noise or r['dstrength'] is None


def test_the_inputs_stay_clear_of_the_kink():
    for act in ('relu', 'lrelu'):
        inp = SC.inputs((3, 33, 31, 20), True, act)
        p = inp['x'].astype(np.float64) + inp['strength'].astype(np.float64) * inp['noise'].astype(np.float64)[..., None]
        assert np.abs(p).min() >= SC.KINK * 0.99


def test_abi_declares_binds_and_exports_the_entries(t2i):
    from t2i_amd import _lib, kernels
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    for name, nargs in (('t2i_adain_chunk_rows', 0), ('t2i_adain_workspace_bytes', 3), ('t2i_adain_stats', 14), ('t2i_adain_apply', 15),
                        ('t2i_adain_bwd_sums', 16), ('t2i_adain_bwd_apply', 20)):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and len(_lib.SIGNATURES[name][1]) == nargs and name + '(' in header, name
    assert kernels.ADAIN_CHUNK_ROWS == SC.CHUNK == 64 and '#define T2I_ADAIN_CHUNK_ROWS 64' in header
    assert 't2i_style' in open(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 'build.sh')).read()
    L = _lib.lib
    assert L.t2i_adain_workspace_bytes(8, 65536, 64) >= 8 * 1024 * 2 * 64 * 4 and L.t2i_adain_workspace_bytes(0, 4, 4) == 0
    assert L.t2i_adain_workspace_bytes(3, 1 << 31, 1) == 0 and L.t2i_adain_workspace_bytes(1 << 20, 1 << 10, 4) == 0


def test_every_entry_refuses_bad_arguments_before_any_launch(t2i):
    """No GPU is touched: every refusal returns before the first launch, so the fake pointers are never read."""
    from t2i_amd import _lib
    L = _lib.lib
    P = ctypes.c_void_p
    a = [P(0x1000 * (i + 1)) for i in range(12)]          # distinct, 16-byte aligned, never dereferenced
    ws, wsn = P(0x100000), 1 << 20
    INVALID, WORKSPACE = -1, -2

    def stats(x=a[0], nz=a[1], s=a[2], B=2, R=16, C=8, act=2, alpha=0.0, eps=1e-8, mean=a[3], rstd=a[4], w=ws, wn=wsn):
        return L.t2i_adain_stats(x, nz, s, B, R, C, act, alpha, eps, mean, rstd, w, wn, None)

    def apply(x=a[0], nz=a[1], s=a[2], mean=a[3], rstd=a[4], ys=a[5], yb=a[6], stride=8, B=2, R=16, C=8, act=2, alpha=0.0, y=a[7]):
        return L.t2i_adain_apply(x, nz, s, mean, rstd, ys, yb, stride, B, R, C, act, alpha, y, None)

    def sums(g=a[8], x=a[0], nz=a[1], s=a[2], mean=a[3], rstd=a[4], B=2, R=16, C=8, act=2, alpha=0.0, dys=a[9], dyb=a[10], w=ws, wn=wsn):
        return L.t2i_adain_bwd_sums(g, x, nz, s, mean, rstd, B, R, C, act, alpha, dys, dyb, w, wn, None)

    def bapply(g=a[8], x=a[0], nz=a[1], s=a[2], mean=a[3], rstd=a[4], ys=a[5], stride=8, dys=a[9], dyb=a[10], B=2, R=16, C=8, act=2, alpha=0.0,
               dx=a[7], ds=a[11], w=ws, wn=wsn):
        return L.t2i_adain_bwd_apply(g, x, nz, s, mean, rstd, ys, stride, dys, dyb, B, R, C, act, alpha, dx, ds, w, wn, None)

    for f in (stats, apply, sums, bapply):
        for kw in (dict(x=None), dict(B=0), dict(R=0), dict(C=0), dict(R=1 << 31), dict(B=1 << 16, R=1 << 10, C=64), dict(act=3), dict(act=7),
                   dict(act=1, alpha=-0.1), dict(act=1, alpha=float('nan')), dict(nz=None), dict(s=None), dict(mean=None), dict(rstd=None)):
            assert f(**kw) == INVALID, (f.__name__, kw)
            assert L.t2i_last_error()
    assert stats(eps=-1.0) == INVALID and stats(eps=float('nan')) == INVALID and stats(eps=float('inf')) == INVALID
    for f in (stats, sums, bapply):
        for kw in (dict(w=None), dict(w=P(0x100004)), dict(wn=16)):
            assert f(**kw) == WORKSPACE, (f.__name__, kw)
    assert apply(stride=7) == INVALID and bapply(stride=7) == INVALID
    assert apply(ys=None) == INVALID and apply(yb=None) == INVALID and apply(y=None) == INVALID and apply(y=a[0]) == INVALID       # y overlaps x
    assert sums(g=None) == INVALID and sums(dys=None) == INVALID and sums(dyb=None) == INVALID
    assert bapply(dx=None) == INVALID and bapply(dx=a[8]) == INVALID and bapply(dx=a[0]) == INVALID and bapply(ys=None) == INVALID
    assert bapply(nz=None, s=None) == INVALID                                   # dstrength without noise


def test_adain_refusals(t2i):
    from t2i_amd import kernels as K, stacked as ST
    from t2i_amd.utils import ops
    x = torch.zeros(2, 4, 4, 8)
    ys, yb, nz, st = torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2, 4, 4), torch.zeros(8)
    with K.dry_run():
        assert ops.adain(x, ys, yb, nz, st, act=ops.relu).shape == x.shape          # the accepted call
        both = torch.zeros(2, 16)
        assert ops.adain(x, both[:, :8], both[:, 8:]).shape == x.shape              # the halves of one dense output, as views
        bad = [
            (dict(x=x.bfloat16()), 'float32'), (dict(x=x[0]), 'rank-4'), (dict(x=x.permute(0, 3, 1, 2)), 'non-contiguous'),
            (dict(ys=torch.zeros(2, 7)), 'ys'), (dict(yb=torch.zeros(3, 8)), 'yb'), (dict(ys=ys.double()), 'ys'),
            (dict(noise=torch.zeros(2, 4, 5)), 'noise'), (dict(strength=torch.zeros(7)), 'strength'), (dict(noise=None), 'strength without noise'),
            (dict(strength=None), 'noise without strength'), (dict(noise=nz.clone().requires_grad_(True)), 'requires a gradient'),
            (dict(noise=torch.zeros(2, 4, 8)[:, :, ::2]), 'contiguous'),
            (dict(act=ops.lrelu_act(-0.1)), 'negative slope'), (dict(act=ops.tanh), 'act must be'), (dict(act=torch.relu), 'act must be'),
            (dict(eps=-1.0), 'eps'), (dict(eps=float('nan')), 'eps'),
        ]
        for kw, word in bad:
            args = dict(x=x, ys=ys, yb=yb, noise=nz, strength=st, act=ops.relu, eps=1e-8)
            args.update(kw)
            with pytest.raises(ValueError, match=word):
                ops.adain(args.pop('x'), args.pop('ys'), args.pop('yb'), **args)
        with pytest.raises(NotImplementedError, match='stacked'):
            ops.adain(ST.Stacked(x, x), ys, yb)
        with pytest.raises(ValueError, match='w must be'):
            ops.style_block(x, torch.zeros(3, 16))
    with pytest.raises(RuntimeError, match='no CPU path'):                              # outside a dry run a CPU tensor is no fallback
        ops.adain(x, ys, yb)


def _pggan(**kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    args = dict(fmap_base=64, fmap_max=32, z_dim=16, embed_dim=32, compr_embed_dim=8, device='cpu')
    args.update(kw)
    stage, trans = args.pop('stage', 2), args.pop('trans', True)
    return PGGAN(4, 100, None, None, None, None, None, stage, trans, **args)


def test_pggan_constructor_validation(t2i):
    for kw, word in ((dict(style_dim=0), 'style_dim'), (dict(style_dim=True), 'style_dim'), (dict(style_dim=16.0), 'style_dim'),
                     (dict(style_dim='16'), 'style_dim'), (dict(style_dim=16, mapping_layers=0), 'mapping_layers'),
                     (dict(style_dim=16, mapping_layers=2.0), 'mapping_layers'), (dict(style_dim=16, style_noise=1), 'style_noise'),
                     (dict(style_dim=16, truncation_psi='0.7'), 'truncation_psi'), (dict(style_dim=16, truncation_psi=float('nan')), 'truncation_psi'),
                     (dict(style_dim=16, truncation_psi=True), 'truncation_psi'), (dict(truncation_psi=0.7), 'needs style_dim')):
        with pytest.raises(ValueError, match=word):
            _pggan(build_model=False, **kw)
    m = _pggan(build_model=False, style_dim=16, mapping_layers=2, style_noise=False, truncation_psi=0.5)
    assert (m.style_dim, m.mapping_layers, m.style_noise, m.truncation_psi) == (16, 2, False, 0.5)
    with pytest.raises(ValueError, match='style-based generator'):
        _pggan().sampler(torch.zeros(4, 16), torch.zeros(4, 32), truncation_psi=0.5)


@pytest.mark.parametrize('stage,trans', [(1, False), (2, True), (3, False)])
def test_the_default_model_is_todays(t2i, stage, trans):
    """style_dim=None: the variables, in order, are the reference's (oracle/torch_pggan.py), and no checkpoint name is added."""
    from oracle import torch_pggan as PG
    m = _pggan(stage=stage, trans=trans)
    ref = PG.init_variables(PG.Cfg(z_dim=16, embed_dim=32, compressed=8, batch=4, base=64, cap=32), stage, trans)
    assert [(n, tuple(v.shape)) for n, v in m.store.vars.items()] == [(n, tuple(v.shape)) for n, v in ref.items()]
    assert m.style_dim is None and m.style_noise_keys() == [] and not any('mapping' in n for n in m.get_variables_up_to_stage(stage))
    assert m.kernel_scales(m.g_vars) is None


def test_the_style_model_and_its_restatement_name_the_same_variables(t2i):
    from oracle import torch_pggan as PG
    from t2i_amd.models.pggan.pggan import W_AVG, style_of_names
    m = _pggan(style_dim=16, equalized_lr=True)
    cfg = PG.Cfg(z_dim=16, embed_dim=32, compressed=8, batch=4, base=64, cap=32)
    V = PG.Vars(None, 0, torch.float64)
    z, c = torch.zeros(4, 16, dtype=torch.float64), torch.zeros(4, 32, dtype=torch.float64)
    nz = [torch.zeros(4, s, s, dtype=torch.float64) for s in SC.style_block_sizes(2)]
    with torch.no_grad():
        SC.style_generator(V, cfg, z, c, 2, True, 0.3, None, 16, 4, nz)
    mine = {n: tuple(v.shape) for n, v in m.store.vars.items() if n.startswith('g_net') and n != W_AVG}
    assert mine == {n: tuple(v.shape) for n, v in V.P.items()}
    assert not m.store.trainable[W_AVG] and W_AVG not in m.g_vars and tuple(m.store.vars[W_AVG].shape) == (16,)
    assert not any('LayerNorm_1' in n for n in mine) and 'g_net/conv_stage_0/LayerNorm/gamma' in mine          # the trunk's norm stays
    assert [k for k, _ in m.style_noise_keys()] == ['style_noise_%s_%d' % (t, k) for t in 'dg' for k in range(4)]
    assert [s for _, s in m.style_noise_keys()] == [4, 4, 8, 8] * 2
    keep = m.get_variables_up_to_stage(2)
    assert W_AVG in keep and 'g_net/mapping/dense_3/kernel' in keep and 'g_net/conv_stage_1/StyleMod_1/noise_strength' in keep
    assert set(m.get_variables_up_to_stage(1)) >= {W_AVG, 'g_net/mapping/dense/kernel'}
    # equalized learning rate: (c, c) for every kernel, (c, 0.01) for the mapping network's
    scales = m.kernel_scales(m.g_vars)
    for n, v in m.g_vars.items():
        if n.startswith('g_net/mapping/') and n.endswith('/kernel'):
            assert scales[n] == (math.sqrt(2.0 / v.shape[0]), 0.01), n
        elif n.endswith('/style/kernel'):
            assert scales[n] == math.sqrt(2.0 / 16), n
        elif n.endswith('noise_strength') or n.endswith('bias'):
            assert n not in scales
    assert sum(1 for n in scales if n.startswith('g_net/mapping/')) == 4
    assert m.G_optimizer.slot_scales['g_net/mapping/dense_1/kernel'] == (math.sqrt(2.0 / 16), 0.01)
    assert style_of_names({n: tuple(v.shape) for n, v in m.store.vars.items()}) == (16, 4, True)
    quiet = _pggan(style_dim=8, mapping_layers=2, style_noise=False)
    assert not any(n.endswith('noise_strength') for n in quiet.store.vars) and quiet.style_noise_keys() == []
    assert style_of_names({n: tuple(v.shape) for n, v in quiet.store.vars.items()}) == (8, 2, False)


def test_flags_and_the_refusal_message(t2i, tmp_path):
    from t2i_amd.models.pggan import options as cli
    from t2i_amd.models.pggan import eval_pggan as E
    from t2i_amd.utils.saver import Saver, save

    def parse(argv, reader=True):
        ap = argparse.ArgumentParser()
        cli.add_style_arguments(ap, reader=reader)
        return cli.style_kwargs_of(ap, ap.parse_args(argv))
    assert parse([]) == {}
    assert parse(['--style-dim', '16']) == {'style_dim': 16}
    assert parse(['--style-dim', '16', '--mapping-layers', '2', '--no-style-noise', '--truncation-psi', '0.7']) == {
        'style_dim': 16, 'mapping_layers': 2, 'style_noise': False, 'truncation_psi': 0.7}
    for argv in (['--mapping-layers', '2'], ['--no-style-noise'], ['--truncation-psi', '0.5'], ['--style-dim', '0'],
                 ['--style-dim', '4', '--mapping-layers', '0'], ['--style-dim', '4', '--truncation-psi', 'nan']):
        with pytest.raises(SystemExit):
            parse(argv)
    with pytest.raises(SystemExit):
        parse(['--style-dim', '4', '--truncation-psi', '0.5'], reader=False)          # the trainer has no truncation
    # a checkpoint of the style-based generator, read by a model built without the flag (and the reverse): refused by name
    styled = _pggan(style_dim=16, stage=1, trans=False)
    d = str(tmp_path / 'stage1') + '/'
    save(Saver(styled.store, var_list=styled.get_variables_up_to_stage(1)), None, d, 7)
    assert E.checkpoint_names(d)['g_net/mapping/w_avg'] == (16,) and E.checkpoint_names(str(tmp_path / 'none')) is None
    plain = _pggan(stage=1, trans=False, build_model=False)
    plain.check_dir_read = d
    with pytest.raises(RuntimeError, match=r'--style-dim 16 --mapping-layers 4.*no --style-dim.*pass the same --style-dim'):
        E.restore_generator(plain)
    other = _pggan(style_dim=16, mapping_layers=2, stage=1, trans=False, build_model=False)
    other.check_dir_read = d
    with pytest.raises(RuntimeError, match=r'--mapping-layers 4.*--mapping-layers 2'):
        E.restore_generator(other)
    d0 = str(tmp_path / 'plain1') + '/'
    ref = _pggan(stage=1, trans=False)
    save(Saver(ref.store, var_list=ref.get_variables_up_to_stage(1)), None, d0, 7)
    styled.check_dir_read = d0
    with pytest.raises(RuntimeError, match=r"the reference's generator.*--style-dim 16"):
        E.restore_generator(styled)
