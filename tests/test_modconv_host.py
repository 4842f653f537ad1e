"""Host-side checks of the weight-demodulated convolution and PGGAN(modulated_conv=True), no GPU: the float64
restatements against torch autograd, the factorised form against the definition, every refusal of ops.modulated_conv2d and of the C
entries (all before any launch), the option's validation and flags, the model's variable list against the restatement's, the equalized
learning-rate scales, the unchanged default and AdaIN variable lists, and the readers' refusal of a checkpoint of the other kind."""
import argparse
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import modconv_cases as MC  # noqa: E402
import style_cases as SC  # noqa: E402


@pytest.fixture(scope='module')
def t2i():
    lib = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd
    return t2i_amd


T64 = lambda a, grad=True: torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


# ---- the restatements against autograd, float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(1, 3, 4, 3), (9, 20, 12, 2)], ids=str)
def test_the_coefficient_restatement_agrees_with_autograd(case):
    W, s, gd = MC.coef_inputs(case)
    r = MC.coef(W, s, gd, np.float64)
    Wt, st = T64(W), T64(s)
    d = torch.rsqrt(((Wt[None] * st[:, None, :, None]) ** 2).sum((1, 2)) + MC.EPS)            # the definition: the modulated filter's norm
    d.backward(T64(gd, False))
    assert np.abs(d.detach().numpy() - r['d']).max() <= 1e-12 * np.abs(r['d']).max()
    for t, k in ((Wt, 'dW'), (st, 'ds')):
        assert np.abs(t.grad.numpy() - r[k]).max() <= 1e-12 * max(1.0, np.abs(r[k]).max()), k


def test_the_scale_restatement_agrees_with_autograd():
    x, s, g = MC.scale_inputs((3, 5, 7, 4))
    r = MC.scale(x, s, g, np.float64)
    xt, st = T64(x), T64(s)
    y = xt * st[:, None, None, :]
    y.backward(T64(g, False))
    assert np.array_equal(y.detach().numpy(), r['xs'])
    assert np.abs(xt.grad.numpy() - r['dx']).max() <= 1e-12 and np.abs(st.grad.numpy() - r['ds']).max() <= 1e-12 * np.abs(r['ds']).max()


@pytest.mark.parametrize('i', [i for i, c in enumerate(MC.EPI_CASES) if c[:4] in ((3, 7, 9, 68), (1, 3, 43, 3))],
                         ids=lambda i: MC.epi_id(MC.EPI_CASES[i]))
def test_the_epilogue_restatement_agrees_with_autograd(i):
    act = MC.EPI_CASES[i][4]
    c, d, bias, noise, strength, g = MC.epi_inputs(MC.EPI_CASES[i])
    r = MC.epilogue(c, d, bias, noise, strength, g, act, np.float64)
    opt = lambda a: None if a is None else T64(a)
    ct, dt, bt, stt = T64(c), opt(d), opt(bias), opt(strength)
    p = ct if dt is None else ct * dt[:, None, None, :]
    if bt is not None:
        p = p + bt
    if noise is not None:
        p = p + stt * T64(noise, False)[..., None]
    out = MC._t_act(p, act)
    out.backward(T64(g, False))
    assert np.abs(out.detach().numpy() - r['out']).max() <= 1e-12
    for t, k in ((ct, 'dc'), (dt, 'dd'), (bt, 'dbias'), (stt, 'dstrength')):
        if t is None:
            assert r[k] is None
        else:
            assert np.abs(t.grad.numpy() - r[k]).max() <= 1e-12 * max(1.0, np.abs(r[k]).max()), k


def test_the_epilogue_inputs_stay_clear_of_the_kink():
    for i, case in enumerate(MC.EPI_CASES):
        if case[4] is None:
            continue
        c, d, bias, noise, strength, _ = MC.epi_inputs(case)
        f = np.float64
        p = c.astype(f) * (1.0 if d is None else d.astype(f)[:, None, None, :]) + (0.0 if bias is None else bias.astype(f))
        if noise is not None:
            p = p + strength.astype(f) * noise.astype(f)[..., None]
        assert np.abs(p).min() >= MC.KINK * 0.99, MC.epi_id(case)


@pytest.mark.parametrize('case', MC.LAYER_CASES, ids=str)
@pytest.mark.parametrize('act', MC.ACTS, ids=lambda a: a or 'none')
def test_the_factorised_form_is_the_definition(case, act):
    """d conv(x s, W) == conv(x, W s d) to 1e-12 in float64, forward and every gradient, with and without demodulation."""
    inp = MC.layer_inputs(case)
    for demod in (True, False):
        res = []
        for fn in (MC.layer_definition, MC.layer_factorised):
            t = {k: T64(v, k not in ('noise', 'g')) for k, v in inp.items()}
            s = 1.0 + t['w'] @ t['kernel'] + t['bias']
            out = fn(t['x'], t['weights'], s, t['biases'], t['noise'], t['noise_strength'], act, demod)
            names = ('x', 'w', 'weights', 'biases', 'noise_strength', 'kernel', 'bias')
            res.append([out.detach()] + list(torch.autograd.grad((out * t['g']).sum(), [t[k] for k in names])))
        for a, b in zip(*res):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))


def test_a_tap_layout_and_an_even_kernel_pad_like_the_package(t2i):
    """The definition's 'SAME' padding is the package's: conv_desc puts the odd pixel bottom / right."""
    from t2i_amd import kernels as K
    for k in (1, 2, 3, 4):
        d = K.conv_desc(1, 5, 5, 1, 1, k, k, 1, 1, 'SAME')[0]
        assert (d.pad_t, d.pad_l, d.Ho, d.Wo) == ((k - 1) // 2, (k - 1) // 2, 5, 5)


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
NAMES = (('t2i_modconv_chunk_rows', 0), ('t2i_demod_coef', 11), ('t2i_demod_coef_bwd', 14), ('t2i_modulate', 8),
         ('t2i_modulate_bwd_scale_workspace_bytes', 3), ('t2i_modulate_bwd_scale', 9), ('t2i_demod_act', 12),
         ('t2i_demod_act_bwd_workspace_bytes', 3), ('t2i_demod_act_bwd', 18))


def test_abi_declares_binds_and_exports_the_entries(t2i):
    from t2i_amd import _lib, kernels
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    for name, nargs in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and len(_lib.SIGNATURES[name][1]) == nargs and name + '(' in header, name
    assert kernels.MODCONV_CHUNK_ROWS == MC.CHUNK == 64 and '#define T2I_MODCONV_CHUNK_ROWS 64' in header
    assert '#define T2I_ABI_VERSION 13' in header                                       # added within v13
    assert 't2i_modconv' in open(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 'build.sh')).read()
    L = _lib.lib
    assert L.t2i_modulate_bwd_scale_workspace_bytes(8, 65536, 64) >= 8 * 1024 * 64 * 4 and L.t2i_modulate_bwd_scale_workspace_bytes(0, 4, 4) == 0
    assert L.t2i_demod_act_bwd_workspace_bytes(8, 65536, 64) >= 8 * 1024 * 3 * 64 * 4 and L.t2i_demod_act_bwd_workspace_bytes(3, 1 << 31, 1) == 0
    assert L.t2i_demod_act_bwd_workspace_bytes(1 << 20, 1 << 10, 4) == 0


def test_every_entry_refuses_bad_arguments_before_any_launch(t2i):
    """No GPU is touched: every refusal returns before the first launch, so the fake pointers are never read."""
    from t2i_amd import _lib
    L = _lib.lib
    P = ctypes.c_void_p
    a = [P(0x100000 * (i + 1)) for i in range(16)]        # distinct, 16-byte aligned, a MiB apart, never dereferenced
    ws, wsn = P(0x10000000), 1 << 20
    INVALID, WORKSPACE = -1, -2

    def coef(W=a[0], s=a[1], stride=8, T=9, Cin=8, Cout=4, B=2, eps=1e-8, q=a[2], d=a[3]):
        return L.t2i_demod_coef(W, s, stride, T, Cin, Cout, B, eps, q, d, None)

    def coefb(gd=a[4], d=a[3], s=a[1], stride=8, W=a[0], q=a[2], T=9, Cin=8, Cout=4, B=2, ds=a[5], dW=a[6], acc=0):
        return L.t2i_demod_coef_bwd(gd, d, s, stride, W, q, T, Cin, Cout, B, ds, dW, acc, None)

    def mod(x=a[0], s=a[1], stride=8, B=2, R=16, C=8, xs=a[2]):
        return L.t2i_modulate(x, s, stride, B, R, C, xs, None)

    def scale(g=a[3], x=a[0], B=2, R=16, C=8, ds=a[4], w=ws, wn=wsn):
        return L.t2i_modulate_bwd_scale(g, x, B, R, C, ds, w, wn, None)

    def act(c=a[0], d=a[1], bias=a[2], nz=a[3], st=a[4], B=2, R=16, C=8, act=2, alpha=0.0, out=a[5]):
        return L.t2i_demod_act(c, d, bias, nz, st, B, R, C, act, alpha, out, None)

    def actb(g=a[6], c=a[0], d=a[1], bias=a[2], nz=a[3], st=a[4], B=2, R=16, C=8, act=2, alpha=0.0, dc=a[7], dd=a[8], db=a[9], dst=a[10], w=ws, wn=wsn):
        return L.t2i_demod_act_bwd(g, c, d, bias, nz, st, B, R, C, act, alpha, dc, dd, db, dst, w, wn, None)

    def refused(f, want=INVALID, **kw):
        assert f(**kw) == want, (f.__name__, kw)
        assert L.t2i_last_error()

    for f in (coef, coefb):
        for kw in (dict(W=None), dict(s=None), dict(T=0), dict(Cin=0), dict(Cout=0), dict(B=0), dict(stride=7), dict(Cin=1 << 16, Cout=1 << 15, stride=1 << 16),
                   dict(T=1 << 12, Cin=1 << 10, Cout=1 << 10, stride=1 << 10), dict(B=1 << 20, Cout=1 << 11), dict(B=1 << 20, stride=1 << 11)):
            refused(f, **kw)
    for kw in (dict(q=None), dict(d=None), dict(eps=-1.0), dict(eps=float('nan')), dict(eps=float('inf')), dict(q=a[0]), dict(d=a[1]), dict(q=a[3])):
        refused(coef, **kw)
    for kw in (dict(gd=None), dict(d=None), dict(q=None), dict(dW=a[0]), dict(ds=a[1]), dict(ds=a[6]), dict(dW=a[4])):
        refused(coefb, **kw)
    for f in (mod, scale, act, actb):
        for kw in (dict(B=0), dict(R=0), dict(C=0), dict(R=1 << 31), dict(B=1 << 16, R=1 << 10, C=64)):
            refused(f, **kw)
    for kw in (dict(x=None), dict(s=None), dict(xs=None), dict(stride=7), dict(xs=a[0]), dict(xs=a[1]), dict(B=1 << 10, stride=1 << 21, R=1, C=8)):
        refused(mod, **kw)
    for kw in (dict(g=None), dict(x=None), dict(ds=None), dict(ds=a[0]), dict(ds=a[3])):
        refused(scale, **kw)
    for f in (act, actb):
        for kw in (dict(c=None), dict(act=3), dict(act=7), dict(act=1, alpha=-0.1), dict(act=1, alpha=float('nan')), dict(nz=None), dict(st=None)):
            refused(f, **kw)
    for kw in (dict(out=None), dict(out=a[0]), dict(out=a[1]), dict(out=a[2]), dict(out=a[3]), dict(out=a[4])):
        refused(act, **kw)
    for kw in (dict(g=None), dict(dc=None, dd=None, db=None, dst=None), dict(nz=None, st=None), dict(d=None), dict(dc=a[0]), dict(dc=a[6]),
               dict(dd=a[1]), dict(db=a[7]), dict(dst=a[9])):
        refused(actb, **kw)                                # ... dstrength without noise, dd without d, overlaps
    for f in (scale, actb):
        for kw in (dict(w=None), dict(w=P(0x10000004)), dict(wn=16)):
            refused(f, WORKSPACE, **kw)
    # ... and each says what it refused
    for call, words in ((lambda: coef(stride=7), 't2i_demod_coef: .*style rows 7 floats apart'), (lambda: coef(eps=-1.0), 't2i_demod_coef: .*eps -1'),
                      (lambda: coefb(dW=a[0]), 't2i_demod_coef_bwd: .*overlaps'), (lambda: mod(xs=a[0]), 't2i_modulate: .*xs overlaps x'),
                      (lambda: mod(R=1 << 31), 't2i_modulate: .*2\\^31 elements'), (lambda: scale(wn=16), 't2i_modulate_bwd_scale: workspace .*16 bytes where'),
                      (lambda: act(act=3), 't2i_demod_act: .*act 3'), (lambda: act(act=1, alpha=-0.1), 't2i_demod_act: .*lrelu slope -0.1'),
                      (lambda: act(nz=None), 't2i_demod_act: .*noise and strength come together'), (lambda: act(B=0), 't2i_demod_act: .*every size must be at least 1'),
                      (lambda: actb(nz=None, st=None), 't2i_demod_act_bwd: .*dstrength without noise'), (lambda: actb(d=None), 't2i_demod_act_bwd: .*dd without d'),
                      (lambda: actb(g=None), 't2i_demod_act_bwd: .*NULL pointer')):
        assert call() < 0 and re.match(words, L.t2i_last_error().decode()), (words, L.t2i_last_error().decode())


def test_modulated_conv2d_refusals(t2i):
    from t2i_amd import kernels as K, scope as S, stacked as ST
    from t2i_amd.utils import ops
    S.set_default_store(S.VariableStore(device='cpu', seed=0))
    x, w, nz = torch.zeros(2, 4, 4, 8), torch.zeros(2, 6), torch.zeros(2, 4, 4)
    with K.dry_run(), torch.no_grad(), S.variable_scope('t'):
        assert ops.modulated_conv2d(x, w, 12, noise=nz, act=ops.relu).shape == (2, 4, 4, 12)                      # the accepted calls
        assert ops.modulated_conv2d(x, w, 5, ks=(1, 1), act=ops.lrelu_act(0.2), demodulate=False).shape == (2, 4, 4, 5)
        st = S.default_store()
        assert [(n, tuple(v.shape)) for n, v in st.vars.items()] == [
            ('t/ModConv/weights', (3, 3, 8, 12)), ('t/ModConv/biases', (12,)), ('t/ModConv/noise_strength', (12,)), ('t/ModConv/style/kernel', (6, 8)),
            ('t/ModConv/style/bias', (8,)), ('t/ModConv_1/weights', (1, 1, 8, 5)), ('t/ModConv_1/biases', (5,)), ('t/ModConv_1/style/kernel', (6, 8)),
            ('t/ModConv_1/style/bias', (8,))]
        assert float(st.vars['t/ModConv/biases'].abs().max()) == 0.0 and float(st.vars['t/ModConv/noise_strength'].abs().max()) == 0.0
        assert float(st.vars['t/ModConv/style/bias'].abs().max()) == 0.0
        std = float(st.vars['t/ModConv/weights'].std())
        assert 0.5 * math.sqrt(2.0 / 72) < std < 1.2 * math.sqrt(2.0 / 72)             # He over kh kw Cin (truncated)
        bad = [
            (dict(x=x.bfloat16()), 'float32'), (dict(x=x[0]), 'rank-4'), (dict(x=x.permute(0, 2, 1, 3)), 'x must be physically NHWC'),
            (dict(w=torch.zeros(3, 6)), 'w must be'), (dict(w=torch.zeros(2, 6, 1)), 'w must be'), (dict(w=w.double()), 'w must be'),
            (dict(w=w.bfloat16()), 'w must be'), (dict(f=0), 'f must be'), (dict(f=2.0), 'f must be'), (dict(ks=(0, 3)), 'ks must be'),
            (dict(noise=torch.zeros(2, 4, 5)), 'noise must be'), (dict(noise=nz.double()), 'noise must be'),
            (dict(noise=torch.zeros(2, 4, 8)[:, :, ::2]), 'noise must be contiguous'), (dict(noise=nz.clone().requires_grad_(True)), 'requires a gradient'),
            (dict(act=ops.lrelu_act(-0.1)), 'negative slope'), (dict(act=ops.tanh), 'act must be'), (dict(act=torch.relu), 'act must be'),
            (dict(demodulate=1), 'demodulate must be'), (dict(eps=-1.0), 'eps must be'), (dict(eps=float('nan')), 'eps must be'),
        ]
        before = list(st.vars)
        for kw, word in bad:
            args = dict(x=x, w=w, f=12, noise=nz, act=ops.relu)
            args.update(kw)
            with pytest.raises(ValueError, match='modulated_conv2d.*' + word):
                ops.modulated_conv2d(args.pop('x'), args.pop('w'), args.pop('f'), **args)
        for kw in (dict(x=ST.Stacked(x, x)), dict(w=ST.Stacked(w, w))):
            args = dict(x=x, w=w)
            args.update(kw)
            with pytest.raises(NotImplementedError, match='modulated_conv2d.*stacked'):
                ops.modulated_conv2d(args['x'], args['w'], 12)
        assert list(st.vars) == before                     # a refused call creates no variable
    with pytest.raises(RuntimeError, match='no CPU path'), S.variable_scope('t', reuse=True):     # outside a dry run a CPU tensor is no fallback
        ops.modulated_conv2d(x, w, 12, name='ModConv')


def test_a_second_differentiation_is_refused_with_adains_sentence(t2i):
    from t2i_amd import autograd as A
    with pytest.raises(NotImplementedError) as mine:
        A._FirstOrder.backward(type('C', (), {'op': 'modulated_conv2d'})())
    with pytest.raises(NotImplementedError) as theirs:
        A.AdaINBwdFn.backward(None)
    assert str(mine.value).split(': ', 1)[1] == str(theirs.value).split(': ', 1)[1] and str(mine.value).startswith('modulated_conv2d: ')


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def _pggan(**kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    args = dict(fmap_base=64, fmap_max=32, z_dim=16, embed_dim=32, compr_embed_dim=8, device='cpu')
    args.update(kw)
    stage, trans = args.pop('stage', 2), args.pop('trans', True)
    return PGGAN(4, 100, None, None, None, None, None, stage, trans, **args)


def _cfg():
    from oracle import torch_pggan as PG
    return PG.Cfg(z_dim=16, embed_dim=32, compressed=8, batch=4, base=64, cap=32)


def test_option_validation_and_flags(t2i):
    from t2i_amd.models.pggan import options as cli
    for kw, word in ((dict(modulated_conv=True), 'modulated_conv needs style_dim'), (dict(style_dim=16, modulated_conv=1), 'modulated_conv must be'),
                     (dict(style_dim=16, modulated_conv='yes'), 'modulated_conv must be')):
        with pytest.raises(ValueError, match=word):
            _pggan(build_model=False, **kw)
    assert _pggan(build_model=False, style_dim=16, modulated_conv=True).modulated_conv is True
    assert _pggan(build_model=False, style_dim=16).modulated_conv is False and _pggan(build_model=False).modulated_conv is False
    assert cli.flag('modulated_conv') == '--modulated-conv'

    def parse(argv, reader=True, full=False):
        ap = argparse.ArgumentParser()
        (cli.add_trainer_arguments if full else lambda ap: cli.add_style_arguments(ap, reader=reader))(ap)
        return cli.kwargs_of(ap, ap.parse_args(argv))
    assert parse([]) == {} and parse(['--style-dim', '16']) == {'style_dim': 16}
    for reader in (True, False):
        assert parse(['--style-dim', '16', '--modulated-conv'], reader) == {'style_dim': 16, 'modulated_conv': True}
    assert parse(['--style-dim', '8', '--modulated-conv', '--equalized-lr'], full=True) == {'style_dim': 8, 'modulated_conv': True, 'equalized_lr': True}
    for full in (False, True):
        with pytest.raises(SystemExit) as e:
            parse(['--modulated-conv'], full=full)
        assert e.value.code == 2


def test_the_trainer_refuses_the_flag_alone_before_a_directory_is_made(t2i, tmp_path, capsys):
    from t2i_amd.models.pggan import train_pggan as TP
    out = str(tmp_path / 'run')
    with pytest.raises(SystemExit) as e:
        TP.main(['--out', out, '--modulated-conv'])
    assert e.value.code == 2 and not os.path.exists(out)
    assert '--modulated-conv needs --style-dim' in capsys.readouterr().err


@pytest.mark.parametrize('stage,trans', [(1, False), (2, True), (3, False)])
def test_the_model_and_its_restatement_name_the_same_variables_in_order(t2i, stage, trans):
    from t2i_amd.models.pggan.pggan import W_AVG
    m = _pggan(stage=stage, trans=trans, style_dim=16, modulated_conv=True)
    want = MC.modconv_variables(_cfg(), stage, trans, 16)
    assert [(n, tuple(v.shape)) for n, v in m.g_vars.items()] == want                   # names, shapes and creation order
    mine = [n for n in m.store.vars if n.startswith('g_net')]
    assert [n for n in mine if n != W_AVG] == [n for n, _ in want] and mine.index(W_AVG) == [n for n, _ in want].index('g_net/conv_stage_0/ModConv/weights')
    assert not any('/Conv' in n and '/rgb_stage' not in n for n in mine) and not any('StyleMod' in n for n in mine)
    assert 'g_net/conv_stage_0/LayerNorm/gamma' in mine and not any('LayerNorm_1' in n for n in mine)           # the trunk's norm stays, no other
    assert [k for k, _ in m.style_noise_keys()] == ['style_noise_%s_%d' % (t, k) for t in 'dg' for k in range(2 * stage)]
    assert [s for _, s in m.style_noise_keys()] == MC.block_sizes(stage) * 2
    keep = m.get_variables_up_to_stage(stage)
    assert {n for n in mine if '/ModConv' in n or n.startswith('g_net/mapping/')} <= set(keep)
    quiet = _pggan(stage=stage, trans=trans, style_dim=16, modulated_conv=True, style_noise=False)
    assert [(n, tuple(v.shape)) for n, v in quiet.g_vars.items()] == MC.modconv_variables(_cfg(), stage, trans, 16, noise=False)


def test_kernel_scales_of_the_new_variables(t2i):
    m = _pggan(style_dim=16, modulated_conv=True, equalized_lr=True)
    scales = m.kernel_scales(m.g_vars)
    seen = 0
    for n, v in m.g_vars.items():
        if n.endswith('/ModConv/weights') or n.endswith('/ModConv_1/weights'):
            assert scales[n] == math.sqrt(2.0 / (9 * v.shape[2])), n                  # a convolution's weights: kh kw Cin
            seen += 1
        elif n.endswith('/style/kernel'):
            assert scales[n] == math.sqrt(2.0 / 16), n                                # a dense kernel: w_dim
            seen += 1
        elif '/ModConv' in n:
            assert n not in scales, n                                                 # biases, noise strengths
    assert seen == 8 and m.G_optimizer.slot_scales['g_net/conv_stage_1/ModConv/style/kernel'] == (math.sqrt(2.0 / 16),) * 2
    assert _pggan(style_dim=16, modulated_conv=True).kernel_scales(m.g_vars) is None


@pytest.mark.parametrize('stage,trans', [(1, False), (2, True), (3, False)])
def test_the_default_and_the_adain_models_are_todays(t2i, stage, trans):
    from oracle import torch_pggan as PG
    from t2i_amd.models.pggan.pggan import W_AVG
    m = _pggan(stage=stage, trans=trans)
    ref = PG.init_variables(_cfg(), stage, trans)
    assert [(n, tuple(v.shape)) for n, v in m.store.vars.items()] == [(n, tuple(v.shape)) for n, v in ref.items()]
    s = _pggan(stage=stage, trans=trans, style_dim=16)
    V = PG.Vars(None, 0, torch.float64)
    nz = [torch.zeros(4, k, k, dtype=torch.float64) for k in SC.style_block_sizes(stage)]
    with torch.no_grad():
        SC.style_generator(V, _cfg(), torch.zeros(4, 16, dtype=torch.float64), torch.zeros(4, 32, dtype=torch.float64), stage, trans, 0.3, None, 16, 4, nz)
    assert [(n, tuple(v.shape)) for n, v in s.g_vars.items()] == [(n, tuple(v.shape)) for n, v in V.P.items()]
    assert not any('ModConv' in n for n in list(m.store.vars) + list(s.store.vars)) and W_AVG in s.store.vars


def test_what_the_checkpoint_names_say(t2i):
    from t2i_amd.models.pggan import options as O
    names = lambda m: {n: tuple(v.shape) for n, v in m.store.vars.items()}
    plain, adain, mod = _pggan(), _pggan(style_dim=16), _pggan(style_dim=16, modulated_conv=True)
    quiet = _pggan(style_dim=8, mapping_layers=2, style_noise=False, modulated_conv=True)
    assert [O.modulated_of_names(names(m)) for m in (plain, adain, mod, quiet)] == [False, False, True, True]
    assert O.style_of_names(names(mod)) == (16, 4, True) == O.style_of_names(names(adain)) and O.style_of_names(names(quiet)) == (8, 2, False)
    assert O.style_of_names(names(plain)) == (None, None, None)
    assert '--modulated-conv' in O.describe_modulated(True) and 'no --modulated-conv' in O.describe_modulated(False)


def test_a_reader_refuses_each_mismatched_checkpoint_and_keeps_its_weights(t2i, tmp_path):
    from t2i_amd.models.pggan import eval_pggan as E
    from t2i_amd.utils.saver import Saver, save
    made = {}
    for kind, kw in (('plain', {}), ('adain', dict(style_dim=16)), ('mod', dict(style_dim=16, modulated_conv=True))):
        m = _pggan(stage=1, trans=False, seed=3, **kw)
        d = str(tmp_path / kind / 'stage1') + '/'
        save(Saver(m.store, var_list=m.get_variables_up_to_stage(1)), None, d, 7)
        made[kind] = (d, kw)
    assert any('/ModConv' in n for n in E.checkpoint_names(made['mod'][0])) and not any('/ModConv' in n for n in E.checkpoint_names(made['adain'][0]))
    refusals = {('adain', 'mod'): r'convolution \+ AdaIN layers \(no --modulated-conv\).*built with weight-demodulated convolutions \(--modulated-conv\)',
                ('mod', 'adain'): r'weight-demodulated convolutions \(--modulated-conv\).*built with convolution \+ AdaIN layers.*pass --modulated-conv',
                ('adain', 'plain'): r'--style-dim 16.*no --style-dim', ('mod', 'plain'): r'--style-dim 16.*no --style-dim',
                ('plain', 'mod'): r"the reference's generator.*--style-dim 16", ('plain', 'adain'): r"the reference's generator.*--style-dim 16"}
    for (ckpt, reader), message in refusals.items():
        m = _pggan(stage=1, trans=False, seed=11, **made[reader][1])
        m.check_dir_read = made[ckpt][0]
        before = {n: v.detach().clone() for n, v in m.store.vars.items()}
        with pytest.raises(RuntimeError, match=message):
            E.restore_generator(m)
        assert list(m.store.vars) == list(before) and all(torch.equal(v, before[n]) for n, v in m.store.vars.items()), (ckpt, reader)
    for kind in made:                                                                   # and every matching pair restores
        m = _pggan(stage=1, trans=False, seed=11, **made[kind][1])
        m.check_dir_read = made[kind][0]
        E.restore_generator(m)
        src = np.load(os.path.join(made[kind][0], 'model-7.npz'))
        assert all(np.array_equal(src[n], v.detach().numpy()) for n, v in m.store.vars.items() if n.startswith('g_net') and n in src.files), kind
