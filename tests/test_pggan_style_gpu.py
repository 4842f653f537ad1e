"""PGGAN(style_dim=16) on the GPU against the float64 restatement of tests/style_cases.py, tiny widths
(fmap_base 64, fmap_max 32, z 16, embedding 32 -> 8, B = 4), every noise fed: the generator image, every generator gradient of one G step
and the D step's scalars at (stage 1, stable), (stage 2, transition), (stage 3, stable); graphs against eager; the checkpoint round trip
and the readers' refusal; truncation; style_noise=False; g_ema + equalized_lr.

Parity measured on an MI355X (bound 1e-4; the largest of image, scalars and every generator gradient, relative to the largest
reference entry): stage 1 1.3e-6, stage 2 transition 3.1e-6, stage 3 7.9e-6."""
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

pytestmark = pytest.mark.gpu

TINY = dict(fmap_base=64, fmap_max=32, z_dim=16, embed_dim=32, compr_embed_dim=8)
B, D, STEPS = 4, 16, 10


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    return torch.device('cuda')


def model(dev, stage, trans, seed=0, **kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    args = dict(TINY, style_dim=D)
    args.update(kw)
    return PGGAN(B, STEPS, None, None, None, None, None, stage, trans, device=dev, seed=seed, **args)


def cfg():
    from oracle import torch_pggan as PG
    return PG.Cfg(z_dim=16, embed_dim=32, compressed=8, batch=B, base=64, cap=32)


def liven(m, seed=3):
    """Variables that start at zero (noise strengths, biases) get values, so that every path carries signal."""
    rng = np.random.default_rng(seed)
    vals = {}
    for n, v in m.store.vars.items():
        if n.endswith('noise_strength'):
            vals[n] = rng.uniform(-0.5, 0.5, tuple(v.shape))
        elif n.endswith('/bias') or n.endswith('/biases'):
            vals[n] = 0.1 * rng.standard_normal(tuple(v.shape))
    m.store.load(vals)


def feeds(stage, dev, seed=1, style=True):
    """-> (float64 CPU feed, float32 device feed) with the CA noise, eps and (style) one noise image per style block and step."""
    from oracle import torch_pggan as PG
    f64 = PG.synthetic_feed(cfg(), stage, seed=seed)
    rng = np.random.default_rng(100 + seed)
    if style:
        for tag in 'dg':
            for k, s in enumerate(SC.style_block_sizes(stage)):
                f64['style_noise_%s_%d' % (tag, k)] = torch.tensor(rng.standard_normal((B, s, s)).astype(np.float32).astype(np.float64))
    f32 = {k: v.to(torch.float32).to(dev) for k, v in f64.items()}
    f32['eps_graph'] = f32.pop('eps')
    f64 = {k: v.to(torch.float32).to(torch.float64) for k, v in f64.items()}         # the float32 values, exactly
    return f64, f32


def relerr(got, ref):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def reference_steps(P, f, stage, trans, alpha):
    """The D step's scalars and the G step (image, losses, every generator gradient) in float64."""
    from oracle import torch_pggan as PG
    from oracle.torch_stackgan import kl_loss
    c = cfg()
    nz = lambda tag: [f['style_noise_%s_%d' % (tag, k)] for k in range(2 * stage)]
    gen = lambda Q, tag: SC.style_generator(PG.Vars(Q), c, f['z'], f['cond'], stage, trans, alpha, f['ca_noise_' + tag], D, 4, nz(tag))
    with torch.no_grad():
        G = gen(P, 'd')[0]
        Dd = lambda img: PG.discriminator(PG.Vars(P), c, img, f['cond'], stage, trans, alpha)
        Dg, Dx, Dxmi = Dd(G), Dd(f['x']), Dd(f['x_mismatch'])
    eps = f['eps'].reshape(-1, 1, 1, 1)
    x_hat = (eps * G + (1.0 - eps) * f['x']).detach().requires_grad_(True)
    cond_inp = f['cond'].detach().clone().requires_grad_(True)
    Dxh = PG.discriminator(PG.Vars(P), c, x_hat, cond_inp, stage, trans, alpha)
    gx, gc = torch.autograd.grad(Dxh.sum(), [x_hat, cond_inp])
    gp, gp2 = PG._gp(gx), PG._gp(gc)
    wdist, wdist2 = Dx.mean() - Dg.mean(), Dx.mean() - Dxmi.mean()
    d = dict(D_loss=float(-wdist - wdist2 + c.gp_coeff * (gp + gp2)), wdist=float(wdist), wdist2=float(wdist2), real_gp=float(gp),
             real_gp2=float(gp2), G=G)
    names = PG.trainable(P, 'g_net')
    Q = dict(P)
    for n in names:
        Q[n] = P[n].detach().requires_grad_(True)
    Gg, mean, log_sigma, w = gen(Q, 'g')
    Dgg = PG.discriminator(PG.Vars(Q), c, Gg, f['cond'], stage, trans, alpha)
    kl = kl_loss(mean, log_sigma)
    loss = -Dgg.mean() + c.kl_coeff * kl
    grads = torch.autograd.grad(loss, [Q[n] for n in names])
    g = dict(G_loss=float(loss), G_kl_loss=float(kl), G=Gg.detach(), w=w.detach(), grads=dict(zip(names, grads)))
    return d, g


@pytest.mark.parametrize('stage,trans', [(1, False), (2, True), (3, False)], ids=['stage1', 'stage2t', 'stage3'])
def test_one_d_and_g_step_against_float64(dev, stage, trans):
    from t2i_amd.models.pggan.pggan import W_AVG
    m = model(dev, stage, trans)
    liven(m)
    P = {n: torch.tensor(a, dtype=torch.float64) for n, a in m.store.state().items() if n != W_AVG}
    f64, f32 = feeds(stage, dev)
    alpha = 0.3
    m.set_alpha(alpha)
    dref, gref = reference_steps(P, f64, stage, trans, alpha)
    d = m.d_losses(f32)
    worst = [('d/G', relerr(d['G'], dref['G']))]
    for k in ('D_loss', 'wdist', 'wdist2', 'real_gp', 'real_gp2'):
        err = abs(float(d[k]) - dref[k]) / max(abs(dref[k]), 1.0)
        worst.append(('d/' + k, err))
        assert err <= 1e-4, (k, float(d[k]), dref[k])
    g = m.g_losses(f32)
    worst.append(('g/G', relerr(g['G'], gref['G'])))
    for k in ('G_loss', 'G_kl_loss'):
        assert abs(float(g[k]) - gref[k]) <= 1e-4 * max(abs(gref[k]), 1.0), (k, float(g[k]), gref[k])
    assert set(m.g_vars) == set(gref['grads'])
    bad = []
    for n in m.g_vars:
        ref = gref['grads'][n].numpy()
        got = m.g_arena.grad_of(n)
        if np.abs(ref).max() < 1e-9:
            err = float(got.abs().max())
        else:
            err = relerr(got, ref)
        worst.append(('g/grad/' + n, err))
        if err > 1e-4:
            bad.append((n, err))
    worst.sort(key=lambda t: -t[1])
    print('pggan style stage %d%s: largest errors %s' % (stage, 't' if trans else '', ', '.join('%s %.2e' % t for t in worst[:4])))
    assert dict(worst)['d/G'] <= 1e-4 and dict(worst)['g/G'] <= 1e-4, worst[:4]
    assert not bad, bad
    # the truncation's centre moved towards the batch mean of w by 1 - 0.995
    w_avg = m.store.vars[W_AVG].detach().double().cpu().numpy()
    assert np.abs(w_avg - 0.005 * gref['w'].mean(0).numpy()).max() <= 1e-4 * 0.005 * max(float(gref['w'].abs().max()), 1e-30) + 1e-12


def _run(dev, use_graphs, fs, stage=2, trans=True, **kw):
    m = model(dev, stage, trans, **kw)
    liven(m)
    m.iteration(1, fs[0])
    if use_graphs:
        m.enable_graphs(fs[0])
    outs = [m.iteration(2 + 2 * i, fs[1 + i]) for i in range(2)]
    torch.cuda.synchronize()
    return m, {n: v.detach().clone() for n, v in m.store.vars.items()}, (float(outs[-1]['d']['D_loss']), float(outs[-1]['g']['G_loss']))


def test_graph_replay_matches_eager_and_redraws_the_style_noise(dev):
    """Two replayed iterations == two eager ones, bit for bit (tests/test_pggan.py's comparison), with every noise fed; without fed style
    noise the static buffers are re-drawn before every replay."""
    fs = [feeds(2, dev, seed=s)[1] for s in (1, 2, 3)]
    (_, s0, l0), (_, s1, l1) = _run(dev, False, fs), _run(dev, True, fs)
    assert l0 == l1
    for n in s0:
        assert torch.equal(s0[n], s1[n]), n
    bare = [feeds(2, dev, seed=s, style=False)[1] for s in (1, 2)]
    m = model(dev, 2, True)
    m.iteration(1, bare[0])
    m.enable_graphs(bare[0])
    keys = [k for k, _ in m.style_noise_keys()]
    assert len(keys) == 8 and all(k in m._graphs.static for k in keys)
    seen = [{k: m._graphs.static[k].clone() for k in keys}]
    for i in (2, 3):
        m.iteration(i, bare[1])
        torch.cuda.synchronize()
        seen.append({k: m._graphs.static[k].clone() for k in keys})
    for k in keys:
        assert not torch.equal(seen[0][k], seen[1][k]) and not torch.equal(seen[1][k], seen[2][k]), k
        assert abs(float(seen[2][k].mean())) < 1.0 and 0.3 < float(seen[2][k].std()) < 3.0, k


def test_checkpoint_round_trip_and_the_readers_refusal(dev, tmp_path):
    from t2i_amd.models.pggan import eval_pggan as E
    from t2i_amd.models.pggan.pggan import W_AVG
    from t2i_amd.utils.saver import Saver, load, save
    f = feeds(2, dev)[1]
    a = model(dev, 2, True, adam_lr=1e-3)
    liven(a)
    a.iteration(1, f)
    d = str(tmp_path / 'stage2') + '/'
    save(Saver(a.store, var_list=a.get_variables_up_to_stage(2)), None, d, 1)
    b = model(dev, 2, False, seed=5)
    ok, step = load(Saver(b.store, var_list=b.get_variables_up_to_stage(2)), None, d)
    assert ok and step == 1
    names = [n for n in a.store.vars if n.startswith('g_net/mapping/') or '/StyleMod' in n]
    assert W_AVG in names and len(names) == 8 + 1 + 4 * 3
    for n in names:
        assert torch.equal(a.store.vars[n], b.store.vars[n]), n
    assert float(a.store.vars[W_AVG].abs().max()) > 0.0
    reader = E.stage_model(type('C', (), {'CHECKPOINT_DIR': str(tmp_path)})(), 2, B, None, dev, **TINY)
    with pytest.raises(RuntimeError, match=r'--style-dim 16 --mapping-layers 4.*no --style-dim.*pass the same --style-dim'):
        E.restore_generator(reader)
    styled = E.stage_model(type('C', (), {'CHECKPOINT_DIR': str(tmp_path)})(), 2, B, None, dev, style_dim=D, **TINY)
    E.restore_generator(styled)
    for n in names:
        assert torch.equal(a.store.vars[n], styled.store.vars[n]), n


def test_truncation(dev):
    from t2i_amd.models.pggan.pggan import W_AVG
    m = model(dev, 2, False)
    liven(m)
    _, f = feeds(2, dev)
    m.iteration(1, f)                                                 # w_avg leaves zero
    noise = [f['style_noise_g_%d' % k] for k in range(4)]
    z1, z2, cond = f['z'], f['z'].flip(0) * 0.7 + 0.1, f['cond']

    def sample(z, **kw):
        torch.cuda.manual_seed(5)                                     # the conditioning noise is drawn: the same draw every time
        return m.sampler(z, cond, noise=noise, **kw)
    plain = sample(z1)
    assert torch.equal(sample(z1, truncation_psi=1.0), plain) and torch.equal(sample(z1), plain)
    assert not torch.equal(sample(z1, truncation_psi=0.5), plain)
    w_avg = m.store.vars[W_AVG].detach()
    # psi = 0: every sample's style is w_avg itself, whatever z is.  (The 4x4 trunk still reads [z, c], so the IMAGES of two z differ;
    # what psi = 0 removes is the mapping network's output: with other mapping weights the image stays the same, bit for bit.)
    a = sample(z1, truncation_psi=0.0)
    assert torch.equal(m._w_used, w_avg.expand(B, D))
    sample(z2, truncation_psi=0.0)
    assert torch.equal(m._w_used, w_avg.expand(B, D))
    kept = {n: v.detach().clone() for n, v in m.store.vars.items() if n.startswith('g_net/mapping/dense')}
    m.store.load({n: (v * -1.7 + 0.3).cpu().numpy() for n, v in kept.items()})
    assert torch.equal(sample(z1, truncation_psi=0.0), a) and not torch.equal(sample(z1), plain)
    m.store.load({n: v.cpu().numpy() for n, v in kept.items()})
    assert torch.equal(sample(z1), plain)
    fresh = m.sampler(z1, cond)                                       # fresh style noise unless given
    assert fresh.shape == plain.shape and not torch.equal(fresh, m.sampler(z1, cond))
    with pytest.raises(ValueError, match='one more'):
        m.sampler(z1, cond, noise=noise[:3])


def test_style_noise_off_and_ema_with_equalized_lr(dev):
    _, f = feeds(2, dev, style=False)
    quiet = model(dev, 2, True, style_noise=False)
    assert not any(n.endswith('noise_strength') for n in quiet.store.vars)
    out = quiet.iteration(1, f)
    assert np.isfinite(float(out['d']['D_loss'])) and np.isfinite(float(out['g']['G_loss']))
    m = model(dev, 2, True, g_ema=0.9, equalized_lr=True, adam_lr=1e-3)
    before = m.g_arena.flat.detach().clone()
    out = m.iteration(1, feeds(2, dev)[1])
    torch.cuda.synchronize()
    assert np.isfinite(float(out['g']['G_loss']))
    opt, a = m.G_optimizer, m.g_arena
    assert opt.ema.shape == a.flat.shape and bool(torch.isfinite(opt.ema).all())
    for n in ('g_net/mapping/dense_2/kernel', 'g_net/conv_stage_1/StyleMod/style/kernel', 'g_net/conv_stage_0/StyleMod_1/noise_strength'):
        o, k = a.offsets[n]
        w0, w1, e = before[o:o + k], a.flat[o:o + k], opt.ema[o:o + k]
        assert not torch.equal(w0, w1), n                             # the variable stepped ...
        assert float((e - (0.9 * w0 + 0.1 * w1)).abs().max()) <= 1e-6 * max(float(w1.abs().max()), 1e-3), n      # ... and its shadow followed
    with m.ema_weights():
        img = m.sampler(f['z'], f['cond'])
    assert bool(torch.isfinite(img).all())


def test_train_pggan_main_with_the_style_flags_and_a_reader_of_its_checkpoint(dev, tmp_path):
    """Stages 1 -> 2t -> 2 on synthetic data through the entry point (full widths): every entry restores the previous one's mapping
    network, style variables and w_avg; the checkpoint carries shadows for the trainable ones and none for w_avg; the reader restores the
    averaged generator (w_avg from its own key) and samples with a truncation."""
    from t2i_amd.models.pggan import eval_pggan as E
    from t2i_amd.models.pggan import train_pggan as TP
    from t2i_amd.models.pggan.pggan import W_AVG
    out = str(tmp_path / 'run')
    records = TP.main(['--out', out, '--style-dim', '32', '--mapping-layers', '2', '--g-ema', '0.999', '--lr', '1e-3', '--iters', '3',
                       '--first', '0', '--last', '2'])
    assert [(r['stage'], r['trans']) for r in records] == [(1, False), (2, True), (2, False)]
    assert W_AVG in records[1]['restored'][2] and W_AVG in records[2]['restored'][2]
    z = np.load(os.path.join(out, 'checkpoints', 'stage2', 'model-2.npz'))
    ema = '/ExponentialMovingAverage'
    assert tuple(z[W_AVG].shape) == (32,) and float(np.abs(z[W_AVG]).max()) > 0.0 and W_AVG + ema not in z.files
    for n in ('g_net/mapping/dense_1/kernel', 'g_net/conv_stage_1/StyleMod_1/noise_strength', 'g_net/conv_stage_1/StyleMod/style/kernel'):
        assert n in z.files and n + ema in z.files and np.isfinite(z[n]).all(), n
    assert 'g_net/mapping/dense_2/kernel' not in z.files
    cfg_like = type('C', (), {'CHECKPOINT_DIR': os.path.join(out, 'checkpoints')})()
    m = E.stage_model(cfg_like, 2, 4, None, dev, style_dim=32, mapping_layers=2, truncation_psi=0.7)
    E.restore_generator(m, ema=True)
    assert np.array_equal(m.store.vars[W_AVG].detach().cpu().numpy(), z[W_AVG])
    assert np.array_equal(m.store.vars['g_net/mapping/dense_1/kernel'].detach().cpu().numpy(), z['g_net/mapping/dense_1/kernel' + ema])
    img = E.generate(m, torch.randn(4, 128, device=dev), torch.randn(4, 1024, device=dev))
    assert tuple(img.shape) == (4, 8, 8, 3) and bool(torch.isfinite(img).all())
    wrong = E.stage_model(cfg_like, 2, 4, None, dev, style_dim=32)
    with pytest.raises(RuntimeError, match=r'--mapping-layers 2.*--mapping-layers 4'):
        E.restore_generator(wrong)
