"""PGGAN(critic_sn=...) at stage 2, batch 4, the tiny widths of tests/test_pggan_diffaug_gpu.py.  False is today's model bit for bit
(arenas after an iteration, the keys of a checkpoint).  True: the critic's gradients are, bit for bit, those of a model without the flag
that was loaded with the normalised weights — which ties the flag to the float64-checked critic path without a tolerance of its own —
and one critic step moves raw, u, sigma and the variables as the float64 restatement (tests/sn_cases.py) says, at the bounds of
tests/test_spectral_gpu.py (1e-5 forward, 1e-4 gradients).  Eager and hipGraph replay agree bit for bit; a checkpoint carries the four
state tensors of every kernel; a checkpoint written without the flag is synced; the generator step does not see the flag."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import sn_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = dict(z_dim=8, embed_dim=32, compressed=16, batch=4, base=32, cap=16)           # tests/test_pggan_diffaug_gpu.py's
WIDTHS = dict(fmap_base=TINY['base'], fmap_max=TINY['cap'], z_dim=TINY['z_dim'], embed_dim=TINY['embed_dim'], compr_embed_dim=TINY['compressed'])
STEPS, BATCH, STAGE = 10, 4, 2
FWD, GRAD = 1e-5, 1e-4
LR = 1e-3                                                                              # (the reference's 2e-6 would move raw by a few ulps)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    return PG


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _model(trans=False, seed=5, dirs=(None, None), dataset=None, sample=None, **kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    return PGGAN(BATCH, STEPS, dirs[0], dirs[1], dataset, sample, None, STAGE, trans, device=torch.device('cuda'), seed=seed, **WIDTHS, **kw)


def _feeds(PG, count=3):
    cfg = PG.Cfg(**TINY)
    feeds = []
    for s in range(1, count + 1):
        f = {k: v.float().cuda() for k, v in PG.synthetic_feed(cfg, STAGE, seed=s).items()}
        feeds.append({'x': f['x'], 'x_mismatch': f['x_mismatch'], 'cond': f['cond'], 'z': f['z'], 'eps_graph': f['eps'],
                      'ca_noise_d': f['ca_noise_d'], 'ca_noise_g': f['ca_noise_g']})
    return feeds


def _use(m):
    """The layers look their variables up in the default store, which is the store of the model built last."""
    from t2i_amd import scope as S
    S.set_default_store(m.store)


def _spectral(m):
    sn = m.critic_spectral
    torch.cuda.synchronize()
    return {k: t.detach().clone() for k, t in (('raw', sn.raw), ('u', sn.u), ('v', sn.v), ('sigma', sn.sigma), ('flat', m.d_arena.flat))}


def _twin_with_the_weights_of(m, **kw):
    """A model without the flag whose variables are m's: the critic's are m's NORMALISED weights."""
    from t2i_amd import kernels as K
    twin = _model(**kw)
    assert twin.critic_spectral is None and list(twin.store.vars) == list(m.store.vars)
    with torch.no_grad():
        twin.d_arena.flat.copy_(m.d_arena.flat)
        twin.g_arena.flat.copy_(m.g_arena.flat)
    K.filter_cache_invalidate()
    return twin


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if 'cuda' in str(getattr(e, 'device_type', '')).lower()]


def test_false_is_the_model_built_without_the_argument(tmp_path):
    PG = need_gpu()
    feed = _feeds(PG, 1)[0]
    base = _seed_checkpoint(tmp_path)
    ends = []
    for i, kw in enumerate(({}, {'critic_sn': False})):
        m = _model(trans=True, **kw)
        assert m.critic_spectral is None and m.D_optimizer.spectral is None
        m.iteration(1, feed)
        torch.cuda.synchronize()
        arenas = (m.d_arena.flat.clone(), m.g_arena.flat.clone())
        del m
        t, logs, z = _train(tmp_path, 'plain%d' % i, base, 3, **kw)
        assert not any('spectral' in line for line in logs) and not any('spectral' in k for k in z.files)
        ends.append((arenas, sorted(z.files), (t.d_arena.flat.clone(), t.g_arena.flat.clone())))
    (a0, k0, t0), (a1, k1, t1) = ends
    assert k0 == k1 and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a0 + t0, a1 + t1))


def test_the_gradients_are_those_of_the_critic_with_the_normalised_weights():
    PG = need_gpu()
    feed = _feeds(PG, 1)[0]
    m = _model(critic_sn=True)
    sn = m.critic_spectral
    assert sn is not None and m.D_optimizer.spectral is sn and m.G_optimizer.spectral is None
    assert sn.names == m.kernel_names(m.d_vars) and 0 < len(sn.names) < len(m.d_vars)
    plain = _model()
    assert not torch.equal(plain.d_arena.flat, m.d_arena.flat) and torch.equal(_bits(plain.d_arena.flat), _bits(sn.raw))    # the same draw, normalised
    sig = sn.sigma.cpu().numpy()
    assert np.all(np.isfinite(sig)) and np.all(sig > 0)
    for n in sn.names:                                            # 15 warm-up iterations: the estimate is the top singular value's
        o, k = m.d_arena.offsets[n]
        R, C = SC.matrix_shape(tuple(m.d_vars[n].shape))
        W = m.d_arena.flat[o:o + k].double().cpu().numpy().reshape(R, C)
        top = float(np.linalg.svd(W, compute_uv=False)[0])
        assert 1.0 - FWD <= top < float('inf'), (n, top)         # W = raw / sigma and sigma <= sigma_top: no singular value of W below 1 - rounding
    twin = _twin_with_the_weights_of(m)
    outs = []
    for model in (m, twin):
        _use(model)
        model.set_alpha(0.3)
        d = model.d_losses(feed)
        torch.cuda.synchronize()
        outs.append((d['D_loss'].clone(), model.d_arena.grad.clone()))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1])) and bool(outs[0][1].abs().max() > 0)


def test_one_critic_step_follows_the_restatement():
    PG = need_gpu()
    feed = _feeds(PG, 1)[0]
    m = _model(critic_sn=True, adam_lr=LR)
    sn, arena = m.critic_spectral, m.d_arena
    m.set_alpha(0.3)
    s0 = _spectral(m)
    m.d_losses(feed)
    torch.cuda.synchronize()
    G = arena.grad.clone()                                        # dL/dW, before the optimizer turns it into dL/draw
    m.D_optimizer.prepare(LR)
    m._d_body(feed)
    s1 = _spectral(m)
    gt = arena.grad.clone()
    worst = dict(grad=0.0, raw=0.0, u=0.0, sigma=0.0, var=0.0)
    f = lambda t: t.double().cpu().numpy()       # noqa: E731
    for n in arena.names:
        o, k = arena.offsets[n]
        if n not in sn.index:                                     # biases, gamma / beta: the plain step, and the variable is raw
            assert torch.equal(_bits(gt[o:o + k]), _bits(G[o:o + k])) and torch.equal(_bits(s1['flat'][o:o + k]), _bits(s1['raw'][o:o + k])), n
            ref, _, _ = SC.adam_tf(f(s0['raw'][o:o + k]), f(gt[o:o + k]), np.zeros(k), 1, LR)
            assert SC.relerr(f(s1['raw'][o:o + k]), ref) <= FWD, n
            continue
        i = sn.index[n]
        _, R, C, uo, vo = (int(x) for x in sn.table.host[i][:5])
        u0, v0, sg0 = f(s0['u'][uo:uo + C]), f(s0['v'][vo:vo + R]), float(s0['sigma'][i])
        ref_g = SC.grad_raw(f(G[o:o + k]).reshape(R, C), f(s0['flat'][o:o + k]).reshape(R, C), u0, v0, sg0)
        e = dict(grad=SC.relerr(f(gt[o:o + k]).reshape(R, C), ref_g))
        ref_raw, _, _ = SC.adam_tf(f(s0['raw'][o:o + k]), f(gt[o:o + k]), np.zeros(k), 1, LR)
        e['raw'] = SC.relerr(f(s1['raw'][o:o + k]), ref_raw)
        raw1 = f(s1['raw'][o:o + k]).reshape(R, C)
        ur, vr, sr = SC.iterate(raw1, u0, 1)
        e['u'], e['sigma'] = SC.relerr(f(s1['u'][uo:uo + C]), ur), abs(float(s1['sigma'][i]) - sr) / sr
        e['var'] = SC.relerr(f(m.d_vars[n].detach()).reshape(R, C), SC.normalised(raw1, sr))
        print('%s [%d, %d]: gradient %.2e  raw %.2e  u %.2e  sigma %.2e  variable %.2e' % (n, R, C, e['grad'], e['raw'], e['u'], e['sigma'], e['var']))
        for key in e:
            worst[key] = max(worst[key], e[key])
        assert e['grad'] <= GRAD and max(e['raw'], e['u'], e['sigma'], e['var']) <= FWD, (n, e)
    assert not torch.equal(s1['raw'], s0['raw']) and not torch.equal(s1['u'], s0['u'])
    print('one critic step: maxima gradient %.2e  raw %.2e  u %.2e  sigma %.2e  variable %.2e' % (
        worst['grad'], worst['raw'], worst['u'], worst['sigma'], worst['var']))


def test_graph_replay_matches_eager():
    PG = need_gpu()
    feeds = _feeds(PG, 3)
    ends = []
    for use_graphs in (False, True):
        m = _model(trans=True, critic_sn=True, adam_lr=LR)
        m.iteration(1, feeds[0])
        if use_graphs:
            m.enable_graphs(feeds[0])
        outs = [m.iteration(2 + 2 * i, feeds[1 + i]) for i in range(2)]
        s = _spectral(m)
        ends.append((s, m.g_arena.flat.detach().clone(), float(outs[-1]['d']['D_loss']), float(outs[-1]['g']['G_loss'])))
    (s0, g0, dl0, gl0), (s1, g1, dl1, gl1) = ends
    assert all(torch.equal(_bits(s0[k]), _bits(s1[k])) for k in s0) and torch.equal(_bits(g0), _bits(g1)) and dl0 == dl1 and gl0 == gl1
    assert bool(torch.isfinite(s0['flat']).all()) and bool((s0['sigma'] > 0).all())


def _dataset(size):
    from t2i_amd.data import SyntheticTextDataset
    from t2i_amd.utils.config import AttrDict
    dcfg = AttrDict({'MODEL': {'Z_DIM': WIDTHS['z_dim'], 'OUTPUT_SIZE': size, 'EMBED_DIM': WIDTHS['embed_dim'], 'IMAGE_SHAPE': {'W': size, 'H': size, 'D': 3}},
                     'TRAIN': {'BATCH_SIZE': BATCH}})
    return SyntheticTextDataset(dcfg, torch.device('cuda'), seed=5, num_examples=512)


def _seed_checkpoint(tmp_path):
    """A stage-2 checkpoint of a model WITHOUT the flag, for the stabilisation stage's restore to start from."""
    from t2i_amd.utils.saver import Saver, save
    d = str(tmp_path / 'base') + '/'
    if not os.path.exists(d):
        m = _model(seed=21)
        save(Saver(m.store, var_list=m.get_variables_up_to_stage(STAGE)), None, d, 1)
    return d


def _train(tmp_path, tag, read_dir, max_steps, **kw):
    wdir, sdir = str(tmp_path / tag / 'ckpt') + '/', str(tmp_path / tag / 'samples') + '/'
    for d in (wdir, sdir):
        os.makedirs(d, exist_ok=True)
    logs = []
    torch.manual_seed(77)
    m = _model(dirs=(wdir, read_dir), dataset=_dataset(8), sample=sdir, **kw)
    m.train(max_steps=max_steps, log=logs.append, side_effects=True)
    torch.cuda.synchronize()
    path = os.path.join(wdir, 'model-%d.npz' % (max_steps - 1))
    return m, logs, (np.load(path) if os.path.exists(path) else None)


def test_a_checkpoint_carries_the_state_and_one_without_it_is_synced(tmp_path):
    need_gpu()
    base = _seed_checkpoint(tmp_path)
    # restoring a checkpoint written without the flag: every kernel starts from the weights the file holds
    m0, logs0, none = _train(tmp_path, 'fresh', base, 1, critic_sn=True)
    sn0 = m0.critic_spectral
    assert none is None and m0.spectral_synced == len(sn0.names) and sum('spectral normalisation' in line for line in logs0) == 1
    assert '0 of %d kernels restored with their state, %d synced' % (len(sn0.names), len(sn0.names)) in ''.join(logs0)
    sig = sn0.sigma.cpu().numpy()
    assert np.all(np.isfinite(sig)) and np.all(sig > 0)
    z0 = np.load(os.path.join(base, 'model-1.npz'))
    for n in m0.d_arena.names:
        o, k = m0.d_arena.offsets[n]
        assert np.array_equal(sn0.raw[o:o + k].cpu().numpy(), z0[n].reshape(-1)), n                      # raw <- the file's weights
        want = z0[n].reshape(-1).astype(np.float64) / (float(sig[sn0.index[n]]) if n in sn0.index else 1.0)
        assert SC.relerr(m0.d_vars[n].detach().double().cpu().numpy().reshape(-1), want) <= FWD, n
    # two iterations, a checkpoint, and a fresh model restored from it
    m1, logs1, z = _train(tmp_path, 'first', base, 3, critic_sn=True, adam_lr=LR)
    sn1 = m1.critic_spectral
    want = _spectral(m1)
    keys = [k for n in sn1.names for k in sn1.keys(n)]
    assert all(k in z.files for k in keys) and sum('/spectral_' in k for k in z.files) == len(keys) == 4 * len(sn1.names)
    for n in sn1.names:                                           # the variable is saved as the normalised weights, raw next to it
        assert np.array_equal(z[n], m1.d_vars[n].detach().cpu().numpy()) and not np.array_equal(z[n], z[n + '/spectral_raw'])
        assert z[n + '/spectral_raw'].shape == z[n].shape and z[n + '/spectral_sigma'].shape == (1,)
    m2, logs2, _ = _train(tmp_path, 'second', str(tmp_path / 'first' / 'ckpt') + '/', 1, critic_sn=True, adam_lr=LR, seed=99)
    assert m2.spectral_synced == 0 and '%d of %d kernels restored with their state, 0 synced' % (len(sn1.names), len(sn1.names)) in ''.join(logs2)
    got = _spectral(m2)
    assert all(torch.equal(_bits(got[k]), _bits(want[k])) for k in want)
    assert torch.equal(_bits(m2.g_arena.flat), _bits(m1.g_arena.flat))
    # a reader without the flag sees a working critic: the normalised weights
    m3, logs3, _ = _train(tmp_path, 'reader', str(tmp_path / 'first' / 'ckpt') + '/', 1, seed=98)
    assert torch.equal(_bits(m3.d_arena.flat), _bits(m1.d_arena.flat)) and not any('spectral' in line for line in logs3)


def test_the_generator_step_does_not_see_the_flag():
    PG = need_gpu()
    feed = _feeds(PG, 1)[0]
    m = _model(critic_sn=True, adam_lr=LR)
    twin = _twin_with_the_weights_of(m, adam_lr=LR)
    ends = []
    for model in (m, twin):
        _use(model)
        model.set_alpha(0.3)
        model.G_optimizer.prepare(LR)
        model._g_body(feed)                                       # (the first call loads code objects: not the one that is listed)
        model.G_optimizer.prepare(LR)
        names = sorted(_kernels(lambda: model._g_body(feed)))     # (sorted: the filter gradients run on a side stream)
        ends.append((names, model.g_arena.flat.clone(), model.g_arena.grad.clone(), model.d_arena.flat.clone()))
    (k0, w0, g0, d0), (k1, w1, g1, d1) = ends
    assert k0 == k1 and len(k0) > 0 and not any('sn_' in k for k in k0)
    assert torch.equal(_bits(w0), _bits(w1)) and torch.equal(_bits(g0), _bits(g1)) and torch.equal(_bits(d0), _bits(d1))
