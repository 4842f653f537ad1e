"""PGGAN(diffaug=...): None is today's model bit for bit; with a policy every image the critic sees goes through the differentiable
augmentation T and one critic step — both gradient penalties as gradients of D o T, i.e. the adjoint kernel and
its backward — and one generator step agree with the float64 oracle, whose `discriminator` is wrapped from here: it applies the float64
restatement of T (tests/diffaug_cases.py) to the image, with the block of the parameter table chosen by call order (the oracle calls D on
G, x, x_mismatch, x_hat).  Tiny widths and criteria of tests/test_pggan_mbstd_gpu.py: forward tensors 1e-4, loss scalars 1e-4 relative,
gradients max-norm 2e-3 per tensor.

Conditioning: feed seed, table seed and critic filter scale of every case were picked on the CPU so that the float64 run has both hinged
penalties above 0.1 (asserted): the second-order path carries gradient."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import diffaug_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = dict(z_dim=8, embed_dim=32, compressed=16, batch=4, base=32, cap=16)           # tests/test_pggan_mbstd_gpu.py's
STEPS, IDX, BATCH = 10, 3, 4
POLICY = DC.ALL
# (stage, trans, critic_mbstd) -> (feed seed of oracle.torch_pggan.synthetic_feed, critic filter scale); the table seed is TABLE_SEED
CASES = {(2, False, None): (3, 1.6), (2, True, None): (3, 1.6), (3, False, None): (3, 1.6), (2, False, 4): (3, 1.6)}
TABLE_SEED = 5


def relerr(got, ref, floor=1e-30):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), floor))


def _model(stage, trans, batch=BATCH, **kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    return PGGAN(batch, STEPS, None, None, None, None, None, stage, trans, device=torch.device('cuda'), fmap_base=TINY['base'],
                 fmap_max=TINY['cap'], z_dim=TINY['z_dim'], embed_dim=TINY['embed_dim'], compr_embed_dim=TINY['compressed'], **kw)


def _gpu_feed(feed, aug_d=None, aug_g=None):
    f = {k: v.float().cuda() for k, v in feed.items()}
    out = {'x': f['x'], 'x_mismatch': f['x_mismatch'], 'cond': f['cond'], 'z': f['z'], 'eps_graph': f['eps'], 'ca_noise_d': f['ca_noise_d'],
           'ca_noise_g': f['ca_noise_g']}
    if aug_d is not None:
        out['aug_d'] = aug_d.float().cuda()
    if aug_g is not None:
        out['aug_g'] = aug_g.float().cuda()
    return out


def oracle_inputs(PG, stage, trans, seed, scale, batch=BATCH):
    """Parameters and feed as tests/test_pggan_mbstd_gpu.py prepares them (critic filters scaled so that the hinged penalties are
    active, non-trivial biases), rounded to fp32; and the two parameter tables.  Must run BEFORE the oracle's discriminator is wrapped
    (init_variables calls it)."""
    cfg = PG.Cfg(**dict(TINY, batch=batch))
    P = PG.init_variables(cfg, stage, trans, seed=0)
    rng = np.random.default_rng(31)
    for n in P:
        if n.startswith('d_net') and (n.endswith('weights') or n.endswith('kernel')):
            P[n] = P[n] * scale
        if n.endswith('biases') or n.endswith('bias') or n.endswith('beta'):
            P[n] = torch.tensor(rng.standard_normal(tuple(P[n].shape)) * 0.1)
        if n.endswith('gamma'):
            P[n] = torch.tensor(1.0 + rng.standard_normal(tuple(P[n].shape)) * 0.1)
    feed = PG.synthetic_feed(cfg, stage, seed=seed)
    P = {n: v.float().double() for n, v in P.items()}
    feed = {n: v.float().double() for n, v in feed.items()}
    size = 4 * 2 ** (stage - 1)
    aug_d = DC.drawn_table(4 * batch, size, size, TABLE_SEED).float().double()
    aug_g = DC.drawn_table(batch, size, size, TABLE_SEED + 1).float().double()
    return cfg, P, feed, aug_d, aug_g


def wrap_discriminator(inner, tables):
    """The oracle's critic behind T: call k transforms its image with tables[k]"""
    calls = []

    def discriminator(V, cfg, img_nhwc, cond, stages, t, alpha):
        k = len(calls)
        calls.append(k)
        return inner(V, cfg, DC.ref_T(img_nhwc, tables[k], POLICY), cond, stages, t, alpha)
    return discriminator, calls


def inner_discriminator(PG, mbstd):
    if mbstd is None:
        return PG.discriminator
    import test_pggan_mbstd_gpu as MB
    return MB._mbstd_discriminator(PG, mbstd)


def oracle_d_step(PG, monkeypatch, stage, trans, mbstd):
    inner = inner_discriminator(PG, mbstd)
    monkeypatch.setattr(PG, 'discriminator', inner)                          # (the layer changes a variable's shape: init_variables must see it)
    cfg, P, feed, aug_d, aug_g = oracle_inputs(PG, stage, trans, *CASES[(stage, trans, mbstd)])
    if mbstd is not None:
        import test_pggan_mbstd_gpu as MB
        del MB.SIGMAS[:]                                                     # (init_variables ran the critic on zeros)
    disc, calls = wrap_discriminator(inner, [aug_d[k * BATCH:(k + 1) * BATCH] for k in range(4)])
    monkeypatch.setattr(PG, 'discriminator', disc)
    ref = PG.d_step(P, cfg, feed, stage, trans, IDX / float(STEPS))
    assert len(calls) == 4                                                   # D(G), D(x), D(x_mismatch), D(x_hat)
    if mbstd is not None:       # the layer's double backward carries 1 / sigma^3: the floor of tests/test_pggan_mbstd_gpu.py holds behind T too
        assert len(MB.SIGMAS) == 4 and min(MB.SIGMAS) >= MB.SIGMA_FLOOR, MB.SIGMAS
    return cfg, P, feed, aug_d, aug_g, ref


def _check_grads(arena, names, ref_grads, tol=2e-3):
    worst = 0.0
    for n in names:
        r = ref_grads[n].numpy()
        if np.abs(r).max() < 1e-9:
            assert float(arena.grad_of(n).abs().max()) <= 1e-4, n
        else:
            e = relerr(arena.grad_of(n), r)
            worst = max(worst, e)
            assert e <= tol, (n, e)
    return worst


def test_diffaug_none_is_the_model_built_without_the_argument():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    feed = _gpu_feed(PG.synthetic_feed(PG.Cfg(**TINY), 2, seed=1))
    outs = []
    for kw in ({}, {'diffaug': None}):
        m = _model(2, True, **kw)
        m.set_alpha(0.3)
        d = m.d_losses(feed)
        g = m.g_losses(feed)
        torch.cuda.synchronize()
        outs.append((list(m.store.vars), {k: d[k].clone() for k in ('D_loss', 'wdist', 'wdist2', 'real_gp', 'real_gp2')}, m.d_arena.grad.clone(),
                     g['G_loss'].clone(), m.g_arena.grad.clone()))
    (n0, d0, g0, l0, gg0), (n1, d1, g1, l1, gg1) = outs
    assert n0 == n1 and torch.equal(g0, g1) and bool(g0.abs().max() > 0)
    assert torch.equal(l0, l1) and torch.equal(gg0, gg1) and bool(gg0.abs().max() > 0)
    for k in d0:
        assert torch.equal(d0[k], d1[k]), k


@pytest.mark.parametrize('stage,trans,mbstd', sorted(CASES, key=str), ids=lambda v: str(v))
def test_critic_step_through_the_augmentation_matches_the_oracle(monkeypatch, stage, trans, mbstd):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    cfg, P, feed, aug_d, aug_g, ref = oracle_d_step(PG, monkeypatch, stage, trans, mbstd)
    assert ref['real_gp'] > 0.1 and ref['real_gp2'] > 0.1                    # both hinges are active
    m = _model(stage, trans, diffaug=POLICY, **({} if mbstd is None else {'critic_mbstd': mbstd}))
    assert [(n, tuple(v.shape)) for n, v in m.store.vars.items()] == [(n, tuple(v.shape)) for n, v in P.items()]
    m.store.load({n: v.numpy() for n, v in P.items()})
    m.set_alpha(IDX / float(STEPS))
    d = m.d_losses(_gpu_feed(feed, aug_d, aug_g))
    torch.cuda.synchronize()
    eg, eh = relerr(d['G'], ref['G']), relerr(d['Dx_hat_logit'], ref['Dx_hat'])
    tag = 'stage %d %s mbstd %s' % (stage, 'transition' if trans else 'stable', mbstd)
    print('%s: G %.2e  Dx_hat %.2e' % (tag, eg, eh))
    assert eg <= 1e-4 and eh <= 1e-4
    for k in ('D_loss', 'wdist', 'wdist2', 'real_gp', 'real_gp2'):
        print('%s %s: %.9g (oracle %.9g)' % (tag, k, float(d[k]), ref[k]))
        assert abs(float(d[k]) - ref[k]) <= 1e-4 * max(abs(ref[k]), 1.0), (k, float(d[k]), ref[k])
    worst = _check_grads(m.d_arena, m.d_vars, ref['grads'])
    print('%s: worst gradient error %.2e of its tensor scale' % (tag, worst))


def test_generator_step_through_the_augmentation_matches_the_oracle(monkeypatch):
    """g_losses: the adjoint kernel carries the frozen critic's input gradient to every generator variable; the returned G is the
    image before T"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    stage, trans = 2, True
    cfg, P, feed, aug_d, aug_g = oracle_inputs(PG, stage, trans, *CASES[(stage, trans, None)])
    disc, calls = wrap_discriminator(PG.discriminator, [aug_g])
    monkeypatch.setattr(PG, 'discriminator', disc)
    ref = PG.g_step(P, cfg, feed, stage, trans, IDX / float(STEPS))
    assert len(calls) == 1
    m = _model(stage, trans, diffaug=POLICY)
    m.store.load({n: v.numpy() for n, v in P.items()})
    m.set_alpha(IDX / float(STEPS))
    g = m.g_losses(_gpu_feed(feed, aug_d, aug_g))
    torch.cuda.synchronize()
    assert relerr(g['G'], ref['G']) <= 1e-4
    for k in ('G_loss', 'G_kl_loss'):
        assert abs(float(g[k]) - ref[k]) <= 1e-4 * max(abs(ref[k]), 1.0), (k, float(g[k]), ref[k])
    assert all(float(ref['grads'][n].abs().max()) > 0 for n in m.g_vars)    # the oracle's gradient reaches every generator variable
    worst = _check_grads(m.g_arena, m.g_vars, ref['grads'])
    assert all(float(m.g_arena.grad_of(n).abs().max()) > 0 for n in m.g_vars)
    print('g_step through the augmentation: worst gradient error %.2e of its tensor scale' % worst)


def _feeds(PG, stage, batch, with_tables):
    cfg = PG.Cfg(**dict(TINY, batch=batch))
    size = 4 * 2 ** (stage - 1)
    feeds = []
    for s in (1, 2, 3):
        tables = (DC.drawn_table(4 * batch, size, size, 10 + s), DC.drawn_table(batch, size, size, 20 + s)) if with_tables else (None, None)
        feeds.append(_gpu_feed(PG.synthetic_feed(cfg, stage, seed=s), *tables))
    return feeds


def test_graph_replay_matches_eager_with_fed_tables():
    """Two models with the same variables and feeds (fixed eps, conditioning noise and tables), one eager and one replaying hipGraphs:
    after two iterations the parameter arenas are equal bit for bit — the kernels capture and replay"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    feeds = _feeds(PG, 2, 8, True)
    states = []
    for use_graphs in (False, True):
        m = _model(2, True, batch=8, diffaug=POLICY, seed=5)
        m.iteration(1, feeds[0])
        if use_graphs:
            m.enable_graphs(feeds[0])
        outs = [m.iteration(2 + 2 * i, feeds[1 + i]) for i in range(2)]
        torch.cuda.synchronize()
        states.append((m.d_arena.flat.detach().clone(), m.g_arena.flat.detach().clone(), float(outs[-1]['d']['D_loss']), float(outs[-1]['g']['G_loss'])))
    (d0, g0, dl0, gl0), (d1, g1, dl1, gl1) = states
    assert torch.equal(d0, d1) and torch.equal(g0, g1) and dl0 == dl1 and gl0 == gl1
    assert bool(torch.isfinite(d0).all()) and bool(d0.abs().max() > 0)


def test_tables_that_are_not_fed_are_redrawn_outside_the_graphs():
    """Without fed tables the static buffers are re-drawn before every replay (they differ from one iteration to the next), the
    losses stay finite, and a replay of the captured graphs on its own leaves both tables as they are"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    feeds = _feeds(PG, 2, 8, False)
    m = _model(2, True, batch=8, diffaug=POLICY, seed=5)
    out = m.iteration(1, feeds[0])                                            # eager, tables drawn inside the step
    assert np.isfinite(float(out['d']['D_loss'])) and np.isfinite(float(out['g']['G_loss']))
    m.enable_graphs(feeds[0])
    st = m._graphs.static
    assert tuple(st['aug_d'].shape) == (32, 9) and tuple(st['aug_g'].shape) == (8, 9)
    seen = []
    for i in range(2):
        out = m.iteration(2 + i, feeds[1 + i])
        torch.cuda.synchronize()
        assert np.isfinite(float(out['d']['D_loss'])) and np.isfinite(float(out['g']['G_loss']))
        seen.append((st['aug_d'].clone(), st['aug_g'].clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])
    m._graphs.replay('d')
    m._graphs.replay('g')
    torch.cuda.synchronize()
    assert torch.equal(st['aug_d'], seen[1][0]) and torch.equal(st['aug_g'], seen[1][1])
    P = st['aug_d'].cpu()
    assert torch.equal(P[:, 3:], P[:, 3:].round()) and bool((P[:, 6] > P[:, 5]).all()) and bool((P[:, 1] >= 0).all())
