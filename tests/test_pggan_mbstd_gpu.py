"""PGGAN(critic_mbstd=G): None is today's critic bit for bit; with a group size the minibatch standard deviation sits in front of the critic's
last block and one critic step — both gradient penalties, i.e. the layer's double backward, and the 3B pass whose
groups must not straddle its parts — agrees with the float64 oracle's d_step, whose `discriminator` is replaced from here by a
restatement with the layer built on oracle/torch_pggan.py's own blocks.  Tiny widths of tests/test_pggan_critic_norm_gpu.py, stage 2,
stable and in transition; its criteria: forward tensors 1e-4, loss scalars 1e-4 relative, gradients max-norm 2e-3 per tensor — and in
addition the statistic channels' slice of the first 3x3 filter's gradient at 2e-3 of ITS OWN maximum (it is a few per cent of the tensor's
and a wrong statistic could hide under the whole-tensor bound).

Conditioning: the double backward carries 1 / sigma^3; every oracle run asserts that no column's sigma in any of its critic passes is below
5e-3 (the feed's seed is chosen so that groups of 4 clear it; each case prints its smallest sigma; groups of 2 or 3 fall below the floor
and are not used here)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TINY = dict(z_dim=8, embed_dim=32, compressed=16, batch=4, base=32, cap=16)           # tests/test_pggan_critic_norm_gpu.py's, batch aside
STAGE, STEPS, IDX = 2, 10, 3
SIGMA_FLOOR = 5e-3
FEED_SEED = 3                     # of oracle.torch_pggan.synthetic_feed, chosen so that every case clears the floors asserted below with room
SIGMAS = []                       # the smallest sigma of every critic pass of the patched oracle, in call order


def relerr(got, ref, floor=1e-30):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), floor))


def _model(trans, batch, **kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    return PGGAN(batch, STEPS, None, None, None, None, None, STAGE, trans, device=torch.device('cuda'), fmap_base=TINY['base'],
                 fmap_max=TINY['cap'], z_dim=TINY['z_dim'], embed_dim=TINY['embed_dim'], compr_embed_dim=TINY['compressed'], **kw)


def _gpu_feed(feed):
    f = {k: v.float().cuda() for k, v in feed.items()}
    return {'x': f['x'], 'x_mismatch': f['x_mismatch'], 'cond': f['cond'], 'z': f['z'], 'eps_graph': f['eps'], 'ca_noise_d': f['ca_noise_d'],
            'ca_noise_g': f['ca_noise_g']}


def _mbstd_nchw(x, group, eps=1e-8):
    """x [B,C,H,W] -> stat [B,F]: groups of contiguous rows, the largest divisor of B not above `group` (the oracle's init_variables
    calls the critic with 2 rows); F = 4 for a multiple of 16 channels, else 1"""
    B, C, H, W = x.shape
    G = max(g for g in range(1, group + 1) if B % g == 0)
    Fs = 4 if C % 16 == 0 else 1
    xg = x.reshape(B // G, G, C, H, W)
    d = xg - xg.mean(1, keepdim=True)
    sigma = torch.sqrt((d ** 2).mean(1) + eps)
    SIGMAS.append(float(sigma.detach().min()))
    return sigma.reshape(B // G, Fs, C // Fs, H, W).mean((2, 3, 4)).repeat_interleave(G, 0)


def _mbstd_discriminator(PG, group, norm=None):
    """oracle.torch_pggan.discriminator with [features | tiled compressed cond | tiled stat] in front of the last block (activations NCHW,
    as in the oracle) and, for norm='pixel', every 3x3 / 4x4 convolution followed by the pixel norm with the lrelu inside"""
    def block(V, x, f, k, pad):
        x = PG._lrelu(V.conv(x, f, k, 1, pad, 'he'))
        return x if norm is None else x / torch.sqrt((x ** 2).mean(1, keepdim=True) + 1e-8)

    def discriminator(V, cfg, img_nhwc, cond, stages, t, alpha):
        inp = img_nhwc.permute(0, 3, 1, 2)
        x_iden = None
        if t:
            x_iden = PG._from_rgb(V, 'd_net', F.avg_pool2d(inp, 2), stages - 2, cfg)
        x = PG._from_rgb(V, 'd_net', inp, stages - 1, cfg)
        for i in range(stages - 1, 0, -1):
            V.enter('d_net/conv_stage_%d' % i)
            x = block(V, x, cfg.dnf(i), 3, 'SAME')
            x = block(V, x, cfg.dnf(i - 1), 3, 'SAME')
            x = F.avg_pool2d(x, 2)
            if i == stages - 1 and t:
                x = alpha * x + (1.0 - alpha) * x_iden
        V.enter('d_net/conv_stage_0')
        e = PG._lrelu(V.dense(cond, cfg.compressed, 'he'))
        s = _mbstd_nchw(x, group)
        x = torch.cat([x, e[:, :, None, None].expand(-1, -1, 4, 4), s[:, :, None, None].expand(-1, -1, 4, 4)], 1)
        x = block(V, x, cfg.dnf(0), 3, 'SAME')
        x = block(V, x, cfg.dnf(0), 4, 'VALID')
        return V.dense(x.reshape(x.shape[0], -1), 1, 'he').reshape(-1)
    return discriminator


def _oracle_inputs(PG, trans, batch, norm=None):
    """Parameters and feed as tests/test_pggan_critic_norm_gpu.py's _oracle_step prepares them (critic filters x 1.6 so that the hinged
    penalties are active — under the pixel norm the final dense layer x 4, as there —, non-trivial biases), rounded to fp32"""
    cfg = PG.Cfg(**dict(TINY, batch=batch))
    P = PG.init_variables(cfg, STAGE, trans, seed=0)
    rng = np.random.default_rng(31)
    for n in P:
        if n.startswith('d_net') and (n.endswith('weights') or n.endswith('kernel')):
            P[n] = P[n] * (4.0 if norm is not None and n.endswith('dense_1/kernel') else 1.6)
        if n.endswith('biases') or n.endswith('bias') or n.endswith('beta'):
            P[n] = torch.tensor(rng.standard_normal(tuple(P[n].shape)) * 0.1)
        if n.endswith('gamma'):
            P[n] = torch.tensor(1.0 + rng.standard_normal(tuple(P[n].shape)) * 0.1)
    feed = PG.synthetic_feed(cfg, STAGE, seed=FEED_SEED)
    P = {n: v.float().double() for n, v in P.items()}
    feed = {n: v.float().double() for n, v in feed.items()}
    del SIGMAS[:]                                       # (init_variables ran the critic on zeros)
    return cfg, P, feed


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


def _critic_step_against_the_oracle(monkeypatch, trans, batch, group, norm):
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    monkeypatch.setattr(PG, 'discriminator', _mbstd_discriminator(PG, group, norm))
    cfg, P, feed = _oracle_inputs(PG, trans, batch, norm)
    ref = PG.d_step(P, cfg, feed, STAGE, trans, IDX / float(STEPS))
    assert len(SIGMAS) == 4 and min(SIGMAS) >= SIGMA_FLOOR, SIGMAS            # D(G), D(x), D(x_mismatch), D(x_hat)
    assert ref['real_gp'] > 0.1 and ref['real_gp2'] > 0.1                        # both hinges are active: the second-order path carries gradient
    kw = {} if norm is None else {'critic_norm': norm}
    m = _model(trans, batch, critic_mbstd=group, **kw)
    assert m.mbstd_group == group
    assert [(n, tuple(v.shape)) for n, v in m.store.vars.items()] == [(n, tuple(v.shape)) for n, v in P.items()]
    m.store.load({n: v.numpy() for n, v in P.items()})
    m.set_alpha(IDX / float(STEPS))
    d = m.d_losses(_gpu_feed(feed))
    torch.cuda.synchronize()
    eg, eh = relerr(d['G'], ref['G']), relerr(d['Dx_hat_logit'], ref['Dx_hat'])
    tag = 'batch %d G %d %s %s' % (batch, group, 'transition' if trans else 'stable', norm)
    print('%s: min sigma %.3g  G %.2e  Dx_hat %.2e' % (tag, min(SIGMAS), eg, eh))
    assert eg <= 1e-4 and eh <= 1e-4
    for k in ('D_loss', 'wdist', 'wdist2', 'real_gp', 'real_gp2'):
        print('%s %s: %.9g (oracle %.9g)' % (tag, k, float(d[k]), ref[k]))
        assert abs(float(d[k]) - ref[k]) <= 1e-4 * max(abs(ref[k]), 1.0), (k, float(d[k]), ref[k])
    worst = _check_grads(m.d_arena, m.d_vars, ref['grads'])
    # the statistic's own channels: the last F input channels of the block's first filter (HWIO)
    name, Fs = 'd_net/conv_stage_0/Conv/weights', 4
    r = ref['grads'][name].numpy()
    assert r.shape[2] == cfg.dnf(0) + cfg.compressed + Fs
    got = m.d_arena.grad_of(name).detach().double().cpu().numpy().reshape(r.shape)
    share = np.abs(r[:, :, -Fs:]).max() / np.abs(r).max()
    es = relerr(got[:, :, -Fs:], r[:, :, -Fs:])
    print('%s: worst gradient error %.2e of its tensor scale; stat channels %.2e of their own scale (%.2g of the tensor maximum)' % (
        tag, worst, es, share))
    assert np.abs(r[:, :, -Fs:]).max() > 0 and es <= 2e-3, es


def test_critic_mbstd_none_is_the_critic_built_without_the_argument():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    feed = _gpu_feed(PG.synthetic_feed(PG.Cfg(**TINY), STAGE, seed=1))
    outs = []
    for kw in ({}, {'critic_mbstd': None}):
        m = _model(True, TINY['batch'], **kw)
        m.set_alpha(0.3)
        d = m.d_losses(feed)
        torch.cuda.synchronize()
        outs.append((list(m.store.vars), {k: d[k].clone() for k in ('D_loss', 'wdist', 'wdist2', 'real_gp', 'real_gp2')}, m.d_arena.grad.clone()))
    (n0, d0, g0), (n1, d1, g1) = outs
    assert n0 == n1 and torch.equal(g0, g1) and bool(g0.abs().max() > 0)
    for k in d0:
        assert torch.equal(d0[k], d1[k]), k


@pytest.mark.parametrize('trans', [False, True])
@pytest.mark.parametrize('batch', [4, 8])
def test_critic_step_with_the_layer_matches_the_oracle(monkeypatch, batch, trans):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _critic_step_against_the_oracle(monkeypatch, trans, batch, 4, None)


def test_the_layer_composes_with_a_pixel_normalised_critic(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _critic_step_against_the_oracle(monkeypatch, False, 4, 4, 'pixel')


def test_generator_step_through_the_layer_matches_the_oracle(monkeypatch):
    """g_losses: the first-order path through the layer (the critic is frozen, its input gradient reaches every generator variable)"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    monkeypatch.setattr(PG, 'discriminator', _mbstd_discriminator(PG, 4))
    cfg, P, feed = _oracle_inputs(PG, True, 4)
    ref = PG.g_step(P, cfg, feed, STAGE, True, IDX / float(STEPS))
    assert len(SIGMAS) == 1 and SIGMAS[0] >= SIGMA_FLOOR, SIGMAS
    m = _model(True, 4, critic_mbstd=4)
    m.store.load({n: v.numpy() for n, v in P.items()})
    m.set_alpha(IDX / float(STEPS))
    g = m.g_losses(_gpu_feed(feed))
    torch.cuda.synchronize()
    assert relerr(g['G'], ref['G']) <= 1e-4
    for k in ('G_loss', 'G_kl_loss'):
        assert abs(float(g[k]) - ref[k]) <= 1e-4 * max(abs(ref[k]), 1.0), (k, float(g[k]), ref[k])
    worst = _check_grads(m.g_arena, m.g_vars, ref['grads'])
    print('g_step through the layer: worst gradient error %.2e of its tensor scale' % worst)


def test_graph_replay_matches_eager_with_the_layer():
    """Two models with the same variables and feeds (fixed eps / conditioning noise), one eager and one replaying hipGraphs: after two
    iterations the parameter arenas are equal bit for bit — the layer's kernels capture and replay"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    cfg = PG.Cfg(**dict(TINY, batch=8))
    feeds = [_gpu_feed(PG.synthetic_feed(cfg, STAGE, seed=s)) for s in (1, 2, 3)]
    states = []
    for use_graphs in (False, True):
        m = _model(True, 8, critic_mbstd=4, seed=5)
        m.iteration(1, feeds[0])
        if use_graphs:
            m.enable_graphs(feeds[0])
        outs = [m.iteration(2 + 2 * i, feeds[1 + i]) for i in range(2)]
        torch.cuda.synchronize()
        states.append((m.d_arena.flat.detach().clone(), m.g_arena.flat.detach().clone(), float(outs[-1]['d']['D_loss']), float(outs[-1]['g']['G_loss'])))
    (d0, g0, dl0, gl0), (d1, g1, dl1, gl1) = states
    assert torch.equal(d0, d1) and torch.equal(g0, g1) and dl0 == dl1 and gl0 == gl1
    assert bool(torch.isfinite(d0).all()) and bool(d0.abs().max() > 0)
