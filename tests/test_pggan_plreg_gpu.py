"""PGGAN(style_dim=16, modulated_conv=True, pl_weight=2) on the GPU: one due generator step against a float64
restatement of the path-length regulariser on top of tests/modconv_cases.py's generator, a non-due step against a model built without
pl_weight bit for bit, graph replay against eager over 2 pl_interval iterations, and the trainer's entry point with the flags: the mean
path length in the checkpoint, its resume, a reader, and a checkpoint written without the flag.  Tiny widths, B = 4, so Bp = 2."""
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
import test_pggan_modconv_gpu as TM  # noqa: E402  (TINY, the model and feed builders)

pytestmark = pytest.mark.gpu

B, D, BP = TM.B, TM.D, 2
PL = dict(pl_weight=2.0, pl_interval=4, pl_shrink=2, pl_decay=0.01)
SEED = 1                                     # of the feed; the float32 CPU evaluation below stays under 1e-5 with it (else a relu branch flipped)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    return torch.device('cuda')


def pl_noise(stage, seed, dev=None):
    """y [Bp,H,W,3]: independent N(0,1) / sqrt(H W), float32 values (as float64 on the CPU, as float32 on `dev`)."""
    s = 4 * 2 ** (stage - 1)
    y = (np.random.default_rng(500 + seed).standard_normal((BP, s, s, 3)) / np.sqrt(s * s)).astype(np.float32)
    return torch.tensor(y.astype(np.float64)) if dev is None else torch.tensor(y, device=dev)


def reference_due_step(P, f, stage, trans, alpha, y, a0, dtype=torch.float64):
    """The due generator step in `dtype` on the CPU: G_loss as tests/test_pggan_modconv_gpu.py states it, the second pass over rows [:Bp],
    J = d sum(G y) / dw, L = |J|, a' = a + decay (mean L - a), pen = mean((L - a')^2), every generator gradient of G_loss + w n pen."""
    from oracle import torch_pggan as PG
    from oracle.torch_stackgan import kl_loss
    c = TM.cfg()
    cast = lambda t: t.to(dtype)
    f = {k: cast(v) for k, v in f.items()}
    names = PG.trainable(P, 'g_net')
    Q = {n: cast(v) for n, v in P.items()}
    for n in names:
        Q[n] = Q[n].detach().requires_grad_(True)
    nz = [f['style_noise_g_%d' % k] for k in range(2 * stage)]
    gen = lambda rows: MC.modconv_generator(PG.Vars(Q), c, f['z'][rows], f['cond'][rows], stage, trans, alpha, f['ca_noise_g'][rows], D, 4,
                                            [n[rows] for n in nz])
    Gg, mean, log_sigma, _ = gen(slice(None))
    Dgg = PG.discriminator(PG.Vars(Q), c, Gg, f['cond'], stage, trans, alpha)
    kl = kl_loss(mean, log_sigma)
    loss = -Dgg.mean() + c.kl_coeff * kl
    Gp, _, _, w = gen(slice(0, BP))
    assert float((Gp - Gg[:BP]).detach().abs().max()) <= (1e-12 if dtype == torch.float64 else 1e-4)       # the second pass is the main pass on those rows
    J, = torch.autograd.grad((Gp * cast(y)).sum(), [w], create_graph=True)
    L = torch.sqrt((J * J).sum(1))
    a1 = a0 + PL['pl_decay'] * (L.detach().mean() - a0)
    pen = ((L - a1) ** 2).mean()
    total = loss + PL['pl_weight'] * PL['pl_interval'] * pen
    grads = torch.autograd.grad(total, [Q[n] for n in names])
    return dict(G_loss=float(loss.detach()), pl_length=float(L.detach().mean()), pl_penalty=float(pen.detach()), pl_mean=float(a1),
                grads={n: g.double() for n, g in zip(names, grads)})


def _grad_err(got, ref):
    """Relative to the tensor's largest reference entry; an all-zero reference tensor is compared absolutely."""
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else ref
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.abs(got).max()) if np.abs(ref).max() < 1e-9 else MC.relerr(got, ref)


@pytest.mark.parametrize('stage,trans', [(1, False), (2, True), (3, False)], ids=['stage1', 'stage2t', 'stage3'])
def test_one_due_generator_step_against_float64(dev, stage, trans):
    """Measured on an MI355X (largest errors per configuration) in DESIGN.md section 4.46."""
    from t2i_amd.models.pggan.pggan import W_AVG
    m = TM.model(dev, stage, trans, **PL)
    TM.liven(m)
    P = {n: torch.tensor(a, dtype=torch.float64) for n, a in m.store.state().items() if n != W_AVG}
    f64, f32 = TM.feeds(stage, dev, seed=SEED)
    alpha, a0 = 0.3, 0.5
    m.set_alpha(alpha)
    ref = reference_due_step(P, f64, stage, trans, alpha, pl_noise(stage, SEED), a0)
    # the condition on the seed: float32 rounding alone, on the CPU, stays below 1e-5 (else a relu branch flipped: change SEED, never the bound)
    r32 = reference_due_step(P, f64, stage, trans, alpha, pl_noise(stage, SEED), a0, torch.float32)
    cpu32 = max([_grad_err(r32['grads'][n].numpy(), ref['grads'][n]) for n in ref['grads']] +
                [abs(r32[k] - ref[k]) / max(abs(ref[k]), 1e-30) for k in ('pl_length', 'pl_penalty', 'pl_mean')])
    print('float32 on the CPU against float64: %.2e' % cpu32)
    assert cpu32 < 1e-5, cpu32
    m.pl_mean.fill_(a0)
    g = m.g_losses(dict(f32, pl_noise=pl_noise(stage, SEED, dev)), pl=True)
    torch.cuda.synchronize()
    worst = []
    for k in ('pl_length', 'pl_penalty', 'pl_mean', 'G_loss'):
        worst.append(('g/' + k, abs(float(g[k]) - ref[k]) / max(abs(ref[k]), 1e-30)))
    assert float(m.pl_mean) == float(g['pl_mean'])                     # written back in place
    assert set(m.g_vars) == set(ref['grads'])
    for n in m.g_vars:
        worst.append(('g/grad/' + n, _grad_err(m.g_arena.grad_of(n), ref['grads'][n])))
    worst.sort(key=lambda t: -t[1])
    print('pggan path length stage %d%s: L %.6f pen %.6f; largest errors %s' % (
        stage, 't' if trans else '', ref['pl_length'], ref['pl_penalty'], ', '.join('%s %.2e' % t for t in worst[:4])))
    assert ref['pl_penalty'] > 0 and ref['pl_length'] > 0
    bad = [t for t in worst if t[1] > 1e-4]
    assert not bad, bad
    # the regulariser's gradient is in the total: without it the arena holds something else
    m.g_losses(f32)
    n = 'g_net/conv_stage_0/ModConv/weights'
    assert _grad_err(m.g_arena.grad_of(n), ref['grads'][n]) > 1e-3


def _state(m):
    out = {'var/' + n: v.detach().clone() for n, v in m.store.vars.items()}
    for tag, opt in (('d', m.D_optimizer), ('g', m.G_optimizer)):
        out.update({'%s/m' % tag: opt.m.clone(), '%s/v' % tag: opt.v.clone()})
    out['g/ema'] = m.G_optimizer.ema.clone()
    return out


def test_a_step_that_is_not_due_is_the_model_without_the_regulariser(dev):
    fs = [TM.feeds(2, dev, seed=s)[1] for s in (1, 2, 3, 4)]
    states = []
    for kw in ({}, PL):
        m = TM.model(dev, 2, True, adam_lr=1e-3, g_ema=0.9, **kw)
        TM.liven(m)
        outs = [m.iteration(i, fs[i - 1]) for i in (1, 2, 3)]
        torch.cuda.synchronize()
        assert all('pl_penalty' not in o['g'] for o in outs)
        states.append(_state(m))
    assert float(m.pl_mean) == 0.0
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k              # every variable, Adam slot and moving average
    out = m.iteration(4, fs[3])                                        # ... and step 4 is due
    assert float(out['g']['pl_penalty']) > 0 and float(m.pl_mean) == float(out['g']['pl_mean']) > 0.0
    assert abs(float(out['g']['pl_mean']) - 0.01 * float(out['g']['pl_length'])) <= 1e-6 * float(out['g']['pl_length'])


def test_graph_replay_matches_eager_over_two_intervals(dev):
    kw = dict(PL, pl_interval=2, adam_lr=1e-3)
    fs = [dict(TM.feeds(2, dev, seed=s)[1], pl_noise=pl_noise(2, s, dev)) for s in (1, 2, 3, 4, 5)]
    runs = []
    for use_graphs in (False, True):
        m = TM.model(dev, 2, True, **kw)
        TM.liven(m)
        m.iteration(1, fs[0])
        if use_graphs:
            m.enable_graphs(fs[0])
            assert set(m._graphs.graphs) == {'d', 'g', 'g_pl'} and tuple(m._graphs.static['pl_noise'].shape) == (BP, 8, 8, 3)
        means, losses = [], []
        for i in range(4):                                             # iterations 2 .. 5: two due, two not
            out = m.iteration(2 + i, fs[1 + i])
            torch.cuda.synchronize()
            means.append(float(m.pl_mean))
            losses.append((float(out['d']['D_loss']), float(out['g']['G_loss'])))       # (read now: a replay returns its static outputs)
            assert ('pl_penalty' in out['g']) == ((2 + i) % 2 == 0)
            if 'pl_penalty' in out['g']:
                losses.append((float(out['g']['pl_penalty']), float(out['g']['pl_length'])))
        assert 0.0 < means[0] == means[1] < means[2] == means[3]       # pl_mean moves on due steps only
        runs.append((_state_plain(m), means, losses))
    assert runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
    # without a fed image the static buffer is re-drawn before every due replay (and only then), scaled by 1 / sqrt(H W)
    bare = TM.feeds(2, dev, seed=2)[1]
    seen = [m._graphs.static['pl_noise'].clone()]
    for i in (6, 7, 8):
        m.iteration(i, bare)
        torch.cuda.synchronize()
        seen.append(m._graphs.static['pl_noise'].clone())
    assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[1], seen[2]) and not torch.equal(seen[2], seen[3])
    assert 0.5 / 8 < float(seen[3].std()) < 2.0 / 8


def _state_plain(m):
    out = {'var/' + n: v.detach().clone() for n, v in m.store.vars.items()}
    for tag, opt in (('d', m.D_optimizer), ('g', m.G_optimizer)):
        out.update({'%s/m' % tag: opt.m.clone(), '%s/v' % tag: opt.v.clone()})
    return out


def test_train_pggan_main_with_the_flags_checkpoints_and_resumes_the_mean_path_length(dev, tmp_path, capsys):
    from t2i_amd.models.pggan import eval_pggan as E
    from t2i_amd.models.pggan import options as O
    from t2i_amd.models.pggan import train_pggan as TP
    style = ['--style-dim', '16', '--mapping-layers', '2', '--modulated-conv', '--lr', '1e-3', '--iters', '3']
    flags = ['--pl-weight', '2', '--pl-interval', '2', '--pl-shrink', '4', '--pl-decay', '0.5']
    out = str(tmp_path / 'run')
    TP.main(['--out', out] + style + flags + ['--first', '0', '--last', '1'])
    z1 = np.load(os.path.join(out, 'checkpoints', 'stage1', 'model-2.npz'))
    z2 = np.load(os.path.join(out, 'checkpoints', 'stage2', 'model-2.npz'))
    assert O.PL_MEAN_KEY == 'pl_reg/pl_mean' and z1[O.PL_MEAN_KEY].shape == () and z1[O.PL_MEAN_KEY].dtype == np.float32
    a1, a2 = float(z1[O.PL_MEAN_KEY]), float(z2[O.PL_MEAN_KEY])
    assert a1 > 0.0 and a2 > 0.0 and a2 != a1                          # step 2 of each entry was due
    said = capsys.readouterr().out
    restored = re.search(r'path-length regularisation: pl_mean ([0-9.]+) restored', said)
    assert restored and abs(float(restored.group(1)) - a1) <= 1e-6     # the transition entry went on from stage 1's value
    # a reader needs no new flag
    cfg_like = type('C', (), {'CHECKPOINT_DIR': os.path.join(out, 'checkpoints')})()
    m = E.stage_model(cfg_like, 2, 4, None, dev, style_dim=16, mapping_layers=2, modulated_conv=True)
    E.restore_generator(m)
    n = 'g_net/conv_stage_1/ModConv/weights'
    assert np.array_equal(m.store.vars[n].detach().cpu().numpy(), z2[n])
    # a checkpoint written without the flag carries no such entry, and resumes with 0 and a line
    out = str(tmp_path / 'plain')
    TP.main(['--out', out] + style + ['--first', '0', '--last', '0'])
    assert O.PL_MEAN_KEY not in np.load(os.path.join(out, 'checkpoints', 'stage1', 'model-2.npz')).files
    capsys.readouterr()
    TP.main(['--out', out] + style + flags + ['--first', '1', '--last', '1'])
    assert 'carries no mean path length' in capsys.readouterr().out
    assert float(np.load(os.path.join(out, 'checkpoints', 'stage2', 'model-2.npz'))[O.PL_MEAN_KEY]) > 0.0
