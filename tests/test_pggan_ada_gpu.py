"""PGGAN(diffaug_p=..., diffaug_adapt=..., diffaug_sampler=...) on the GPU.  The defaults are the model built
without the arguments, bit for bit.  With a sampler an unfed table is drawn inside the step: one iteration equals, bit for bit, that of
a model WITHOUT a sampler that is fed the numpy restatement's tables for calls 0 and 1 (tests/ada_cases.py) — which ties the in-step
draw to the path tests/test_pggan_diffaug_gpu.py checks against the float64 oracle, with no tolerance of its own.  Graph replay equals
eager launches, arenas and state words; a bare replay advances the call counter by two; the controller's state after five adapting
iterations is the restatement's on the logits the steps returned; and the state words travel through a checkpoint.  Tiny widths and
the `synthetic_feed` conventions of tests/test_pggan_diffaug_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import ada_cases as AC  # noqa: E402
import diffaug_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = dict(z_dim=8, embed_dim=32, compressed=16, base=32, cap=16)                   # tests/test_pggan_diffaug_gpu.py's widths
WIDTHS = dict(fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)
STEPS, BATCH = 10, 8
POLICY = DC.ALL


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from oracle import torch_pggan as PG
    return PG


def _model(stage, trans, batch=BATCH, seed=5, **kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    return PGGAN(batch, STEPS, None, None, None, None, None, stage, trans, device=torch.device('cuda'), seed=seed, **WIDTHS, **kw)


def _feeds(PG, stage, batch=BATCH, count=6):
    """fixed eps and conditioning noise, no tables"""
    cfg = PG.Cfg(**dict(CFG, batch=batch))
    feeds = []
    for s in range(1, count + 1):
        f = {k: v.float().cuda() for k, v in PG.synthetic_feed(cfg, stage, seed=s).items()}
        feeds.append({'x': f['x'], 'x_mismatch': f['x_mismatch'], 'cond': f['cond'], 'z': f['z'], 'eps_graph': f['eps'],
                      'ca_noise_d': f['ca_noise_d'], 'ca_noise_g': f['ca_noise_g']})
    return feeds


def _arenas(m):
    torch.cuda.synchronize()
    return m.d_arena.flat.detach().clone(), m.g_arena.flat.detach().clone()


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_the_defaults_are_the_model_built_without_the_arguments():
    PG = need_gpu()
    feed = dict(_feeds(PG, 2, count=1)[0], aug_d=DC.drawn_table(4 * BATCH, 8, 8, 3).float().cuda(), aug_g=DC.drawn_table(BATCH, 8, 8, 4).float().cuda())
    outs = []
    for kw in ({}, dict(diffaug_p=None, diffaug_adapt=False, diffaug_sampler=None)):
        m = _model(2, True, diffaug=POLICY, **kw)
        assert m.aug_sampler is None
        out = m.iteration(3, feed)
        assert 'aug_p' not in out['d'] and 'Dx_logit' not in out['d']
        outs.append((_arenas(m), sorted(out['d'])))
    assert _same(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and bool(outs[0][0][0].abs().max() > 0)


@pytest.mark.parametrize('trans', [False, True], ids=['stable', 'transition'])
def test_an_unfed_table_is_the_restatements_table(trans):
    PG = need_gpu()
    feed = _feeds(PG, 2, count=1)[0]
    m = _model(2, trans, seed=5, diffaug=POLICY, diffaug_p=0.5)
    assert np.array_equal(m.aug_sampler.state_dict(), AC.make_state(5, 0.5))
    out = m.iteration(3, feed)
    got = _arenas(m)
    assert m.aug_sampler.counter == 2 and float(out['d']['aug_p']) == 0.5 and out['d']['aug_p'].is_cuda
    assert tuple(out['d']['Dx_logit'].shape) == (BATCH,) and tuple(out['d']['Dg_logit'].shape) == (BATCH,)
    aug_d, after = AC.draw(AC.make_state(5, 0.5), 4 * BATCH, 8, 8, 7)                 # call 0: the critic step's
    aug_g, after = AC.draw(after, BATCH, 8, 8, 7)                                     # call 1: the generator step's
    assert np.array_equal(m.aug_sampler.state_dict(), after)
    on = AC.gates(AC.make_state(5, 0.5), 4 * BATCH)
    assert on.any() and not on.all()                                                   # some rows transformed, some the identity
    ref = _model(2, trans, seed=5, diffaug=POLICY)
    ref.iteration(3, dict(feed, aug_d=torch.from_numpy(aug_d).cuda(), aug_g=torch.from_numpy(aug_g).cuda()))
    assert _same(got, _arenas(ref))
    # a fed table still wins: nothing is drawn and the counter does not move
    m.iteration(4, dict(feed, aug_d=torch.from_numpy(aug_d).cuda(), aug_g=torch.from_numpy(aug_g).cuda()))
    torch.cuda.synchronize()
    assert m.aug_sampler.counter == 2


def test_graph_replay_matches_eager_with_unfed_tables_and_a_bare_replay_draws_twice():
    PG = need_gpu()
    from t2i_amd.utils.ops import DiffAugmentSampler
    feeds = _feeds(PG, 2, count=3)
    states = []
    for use_graphs in (False, True):
        s = DiffAugmentSampler(POLICY, p=0.5, seed=9, device='cuda', adapt='midpoint', interval=2, ramp_images=8 * BATCH)
        m = _model(2, True, diffaug=POLICY, diffaug_adapt=True, diffaug_sampler=s)
        m.iteration(1, feeds[0])
        if use_graphs:
            m.enable_graphs(feeds[0])
            assert 'aug_d' not in m._graphs.static and 'aug_g' not in m._graphs.static
            assert s.counter == 2                                                       # capturing drew nothing
        outs = [m.iteration(2 + 2 * i, feeds[1 + i]) for i in range(2)]
        states.append((_arenas(m), s.state_dict(), float(outs[-1]['d']['aug_p']), float(outs[-1]['d']['D_loss'])))
    (a0, w0, p0, l0), (a1, w1, p1, l1) = states
    assert _same(a0, a1) and np.array_equal(w0, w1) and p0 == p1 and l0 == l1
    assert AC.counter_of(w1) == 6 and int(w1[9]) == 1 and int(w1[7]) == 1             # three observations, interval 2
    m._graphs.replay('d')
    m._graphs.replay('g')
    torch.cuda.synchronize()
    w2 = s.state_dict()
    assert AC.counter_of(w2) == 8 and int(w2[9]) == 2 and int(w2[7]) == 0
    with pytest.raises(ValueError, match='aug_d'):                                       # captured drawing it: a table fed now would be ignored
        m.iteration(7, dict(feeds[2], aug_d=torch.zeros(4 * BATCH, 9, device='cuda')))


def test_the_controller_follows_the_restatement_over_five_iterations():
    PG = need_gpu()
    from t2i_amd.utils.ops import DiffAugmentSampler
    feeds = _feeds(PG, 2, count=5)
    ramp = 8 * BATCH
    s = DiffAugmentSampler(POLICY, p=0.5, seed=9, device='cuda', adapt='midpoint', target=0.6, interval=2, ramp_images=ramp)
    m = _model(2, False, diffaug=POLICY, diffaug_adapt=True, diffaug_sampler=s)
    words, ps = AC.make_state(9, 0.5), []
    for i, feed in enumerate(feeds):
        out = m.iteration(1 + i, feed)
        dx, dg = out['d']['Dx_logit'].cpu().numpy(), out['d']['Dg_logit'].cpu().numpy()
        # no sign may hang on the rounding of the threshold, which the kernel forms in float32: a few ulp of the logits' scale
        scale = max(float(np.abs(dx).max()), float(np.abs(dg).max()))
        print('iteration %d: margin %.3e of scale %.3e' % (i, AC.margin(dx, dg, AC.MIDPOINT), scale))
        assert AC.margin(dx, dg, AC.MIDPOINT) > 1e-5 * scale
        words[2] += 2                                                                   # the two draws
        words = AC.observe(words, dx, dg, AC.MIDPOINT, 0.6, 2, float(ramp))
        got = s.state_dict()
        for j in (0, 1, 2, 3, 5, 6, 7, 9) + tuple(range(10, 16)):
            assert int(got[j]) == int(words[j]), (i, j)
        for j in (4, 8):
            assert abs(float(AC.f32_of(got[j])) - float(AC.f32_of(words[j]))) <= 1e-6, (i, j)
        assert abs(float(out['d']['aug_p']) - float(AC.f32_of(words[4]))) <= 1e-6
        ps.append(float(AC.f32_of(words[4])))
    assert int(words[9]) == 2 and ps[0] == 0.5 and ps[1] != 0.5 and abs(ps[1] - 0.5) == 0.25    # p moved, by 2 * BATCH / ramp
    assert s.updates == 2 and abs(s.last_r - float(AC.f32_of(words[8]))) <= 1e-6


def _dataset(size):
    from t2i_amd.data import SyntheticTextDataset
    from t2i_amd.utils.config import AttrDict
    dcfg = AttrDict({'MODEL': {'Z_DIM': WIDTHS['z_dim'], 'OUTPUT_SIZE': size, 'EMBED_DIM': WIDTHS['embed_dim'], 'IMAGE_SHAPE': {'W': size, 'H': size, 'D': 3}},
                     'TRAIN': {'BATCH_SIZE': 4}})
    return SyntheticTextDataset(dcfg, torch.device('cuda'), seed=5, num_examples=512)


def test_the_state_words_travel_through_a_checkpoint(tmp_path):
    """Stage 1 then the transition to stage 2.  Uninterrupted: one sampler through both entries.  Interrupted: the second entry starts
    with a fresh sampler (another seed, another p) and gets the words from stage 1's checkpoint.  Both end in the same words and arenas.
    A run without a sampler writes no such key, and restoring its checkpoint into a run with one logs a line and leaves the sampler."""
    need_gpu()
    from t2i_amd.models.pggan.pggan import PGGAN
    from t2i_amd.utils.ops import DiffAugmentSampler

    def sampler(seed, p):
        return DiffAugmentSampler(POLICY, p=p, seed=seed, device='cuda', adapt='midpoint', interval=1, ramp_images=16)

    def run(root, second_sampler, first_sampler=True):
        ck = lambda k: os.path.join(root, 'ckpt', 'stage%d/' % k)       # noqa: E731
        logs = []
        for d in (ck(1), ck(2), os.path.join(root, 's1'), os.path.join(root, 's2')):
            os.makedirs(d, exist_ok=True)
        torch.manual_seed(77)
        s = sampler(3, 0.5) if first_sampler else None
        kw = dict(diffaug=POLICY, **({} if s is None else dict(diffaug_adapt=True, diffaug_sampler=s)))
        m1 = PGGAN(4, 100, ck(1), ck(1), _dataset(4), os.path.join(root, 's1') + '/', None, 1, False, device=torch.device('cuda'), seed=11, **WIDTHS, **kw)
        m1.train(max_steps=4, log=logs.append, side_effects=True)
        z = np.load(os.path.join(ck(1), 'model-3.npz'))
        if s is not None:
            assert np.array_equal(z['diffaug/state'], s.state_dict()) and z['diffaug/state'].dtype == np.int64 and s.counter == 6
        else:
            assert 'diffaug/state' not in z.files
        s2 = second_sampler(s)
        m2 = PGGAN(4, 100, ck(2), ck(1), _dataset(8), os.path.join(root, 's2') + '/', None, 2, True, device=torch.device('cuda'), seed=12, **WIDTHS,
                   diffaug=POLICY, diffaug_adapt=True, diffaug_sampler=s2)
        m2.train(max_steps=4, log=logs.append, side_effects=True)
        return _arenas(m2), s2.state_dict(), logs

    a0, w0, logs0 = run(str(tmp_path / 'whole'), lambda s: s)
    a1, w1, logs1 = run(str(tmp_path / 'resumed'), lambda s: sampler(99, 0.125))
    assert np.array_equal(w0, w1) and _same(a0, a1) and AC.counter_of(w0) == 12 and int(w0[9]) == 6
    assert not any('augmentation state' in line for line in logs0 + logs1)
    fresh = AC.make_state(99, 0.125)
    a2, w2, logs2 = run(str(tmp_path / 'without'), lambda s: sampler(99, 0.125), first_sampler=False)
    assert sum('augmentation state' in line for line in logs2) == 1
    assert np.array_equal(w2[:2], fresh[:2]) and AC.counter_of(w2) == 6                # started fresh: its own seed, three iterations
