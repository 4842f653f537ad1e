"""Precision, recall, density and coverage on the GPU: t2i_knn_dist2 and t2i_ball_counts (csrc/t2i_knn.hip) against the float64
restatement of tests/prdc_cases.py, ManifoldMetrics end to end, and GeneratorEval.evaluate_prdc.

Distances are compared within 2 band (prdc_cases.band: one band for the kernel's fp64 Gram form, one for the restatement's own
rounding); counts and metrics must be EQUAL, which the band condition on the inputs (asserted in tests/test_prdc_host.py and
again here) allows."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import prdc_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu

SEGMENTS = (1, 2, 7, 0)
IDS = dict(ids=lambda s: 'x'.join(str(v) for v in s))
METRICS = ('precision', 'recall', 'density', 'coverage')


@pytest.fixture(scope='module')
def K():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def knn_all_segments(K, q, r, k, exclude_self):
    """The kernel at every value of `segments` (those above N are left out) and twice at the first: all must be the same bits."""
    N = r.shape[0]
    outs = [K.knn_dist2(q, r, k, exclude_self=exclude_self, segments=s) for s in SEGMENTS if s <= N]
    outs.append(K.knn_dist2(q, r, k, exclude_self=exclude_self, segments=SEGMENTS[0]))
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    return outs[0].cpu().numpy()


def ball_all_segments(K, q, r, r2):
    N = r.shape[0]
    outs = [K.ball_counts(q, r, r2, segments=s) for s in SEGMENTS if s <= N]
    outs.append(K.ball_counts(q, r, r2, segments=SEGMENTS[0]))
    for c, d in outs[1:]:
        assert torch.equal(c, outs[0][0]) and torch.equal(d, outs[0][1])
    return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()


# ---- 1. knn_dist2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', PC.SHAPES, **IDS)
def test_knn_dist2_within_two_bands_of_the_restatement(K, shape):
    """(G, R) and (R, R, exclude_self): every output within 2 band of the restatement's value at the pair that attains it, rows
    ascending, the same bits for segments = 1, 2, 7, 0 and across a second call."""
    M, N, D, k = shape
    R, G, ref = PC.case(*shape)
    worst = 0.0
    for A, B, ex, d in ((G, R, False, ref['d_gr']), (R, R, True, None)):
        got = knn_all_segments(K, dev(A), dev(B), k, ex)
        want, idx = PC.knn(A, B, k, ex, d)
        bands = np.take_along_axis(PC.band(A, B), idx, 1)
        assert got.shape == want.shape == (A.shape[0], k) and got.dtype == np.float64
        assert np.all(np.diff(got, axis=1) >= 0) and np.all(got >= 0)
        ratio = np.abs(got - want) / bands
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 2.0), (shape, ex, float(ratio.max()))
    print('%s: largest |kernel - restatement| = %.3g band' % (shape, worst))


# ---- 2. ball_counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', PC.SHAPES, **IDS)
def test_ball_counts_equal_the_restatement(K, shape):
    M, N, D, k = shape
    R, G, ref = PC.case(*shape)
    assert PC.decision_margin(R, G, k, ref) > 2.0                                    # the condition for equality
    cnt, dmin = ball_all_segments(K, dev(G), dev(R), dev(ref['r2_real']))
    assert cnt.dtype == np.int32 and dmin.dtype == np.float64
    assert np.array_equal(cnt, ref['cnt_gen'])
    b = PC.band(G, R)
    assert np.all(np.abs(dmin - ref['dmin_gen']) <= 2.0 * b[np.arange(M), ref['d_gr'].argmin(1)])
    if M > k:                                                                        # (one query has no radius: no second direction)
        cnt, dmin = ball_all_segments(K, dev(R), dev(G), dev(ref['r2_gen']))
        assert np.array_equal(cnt, ref['cnt_real'])
        assert np.all(np.abs(dmin - ref['dmin_real']) <= 2.0 * b[ref['d_gr'].argmin(0), np.arange(N)])
        assert np.array_equal(dmin <= ref['r2_real'], ref['covered'])


# ---- 3. layout traps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(17, 35, 4), (16, 16, 5), (70, 130, 9)], **IDS)
def test_integer_features_are_exact(K, shape):
    """Integer-valued features with an asymmetric pattern: every d2 is an exact integer, so values and counts must EQUAL the
    restatement.  A wrong f64 accumulator map, a swapped operand or a mishandled tail in D, M or N cannot pass: D = 5 and 9 are no
    multiple of the MFMA's 4, 17 / 35 / 70 / 130 no multiple of the tile."""
    M, N, D = shape
    Q, R = PC.integer_sets(M, N, D)
    d = PC.dist2(Q, R)
    assert np.array_equal(d, np.round(d))
    for k in (1, min(8, N)):
        assert np.array_equal(knn_all_segments(K, dev(Q), dev(R), k, False), np.sort(d, axis=1)[:, :k])
    kk = min(3, N - 1)
    r2 = PC.knn(R, R, kk, True)[0]
    assert np.array_equal(knn_all_segments(K, dev(R), dev(R), kk, True), r2)
    cnt, dmin = ball_all_segments(K, dev(Q), dev(R), dev(r2[:, kk - 1]))
    assert np.array_equal(cnt, (d <= r2[None, :, kk - 1]).sum(1)) and np.array_equal(dmin, d.min(1))
    if M == N:                                             # with itself and without exclusion: the zero on the diagonal comes first
        assert np.all(knn_all_segments(K, dev(Q), dev(Q), 1, False) == 0.0)


# ---- 4. duplicates -----------------------------------------------------------------------------------------------------------------
def test_duplicates_are_neighbours_by_the_index_rule(K):
    """Every real row has an exact copy and ten generated rows are real rows.  exclude_self skips the query's own INDEX, so the
    copy is its first neighbour at distance 0 and the k = 3 radius is a genuine distance (at least 2e12 bands)."""
    R, G = PC.duplicates()
    k = 3
    ref = PC.restate(R, G, k)
    own = PC.band(R, R)[np.arange(60), np.arange(60)]
    assert (ref['r2_real'] / own).min() >= 2e12
    got = knn_all_segments(K, dev(R), dev(R), k, True)
    want, idx = PC.knn(R, R, k, True)
    bands = np.take_along_axis(PC.band(R, R), idx, 1)
    assert np.all(np.abs(got - want) <= bands)
    assert np.all(got[:, 0] <= own) and np.all(want[:, 0] == 0.0)                    # the copy
    cnt, dmin = ball_all_segments(K, dev(G), dev(R), dev(ref['r2_real']))
    b = PC.band(G, R)
    assert np.all(np.abs(dmin[:10]) <= 2.0 * b[np.arange(10), np.arange(10)])
    assert np.all(cnt[:10] >= 2)                           # the real row and its copy, both at distance 0 <= a genuine radius
    # (no equality with the restatement's counts here: a copy of R_i lies EXACTLY on the ball of every R_n whose k-th neighbour is R_i)


def test_nan_and_missing_candidates(K):
    """A NaN distance is never selected or counted; a slot with no finite candidate holds +inf."""
    R, G, _ = PC.case(65, 130, 36, 3)
    Rn = R.copy()
    Rn[5, 7] = np.nan
    got = knn_all_segments(K, dev(G), dev(Rn), 3, False)
    keep = np.arange(130) != 5
    want = PC.knn(G, R[keep], 3)[0]
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 2.0 * PC.band(G, R).max())
    r2 = np.full(130, 1e30)
    cnt, dmin = ball_all_segments(K, dev(G), dev(Rn), dev(r2))
    assert np.all(cnt == 129) and np.all(np.isfinite(dmin))
    allnan = np.full((3, 36), np.nan, np.float32)
    got = K.knn_dist2(dev(G), dev(allnan), 2).cpu().numpy()
    assert np.all(np.isposinf(got))
    cnt, dmin = K.ball_counts(dev(G), dev(allnan), dev(np.full(3, 1e30)))
    assert np.all(cnt.cpu().numpy() == 0) and np.all(np.isposinf(dmin.cpu().numpy()))


# ---- 5. ManifoldMetrics ------------------------------------------------------------------------------------------------------------
def feed(mm, R, G):
    for a, b in ((0, 1), (1, R.shape[0] // 3), (R.shape[0] // 3, R.shape[0])):
        mm.add_real(dev(R[a:b]))
    for a, b in ((0, G.shape[0] // 2 + 3), (G.shape[0] // 2 + 3, G.shape[0] - 1), (G.shape[0] - 1, G.shape[0])):
        mm.add_gen(dev(G[a:b]))
    return mm


@pytest.mark.parametrize('shape', [(129, 300, 100, 5), (100, 257, 2048, 5)], **IDS)
def test_manifold_metrics_equal_the_restatement(K, shape):
    from t2i_amd.evaluation.prdc import ManifoldMetrics
    M, N, D, k = shape
    R, G, ref = PC.case(*shape)
    out = feed(ManifoldMetrics(D, 'cuda', nearest_k=k), R, G).finalize()
    assert out == {key: ref[key] for key in METRICS + ('nearest_k', 'n_real', 'n_gen')}
    assert all(type(out[key]) is float for key in METRICS)
    perm = np.random.RandomState(3).permutation(N)
    assert feed(ManifoldMetrics(D, 'cuda', nearest_k=k), R[perm], G).finalize() == out
    same = feed(ManifoldMetrics(D, 'cuda', nearest_k=k), R, R).finalize()
    assert same['precision'] == same['recall'] == same['coverage'] == 1.0 and same['n_gen'] == N


def test_the_chain_of_passes_replays_from_a_graph(K):
    """manifold_passes only enqueues work: captured once, replayed on fresh inputs of the same shape, it equals the eager chain."""
    from t2i_amd.evaluation import prdc
    M, N, D, k = 129, 300, 100, 5
    R, G, ref = PC.case(M, N, D, k)
    R2, G2 = PC.latent(M, N, D, 77)
    real, gen = dev(R2), dev(G2)
    eager2 = [t.clone() for t in prdc.manifold_passes(real, gen, k)]                 # (the workspace exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = prdc.manifold_passes(real, gen, k)
    real.copy_(dev(R))
    gen.copy_(dev(G))
    g.replay()
    torch.cuda.synchronize()
    cnt_gen, cnt_real, covered = (t.cpu().numpy() for t in outs)
    assert np.array_equal(cnt_gen, ref['cnt_gen']) and np.array_equal(cnt_real, ref['cnt_real']) and np.array_equal(covered, ref['covered'])
    assert prdc.ratios(cnt_gen, cnt_real, covered, k) == {key: ref[key] for key in METRICS + ('nearest_k', 'n_real', 'n_gen')}
    real.copy_(dev(R2))
    gen.copy_(dev(G2))
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, eager2))


def test_manifold_metrics_refusals(K):
    from t2i_amd.evaluation.prdc import ManifoldMetrics
    R, G, _ = PC.case(65, 130, 36, 3)
    for k in (0, 9):
        with pytest.raises(ValueError, match='nearest_k'):
            ManifoldMetrics(36, 'cuda', nearest_k=k)
    mm = ManifoldMetrics(36, 'cuda', nearest_k=3)
    mm.add_real(dev(R))
    mm.add_gen(dev(G[:3]))
    with pytest.raises(ValueError, match='3 generated rows'):
        mm.finalize()
    mm.add_gen(dev(G[3:]))
    bad = R[:1].copy()
    bad[0, 4] = np.nan
    mm.add_real(dev(bad))
    with pytest.raises(ValueError, match='real feature is not finite'):
        mm.finalize()


# ---- 6. the evaluator ---------------------------------------------------------------------------------------------------------------
def _evaluator(gen_fn):
    from t2i_amd.evaluation.evaluator import GeneratorEval
    from t2i_amd.utils.config import AttrDict
    rs = np.random.RandomState(21)
    lat = rs.randn(12, 6).astype(np.float32)
    basis = rs.randn(6, 16 * 16 * 3).astype(np.float32) / 4
    store = torch.from_numpy(np.tanh(lat @ basis).reshape(12, 16, 16, 3).astype(np.float32)).cuda()
    proj = torch.from_numpy(np.random.RandomState(22).randn(8 * 8 * 3, 64).astype(np.float32)).cuda()

    class Split(object):
        num_examples = 12

        def __init__(self):
            self.at, self.last = 0, None

        def next_batch(self, bs, k, embeddings=True):
            self.last = store[self.at:self.at + bs]
            self.at = (self.at + bs) % store.shape[0]
            return self.last, None, np.random.standard_normal((bs, 8)).astype(np.float32), None, None

    class Data(object):
        pass

    class Model(object):
        device, z_dim, embed_dim = torch.device('cuda'), 4, 8

    def net(x):
        """(logits, pre): pre a fixed linear map of the 8 x 8 average-pooled 299 x 299 input to 64 features."""
        assert tuple(x.shape[1:]) == (299, 299, 3)
        pooled = torch.nn.functional.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), 8).permute(0, 2, 3, 1).reshape(x.shape[0], -1)
        return torch.zeros(x.shape[0], 20, device=x.device), (pooled @ proj).reshape(x.shape[0], 1, 1, 64)

    class Ev(GeneratorEval):
        def restore(self):
            self.restored = True

        def _inception(self):
            return net

        def generate_batch(self, z, cond, is_training):
            assert not is_training
            return gen_fn(self, z, cond)

    data = Data()
    data.test = Split()
    return Ev(None, Model(), data, AttrDict({'EVAL': {'SIZE': 22, 'SAMPLE_SIZE': 4, 'INCEP_BATCH_SIZE': 4}}))


def _shifted(ev, z, cond):
    """Images that depend on the batch's reals, on z and on the embeddings."""
    real = ev.dataset.test.last
    return torch.clamp(0.7 * real + 0.1 * z.mean(1).reshape(-1, 1, 1, 1) + 0.05 * cond.mean(1).reshape(-1, 1, 1, 1), -1, 1)


def test_evaluate_prdc_against_the_restatement_on_its_features(K, capsys):
    """A store of 12 images, batches of 4, SIZE 22: five batches, of which only the first three (one epoch) feed the real set."""
    def run():
        ev = _evaluator(_shifted)
        np.random.seed(5)
        out = ev.evaluate_prdc(nearest_k=2, keep_features=True)
        assert ev.restored
        return out, np.random.get_state()

    a, state_a = run()
    text = capsys.readouterr().out
    b, _ = run()
    assert a['n_real'] == 12 and a['n_gen'] == 20 and a['nearest_k'] == 2
    assert a['real_features'].shape == (12, 64) and a['gen_features'].shape == (20, 64) and a['real_features'].dtype == np.float32
    assert all(a[key] == b[key] for key in METRICS) and np.array_equal(a['real_features'], b['real_features'])
    assert np.array_equal(a['gen_features'], b['gen_features'])
    ref = PC.restate(a['real_features'], a['gen_features'], 2)
    margin = PC.decision_margin(a['real_features'], a['gen_features'], 2, ref)
    print('closest decision: %.3g bands' % margin)
    assert margin > 2.0
    assert all(a[key] == ref[key] for key in METRICS)
    assert text.count('PRDC (k = 2) |') == 1 and '12 real, 20 generated' in text and 'precision: %.4f' % a['precision'] in text

    ev = _evaluator(_shifted)                              # the global numpy stream: that of evaluate_imd on the same setup
    np.random.seed(5)
    ev.evaluate_imd()
    state_imd = np.random.get_state()
    assert state_a[0] == state_imd[0] and np.array_equal(state_a[1], state_imd[1]) and state_a[2:] == state_imd[2:]


def test_evaluate_prdc_of_a_generator_that_returns_the_reals(K):
    ev = _evaluator(lambda ev, z, cond: ev.dataset.test.last.clone())
    np.random.seed(5)
    out = ev.evaluate_prdc(nearest_k=2)
    assert out['precision'] == 1.0 and out['coverage'] == 1.0 and out['n_real'] == 12 and out['n_gen'] == 20
    with pytest.raises(ValueError, match='nearest_k'):
        ev.evaluate_prdc(nearest_k=0)
