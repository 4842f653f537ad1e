"""Sliced Wasserstein distance on the GPU: every kernel of csrc/t2i_swd.hip against the float64 restatement of tests/swd_cases.py
(scipy.ndimage for the pyramid, numpy for the rest), SlicedWasserstein end to end, and GeneratorEval.evaluate_swd."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import swd_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()          # a copy: np.sort(...)[:, ::-1] has negative strides


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,levels', [((2, 16, 16, 3), 1), ((2, 32, 32, 3), 2), ((1, 64, 64, 1), 3), ((1, 32, 64, 3), 2),
                                          ((3, 48, 80, 2), 2)], ids=lambda v: str(v).replace(' ', ''))
def test_laplacian_pyramid_matches_scipy(K, shape, levels):
    """max |delta| <= 4e-6 max |x| per level (51 roundings of 2^-24: 25 + 25 taps and the subtraction); the edge rows and columns
    are asserted on their own so that a wrong mirror cannot hide behind the interior.  (3, 48, 80, 2): more than one tile of the
    reduction in both directions, a partial tile, two channels."""
    x = SC.images(5, *shape)
    want = SC.laplacian_pyramid(x, levels)
    got = K.laplacian_pyramid(dev(x), levels)
    again = K.laplacian_pyramid(dev(x), levels)
    bound = 4e-6 * float(np.abs(x).max())
    assert len(got) == levels
    for i, (g, w) in enumerate(zip(got, want)):
        assert tuple(g.shape) == w.shape == (shape[0], shape[1] >> i, shape[2] >> i, shape[3])
        assert torch.equal(g, again[i])
        err = np.abs(g.cpu().numpy().astype(np.float64) - w)
        print('level %d: interior %.3g, edges %.3g (bound %.3g)' % (i, err[:, 2:-2, 2:-2].max(), max(
            err[:, :2].max(), err[:, -2:].max(), err[:, :, :2].max(), err[:, :, -2:].max()), bound))
        for name, part in (('top rows', err[:, :2]), ('bottom rows', err[:, -2:]), ('left columns', err[:, :, :2]),
                           ('right columns', err[:, :, -2:]), ('interior', err[:, 2:-2, 2:-2])):
            assert part.max() <= bound, (i, name, part.max())


# ---- descriptors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,C', [(16, 16, 3), (9, 23, 1), (32, 32, 4)])
def test_descriptors_are_numpy_fancy_indexing_bit_for_bit(K, h, w, C):
    rng = np.random.RandomState(3)
    N, P = 3, 37
    level = rng.standard_normal((N, h, w, C)).astype(np.float32)
    pos = np.stack([rng.randint(3, h - 3, size=(N, P)), rng.randint(3, w - 3, size=(N, P))], -1).astype(np.int32)
    pos[0, :4] = [[3, 3], [3, w - 4], [h - 4, 3], [h - 4, w - 4]]           # the four corner centres
    for row0, total in ((0, N * P), (5, N * P + 9)):
        out = torch.full((total, 49 * C), -7.0, device='cuda')
        K.swd_descriptors(dev(level), pos, out, row0)
        got = out.cpu().numpy()
        assert np.array_equal(got[row0:row0 + N * P], SC.descriptors(level, pos))
        assert np.all(got[:row0] == -7.0) and np.all(got[row0 + N * P:] == -7.0)          # nothing else is written


# ---- channel statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,C', [(1, 1), (129, 3), (129, 1), (30011, 4)])
def test_channel_stats_in_fp64(K, rows, C):
    """Relative 1e-12 against numpy's float64.  The data has a mean of the order of its spread (a mean that cancels to nothing has
    no relative accuracy in any summation order); 129 and 30011 rows are no multiple of the 4096-element tile, 30011 x 196
    elements are more tiles than the 1024 workgroups, so the round-robin over tiles runs too."""
    rng = np.random.RandomState(rows + C)
    A = (rng.standard_normal((rows, 49 * C)) * np.repeat(np.arange(1, C + 1), 49) + np.repeat(np.arange(C) - 1.5, 49)).astype(np.float32)
    mean, std = K.swd_channel_stats(dev(A), C)
    m2, s2 = K.swd_channel_stats(dev(A), C)
    wm, ws = SC.channel_stats(A, C)
    assert torch.equal(mean, m2) and torch.equal(std, s2)
    em, es = np.abs(mean.cpu().numpy() - wm) / np.abs(wm), np.abs(std.cpu().numpy() - ws) / ws
    print('relative error: mean %.3g, std %.3g' % (em.max(), es.max()))
    assert em.max() <= 1e-12 and es.max() <= 1e-12


# ---- projection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [128, 40])
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('rows', [1, 129])
def test_projection_standardises_on_load_and_pads_with_inf(K, rows, C, S):
    """Per entry |delta| <= (D + 2) 2^-24 sum_j |a^_j d_j| (float64 restatement from the same fp64 statistics); S = 40 is no multiple
    of a wave's 32 slices.  The padding is exactly +inf."""
    rng = np.random.RandomState(rows * 7 + C + S)
    D = 49 * C
    A = (rng.standard_normal((rows, D)) * 0.3 + 0.1).astype(np.float32)
    mean, std = rng.standard_normal(C) * 0.1, rng.uniform(0.2, 0.5, C)          # any statistics: the kernel takes them as given
    dirs = rng.standard_normal((D, S))
    dirs = (dirs / np.sqrt((dirs * dirs).sum(0, keepdims=True))).astype(np.float32)
    out = K.swd_project(dev(A), dev(mean), dev(std), dev(dirs))
    pad = K.next_pow2(rows)
    assert tuple(out.shape) == (S, pad)
    got = out.cpu().numpy()
    a_hat = SC.standardise(A, C, mean, std)
    want = (a_hat @ dirs.astype(np.float64)).T
    bound = ((D + 2) * 2.0 ** -24 * (np.abs(a_hat) @ np.abs(dirs.astype(np.float64)))).T
    err = np.abs(got[:, :rows].astype(np.float64) - want)
    print('largest error / bound: %.3g' % (err / bound).max())
    assert np.all(err <= bound)
    assert np.all(np.isposinf(got[:, rows:])) and got[:, rows:].size == S * (pad - rows)
    assert torch.equal(out, K.swd_project(dev(A), dev(mean), dev(std), dev(dirs)))


# ---- segmented sort --------------------------------------------------------------------------------------------------------------
def _sort_inputs(rng, segments, n):
    yield 'random', rng.standard_normal((segments, n)).astype(np.float32)
    yield 'duplicates', rng.randint(-3, 4, size=(segments, n)).astype(np.float32)
    yield 'sorted', np.sort(rng.standard_normal((segments, n)).astype(np.float32), axis=1)
    yield 'reversed', np.sort(rng.standard_normal((segments, n)).astype(np.float32), axis=1)[:, ::-1]
    tail = rng.standard_normal((segments, n)).astype(np.float32)
    tail[:, n - n // 3:] = np.inf                          # the projection's padding (n = 1, 2: none, and the whole of nothing)
    yield 'inf tail', tail


CHUNK = 4096                                               # include/t2i_hip.h T2I_SORT_CHUNK (asserted below)


@pytest.mark.parametrize('segments,n', [(s, n) for n in (1, 2, CHUNK // 2, CHUNK, 2 * CHUNK, 8 * CHUNK) for s in (1, 3)] + [(256, 2 * CHUNK)])
def test_segmented_sort_equals_numpy(K, segments, n):
    """len straddles the LDS chunk: below it one launch, at 2 x one global pass per merge, at 8 x passes of one, two and three
    strides."""
    assert K.SORT_CHUNK == CHUNK
    rng = np.random.RandomState(segments * 31 + n)
    for name, x in _sort_inputs(rng, segments, n):
        d = dev(x)
        assert K.segmented_sort(d) is d
        assert np.array_equal(d.cpu().numpy(), np.sort(x, axis=1)), name


# ---- sorted L1 mean --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('segments,n,rows', [(3, 8192, 5000), (1, 1, 1), (128, 256, 129)])
def test_sorted_l1_mean_reads_only_the_valid_rows(K, segments, n, rows):
    rng = np.random.RandomState(n)
    a, b = rng.standard_normal((2, segments, n)).astype(np.float32)
    a[:, rows:] = np.inf                                   # inf - inf would be NaN: the padding must not be read
    b[:, rows:] = np.inf
    got = K.sorted_l1_mean(dev(a), dev(b), rows)
    want = np.mean(np.abs(a[:, :rows].astype(np.float64) - b[:, :rows].astype(np.float64)))
    assert got.dtype == torch.float64 and tuple(got.shape) == (1,)
    assert abs(float(got) - want) <= 1e-12 * want
    assert torch.equal(got, K.sorted_l1_mean(dev(a), dev(b), rows))


def test_sort_and_l1_mean_are_capturable(K):
    rng = np.random.RandomState(9)
    x = rng.standard_normal((4, 2 * K.SORT_CHUNK)).astype(np.float32)
    d = dev(x)
    K.sorted_l1_mean(d[:2], d[2:], 100)                    # the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.segmented_sort(d)
        out = K.sorted_l1_mean(d[:2], d[2:], 5000)
    d.copy_(dev(x))
    g.replay()
    torch.cuda.synchronize()
    s = np.sort(x, axis=1).astype(np.float64)
    assert np.array_equal(d.cpu().numpy(), np.sort(x, axis=1))
    want = np.mean(np.abs(s[:2, :5000] - s[2:, :5000]))
    assert abs(float(out) - want) <= 1e-12 * want


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_sliced_wasserstein_end_to_end_against_the_restatement(K):
    """Two batches of 4 images of 32 x 32 x 3, P = 16: the restatement is fed the same centre tables and directions (the draw
    order of evaluation/swd.py, replayed here).  Per level |delta| <= the largest projection error bound (D + 2) 2^-24 sum |a^ d|
    over both sets and all repeats: a sorted-L1 mean is 1-Lipschitz in the projections."""
    from t2i_amd.evaluation.swd import SlicedWasserstein
    n, side, C, P, R, S, seed = 4, 32, 3, 16, 4, 128, 11
    real = [SC.images(20 + i, n, side, side, C) for i in range(2)]
    gen = [np.clip(0.8 * SC.images(40 + i, n, side, side, C) + 0.1, -1, 1).astype(np.float32) for i in range(2)]
    sw = SlicedWasserstein((side, side, C), 2 * n, 'cuda', seed=seed, nhoods=P, verbose=False)
    for r, g in zip(real, gen):
        sw.add(dev(r), dev(g))
    out = sw.finalize()
    assert out['sides'] == [32, 16] and len(out['levels']) == 2 and out['mean'] == pytest.approx(np.mean(out['levels']), rel=1e-15)

    rs = np.random.RandomState(seed)
    A, B = [[], []], [[], []]
    for r, g in zip(real, gen):
        pr, pg = SC.laplacian_pyramid(r, 2), SC.laplacian_pyramid(g, 2)
        for i, s in enumerate((32, 16)):
            A[i].append(SC.descriptors(pr[i], rs.randint(3, s - 3, size=(n, P, 2))))
            B[i].append(SC.descriptors(pg[i], rs.randint(3, s - 3, size=(n, P, 2))))
    for i in range(2):
        a, b = np.concatenate(A[i]), np.concatenate(B[i])
        dirs = []
        for _ in range(R):
            d = rs.randn(49 * C, S)
            dirs.append((d / np.sqrt((d * d).sum(0, keepdims=True))).astype(np.float32))
        want = SC.sliced_distance(a, b, dirs, C) * 1e3
        bound = max(max(SC.projection_bound(a, C, d).max(), SC.projection_bound(b, C, d).max()) for d in dirs) * 1e3
        print('level %d: %.6f (restatement %.6f, |delta| %.3g, bound %.3g)' % (i, out['levels'][i], want, abs(out['levels'][i] - want), bound))
        assert want > 1.0 and abs(out['levels'][i] - want) <= bound


def test_zero_variance_channel_is_named(K):
    from t2i_amd.evaluation.swd import SlicedWasserstein
    x = SC.images(1, 2, 16, 16, 3)
    flat = x.copy()
    flat[..., 1] = 0.25
    sw = SlicedWasserstein((16, 16, 3), 2, 'cuda', nhoods=8, verbose=False)
    sw.add(dev(x), dev(flat))
    with pytest.raises(ValueError, match='level 0 .*channel 1 of the generated set'):
        sw.finalize()


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------
def test_evaluate_swd_with_a_generator_that_returns_the_reals(K, capsys):
    """A model stub whose generate_batch returns the batch's real images.  The centre tables of the real and of the generated set
    are separate draws (evaluation/swd.py), so they do NOT coincide: the levels are finite and positive, not 0 — two samples of
    patches of one image set.  Two runs give the same bits."""
    from t2i_amd.evaluation.evaluator import GeneratorEval
    from t2i_amd.utils.config import AttrDict
    store = torch.from_numpy(np.concatenate([SC.images(60 + i, 4, 32, 32, 3) for i in range(3)])).cuda()

    class Split(object):
        def __init__(self):
            self.at, self.last = 0, None

        def next_batch(self, bs, k, embeddings=True):
            self.last = store[self.at:self.at + bs]
            self.at = (self.at + bs) % store.shape[0]
            return self.last, None, np.zeros((bs, 8), np.float32), None, None

    class Data(object):
        pass

    class Model(object):
        device, z_dim, embed_dim = torch.device('cuda'), 4, 8

    class Ev(GeneratorEval):
        def restore(self):
            self.restored = True

        def generate_batch(self, z, cond, is_training):
            assert not is_training
            return self.dataset.test.last.clone()

    def run():
        data = Data()
        data.test = Split()
        ev = Ev(None, Model(), data, AttrDict({'EVAL': {'SIZE': 13, 'SAMPLE_SIZE': 4, 'INCEP_BATCH_SIZE': 4}}))
        np.random.seed(5)
        out = ev.evaluate_swd()
        assert ev.restored
        return out

    a = run()
    text = capsys.readouterr().out
    b = run()
    assert a == b                                          # bitwise: the dict holds Python floats
    assert a['sides'] == [32, 16] and len(a['levels']) == 2 and all(np.isfinite(v) and v > 0 for v in a['levels'])
    assert a['mean'] == pytest.approx(np.mean(a['levels']), rel=1e-15)
    assert text.count('SWD x 1e3 |') == 3 and 'mean: %.4f' % a['mean'] in text
