"""The Kernel Inception distance on the GPU: t2i_poly_mmd_sums (csrc/t2i_mmd.hip) against the float64 restatement of
tests/mmd_cases.py, KernelDistance end to end, and GeneratorEval.evaluate_mmd.

Every sum is compared within 2 band (mmd_cases.bands: one band for the kernel's fp64 arithmetic, one for the restatement's own
rounding; the derivation is in mmd_cases.py), the estimates within the same bands propagated linearly; integer-valued inputs must
be EQUAL.

Measured on an MI355X (largest |kernel - restatement| over the three sums and the subsets): 0.0219 band on (7, 5, 3, 2, 3),
3.8e-5 band at D = 2048, at most 7.1e-4 band over the other kernels; DESIGN 4.38 has the list."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import mmd_cases as MC  # noqa: E402
from test_prdc_gpu import _evaluator, _shifted  # noqa: E402  (the stubs of the evaluate_prdc test)

pytestmark = pytest.mark.gpu

IDS = dict(ids=lambda s: 'x'.join(str(v) for v in s))


@pytest.fixture(scope='module')
def K():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def twice(K, x, y, ix, iy, **kw):
    """The kernel called twice: the same bits. -> host float64 [S, 3]"""
    a = K.poly_mmd_sums(x, y, ix, iy, **kw)
    b = K.poly_mmd_sums(x, y, ix, iy, **kw)
    assert a.dtype == torch.float64 and tuple(a.shape) == (ix.shape[0], 3) and torch.equal(a, b)
    return a.cpu().numpy()


def within(got, want, band, what):
    ratio = np.abs(got - want) / band
    print('%s: largest |kernel - restatement| = %.3g band' % (what, float(ratio.max())))
    assert np.all(np.isfinite(got)) and np.all(ratio <= 2.0), (what, float(ratio.max()))


# ---- 1. the sums -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', MC.SHAPES, **IDS)
def test_sums_within_two_bands_of_the_restatement(K, shape):
    X, Y, ix, iy, ref, band = MC.case(*shape)
    within(twice(K, dev(X), dev(Y), dev(ix), dev(iy)), ref, band, shape)


@pytest.mark.parametrize('kernel', [dict(degree=1), dict(degree=2), dict(gamma=0.37), dict(coef0=0.0), dict(coef0=-0.5)],
                         ids=lambda k: '%s=%s' % tuple(k.items())[0])
def test_other_kernels_within_two_bands(K, kernel):
    for shape in ((70, 90, 36, 3, 64), (130, 129, 100, 4, 65)):
        X, Y, ix, iy, _, _ = MC.case(*shape)
        got = twice(K, dev(X), dev(Y), dev(ix), dev(iy), **kernel)
        within(got, MC.sums(X, Y, ix, iy, **kernel), MC.bands(X, Y, ix, iy, **kernel), (shape, kernel))


def test_one_tensor_as_both_sets(K):
    X, _, ix, _, _, _ = MC.case(130, 129, 100, 4, 65)
    iy = MC.tables(130, 130, 4, 65, seed=5)[1]
    x = dev(X)
    got = twice(K, x, x, dev(ix), dev(iy))
    within(got, MC.sums(X, X, ix, iy), MC.bands(X, X, ix, iy), 'X is Y')


def test_a_misaligned_base_takes_the_scalar_loads_to_the_same_bits(K):
    """D % 4 == 0, but the features start one float into their buffer: no float4 load is possible; the arithmetic is the same."""
    X, Y, ix, iy, ref, band = MC.case(130, 129, 100, 4, 65)
    aligned = twice(K, dev(X), dev(Y), dev(ix), dev(iy))
    bx = torch.empty(X.size + 1, dtype=torch.float32, device='cuda')
    by = torch.empty(Y.size + 1, dtype=torch.float32, device='cuda')
    x, y = bx[1:].view(X.shape), by[1:].view(Y.shape)
    x.copy_(dev(X))
    y.copy_(dev(Y))
    assert x.data_ptr() % 16 == 4 and y.data_ptr() % 16 == 4 and x.is_contiguous()
    assert np.array_equal(twice(K, x, y, dev(ix), dev(iy)), aligned)
    assert np.array_equal(twice(K, x, dev(Y), dev(ix), dev(iy)), aligned)          # one misaligned set is enough for the scalar path


@pytest.mark.parametrize('shape', MC.INTEGER_SHAPES, **IDS)
def test_integer_features_are_exact(K, shape):
    """Integer-valued features with an asymmetric pattern, gamma = coef0 = 1, degree 3: every k and every sum is an exact integer
    below 2^53 in any order, so the kernel must EQUAL the restatement.  A wrong f64 accumulator map, a swapped operand, a mishandled
    tail in D or m, an unmasked padded row (k = 1) or a wrong diagonal cannot pass."""
    NX, NY, D = shape
    X, Y = MC.integer_sets(NX, NY, D)
    m = min(NX, NY)
    ix, iy = MC.tables(NX, NY, 3, m, seed=2)
    want = MC.sums(X, Y, ix, iy, degree=3, gamma=1.0, coef0=1.0)
    assert np.array_equal(want, np.round(want)) and want.max() < 2.0 ** 53
    assert float(MC.bound_matrix(X, Y, 3, 1.0, 1.0).sum()) < 2.0 ** 53
    assert np.array_equal(twice(K, dev(X), dev(Y), dev(ix), dev(iy), degree=3, gamma=1.0, coef0=1.0), want)


# ---- 2. positions and the index guard ----------------------------------------------------------------------------------------------
def test_pairs_are_positions_not_values(K):
    """A table that names one row twice: the pair of the two copies counts (k(x, x) of that row), a position with itself does not."""
    X, Y, ix, iy, _, _ = MC.case(130, 129, 100, 4, 65)
    ix = ix.copy()
    ix[1, 40] = ix[1, 3]
    ix[2, 64] = ix[2, 0]                                                          # across the two row tiles
    want, band = MC.sums(X, Y, ix, iy), MC.bands(X, Y, ix, iy)
    self_k = (np.float64(1.0 / 100) * (X[ix[1, 3]].astype(np.float64) ** 2).sum() + 1.0) ** 3
    assert self_k > 1e6 * band[1, 0]                                              # dropping the pair of the copies would show
    within(twice(K, dev(X), dev(Y), dev(ix), dev(iy), check_indices=False), want, band, 'a row twice')


def test_an_index_out_of_range_is_not_dereferenced(K):
    """X is the first NX rows of a buffer with 8 spare rows (even a wrong guard reads allocated memory); one entry of subset 1 names
    row NX.  That subset's P_xx and S_xy are NaN, every other sum has the bits of the clean call; check_indices=True raises."""
    NX, NY, D, S, m = 130, 129, 100, 4, 65
    X, Y, ix, iy, _, _ = MC.case(NX, NY, D, S, m)
    buf = torch.zeros((NX + 8, D), dtype=torch.float32, device='cuda')
    buf[:NX] = dev(X)
    x, y = buf[:NX], dev(Y)
    clean = twice(K, x, y, dev(ix), dev(iy))
    for value in (NX, -1):
        bad = ix.copy()
        bad[1, 17] = value
        got = twice_nan(K, x, y, dev(bad), dev(iy))
        assert np.isnan(got[1, 0]) and np.isnan(got[1, 2])
        keep = np.ones((S, 3), bool)
        keep[1, 0] = keep[1, 2] = False
        assert np.array_equal(got[keep], clean[keep])
        with pytest.raises(ValueError, match='ix holds indices'):
            K.poly_mmd_sums(x, y, dev(bad), dev(iy))
    bad = iy.copy()
    bad[3, 64] = NY
    with pytest.raises(ValueError, match='iy holds indices'):
        K.poly_mmd_sums(x, y, dev(ix), dev(bad), check_indices=True)


def twice_nan(K, x, y, ix, iy):
    a = K.poly_mmd_sums(x, y, ix, iy, check_indices=False).cpu().numpy()
    b = K.poly_mmd_sums(x, y, ix, iy, check_indices=False).cpu().numpy()
    assert np.array_equal(a, b, equal_nan=True)
    return a


# ---- 3. KernelDistance -------------------------------------------------------------------------------------------------------------
def feed(kd, X, Y):
    for a, b in ((0, 1), (1, X.shape[0] // 3), (X.shape[0] // 3, X.shape[0])):
        kd.add_real(dev(X[a:b]))
    for a, b in ((0, Y.shape[0] // 2 + 3), (Y.shape[0] // 2 + 3, Y.shape[0] - 1), (Y.shape[0] - 1, Y.shape[0])):
        kd.add_gen(dev(Y[a:b]))
    return kd


@pytest.mark.parametrize('shape', [(130, 129, 100), (300, 257, 2048)], **IDS)
def test_kernel_distance_within_the_propagated_band(K, shape):
    from t2i_amd.evaluation.mmd import KernelDistance
    NX, NY, D = shape
    S = 4
    X, Y = MC.sets(NX, NY, D)
    kd = feed(KernelDistance(D, 'cuda', num_subsets=S), X, Y)
    out = kd.finalize()
    m = min(NX, NY)
    ix, iy = MC.tables(NX, NY, S, m)
    est, eb = MC.mmd2(MC.sums(X, Y, ix, iy), m), MC.mmd2_band(MC.bands(X, Y, ix, iy), m)
    print('%s: KID %.6g +- %.3g, |kid - restatement| = %.3g band, std %.3g band' % (
        shape, out['kid'], out['kid_std'], abs(out['kid'] - est.mean()) / eb.mean(), abs(out['kid_std'] - est.std()) / eb.max()))
    assert abs(out['kid'] - est.mean()) <= 2.0 * eb.mean()
    assert abs(out['kid_std'] - est.std()) <= 2.0 * eb.max()
    assert {k: out[k] for k in ('subsets', 'subset_size', 'n_real', 'n_gen', 'degree', 'gamma', 'coef0')} == dict(
        subsets=S, subset_size=m, n_real=NX, n_gen=NY, degree=3, gamma=1.0 / D, coef0=1.0)
    assert type(out['kid']) is float and type(out['kid_std']) is float
    assert kd.finalize() == out                                                   # the same bits


def test_kernel_distance_of_a_set_against_itself(K):
    """Y = X and one table for both sets: mmd2 = 2 (2 P / (m (m - 1))) - 2 S_xy / m^2 of the restatement, within the band."""
    from t2i_amd.evaluation import mmd
    X, _ = MC.sets(130, 129, 100)
    S, m = 4, 130
    ix, _ = MC.tables(130, 130, S, m)
    x = dev(X)
    sums = twice(K, x, x, dev(ix), dev(ix))
    assert np.array_equal(sums[:, 0], sums[:, 1])                                 # the same pairs in the same order
    got = mmd.estimates(sums, m)
    ref, band = MC.sums(X, X, ix, ix), MC.bands(X, X, ix, ix)
    want = 2.0 * (2.0 * ref[:, 0] / (m * (m - 1))) - 2.0 * ref[:, 2] / (m * m)
    assert got.shape == (S,) and np.all(np.abs(got - want) <= 2.0 * MC.mmd2_band(band, m))


# ---- 4. graph capture --------------------------------------------------------------------------------------------------------------
def test_the_two_launches_replay_from_a_graph(K):
    """poly_mmd_sums only enqueues work: captured once, replayed on fresh inputs of the same shape, it equals the eager call."""
    shape = (130, 129, 100, 4, 65)
    X, Y, ix, iy, ref, band = MC.case(*shape)
    X2, Y2 = MC.latent(129, 130, 100, 77)
    ix2, iy2 = MC.tables(130, 129, 4, 65, seed=9)
    x, y, tx, ty = dev(X2), dev(Y2), dev(ix2), dev(iy2)
    eager2 = K.poly_mmd_sums(x, y, tx, ty).clone()                                # (the workspace exists before the capture)
    eager1 = K.poly_mmd_sums(dev(X), dev(Y), dev(ix), dev(iy)).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = K.poly_mmd_sums(x, y, tx, ty, check_indices=False)
    for t, a in ((x, X), (y, Y), (tx, ix), (ty, iy)):
        t.copy_(dev(a))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager1)
    within(out.cpu().numpy(), ref, band, 'replay')
    for t, a in ((x, X2), (y, Y2), (tx, ix2), (ty, iy2)):
        t.copy_(dev(a))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2)


# ---- 5. the evaluator ----------------------------------------------------------------------------------------------------------------
def test_evaluate_mmd_against_kernel_distance_on_its_features(K, capsys):
    """A store of 12 images, batches of 4, SIZE 22: five batches, of which only the first three (one epoch) feed the real set."""
    from t2i_amd.evaluation.mmd import KernelDistance

    def run():
        ev = _evaluator(_shifted)
        np.random.seed(5)
        out = ev.evaluate_mmd(num_subsets=6, max_subset_size=10, keep_features=True)
        assert ev.restored
        return out, np.random.get_state()

    a, state_a = run()
    text = capsys.readouterr().out
    b, _ = run()
    assert a['n_real'] == 12 and a['n_gen'] == 20 and a['subsets'] == 6 and a['subset_size'] == 10
    assert a['real_features'].shape == (12, 64) and a['gen_features'].shape == (20, 64) and a['real_features'].dtype == np.float32
    assert a['kid'] == b['kid'] and a['kid_std'] == b['kid_std'] and np.array_equal(a['real_features'], b['real_features'])
    assert np.array_equal(a['gen_features'], b['gen_features'])
    kd = KernelDistance(64, 'cuda', num_subsets=6, max_subset_size=10)
    kd.add_real(dev(a['real_features']))
    kd.add_gen(dev(a['gen_features']))
    assert kd.finalize() == {k: v for k, v in a.items() if k not in ('real_features', 'gen_features')}
    ix, iy = MC.tables(12, 20, 6, 10)
    est = MC.mmd2(MC.sums(a['real_features'], a['gen_features'], ix, iy), 10)
    eb = MC.mmd2_band(MC.bands(a['real_features'], a['gen_features'], ix, iy), 10)
    assert abs(a['kid'] - est.mean()) <= 2.0 * eb.mean() and abs(a['kid_std'] - est.std()) <= 2.0 * eb.max()
    line = 'KID x 1e3 (--eval mmd) | mean: %.4f std: %.4f | 6 subsets of 10 | 12 real, 20 generated' % (1e3 * a['kid'], 1e3 * a['kid_std'])
    assert text.count('KID x 1e3') == 1 and line in text
    assert ev_default_subset_size() == 12

    ev = _evaluator(_shifted)                              # the global numpy stream: that of evaluate_imd on the same setup
    np.random.seed(5)
    ev.evaluate_imd()
    state_imd = np.random.get_state()
    assert state_a[0] == state_imd[0] and np.array_equal(state_a[1], state_imd[1]) and state_a[2:] == state_imd[2:]


def ev_default_subset_size():
    """The defaults: m = min(n_real, n_gen, 1000)."""
    ev = _evaluator(_shifted)
    np.random.seed(5)
    out = ev.evaluate_mmd(num_subsets=2)
    assert out['subsets'] == 2
    return out['subset_size']
