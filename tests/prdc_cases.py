"""Precision, recall, density and coverage restated in numpy float64, and the inputs of tests/test_prdc_host.py and
tests/test_prdc_gpu.py.

The restatement forms every squared distance in the DIRECT form sum((a - b)^2) in float64 (the kernel uses the Gram form
|a|^2 + |b|^2 - 2 a.b in fp64), sorts with np.sort for the radii and applies the four definitions of evaluation/prdc.py.

band(a, b) = 4 D 2^-53 (|a|^2 + |b|^2) bounds the distance between an fp64 Gram form and the true d2: each of its three fp64 sums
errs by at most D 2^-53 of its absolute terms, the dot's absolute terms are at most (|a|^2 + |b|^2) / 2, so the total is
2 D 2^-53 (|a|^2 + |b|^2); the rest is headroom for the final additions.  The tests demand EQUALITY of every count and metric, which
holds when no decision (d2 <= r2, dmin <= r2) of the restatement lies within 2 bands of its threshold: decision_margin() measures
that on the inputs, and a shape that violates it is a bad input, not a tolerance to widen."""
import functools

import numpy as np

SHAPES = [(1, 2, 1, 1), (5, 7, 3, 1), (64, 64, 4, 3), (65, 130, 36, 3), (129, 300, 100, 5), (200, 200, 64, 8), (100, 257, 2048, 5)]


def seed_of(M, N):
    return 1000 * M + N


def latent(M, N, D, seed):
    """-> (R [N, D], G [M, D]) float32: an 8-dimensional latent mapped into D dimensions plus noise; the generated set is narrower
    and shifted, so that precision is high and recall is not."""
    rs = np.random.RandomState(seed)
    W = rs.randn(8, D) / np.sqrt(8)
    R = rs.randn(N, 8) @ W + 0.05 * rs.randn(N, D)
    G = (0.8 * rs.randn(M, 8) + 0.3) @ W + 0.05 * rs.randn(M, D)
    return R.astype(np.float32), G.astype(np.float32)


def integer_sets(M, N, D):
    """Integer-valued features with an asymmetric pattern: every d2 is an exact integer in any form. -> (Q [M, D], R [N, D])."""
    m, n, d = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(D)[None, :]
    return ((3 * m + d) % 7).astype(np.float32), ((5 * n + 2 * d) % 11).astype(np.float32)


def dist2(A, B):
    """float64 [len(A), len(B)], direct form, row by row."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        diff = B - A[i]
        out[i] = (diff * diff).sum(1)
    return out


def gram_dist2(A, B):
    """The Gram form in numpy float64 (what the kernel computes, in another summation order)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T), 0.0)


def band(A, B):
    """float64 [len(A), len(B)]"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return 4.0 * A.shape[1] * 2.0 ** -53 * ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :])


def knn(A, B, k, exclude_self=False, d=None):
    """-> (values float64 [len(A), k] ascending, their candidate indices).  exclude_self removes candidate i of query i by index."""
    d = np.array(dist2(A, B) if d is None else d)
    if exclude_self:
        assert d.shape[0] == d.shape[1]
        d[np.arange(d.shape[0]), np.arange(d.shape[0])] = np.inf
    idx = np.argsort(d, axis=1, kind='stable')[:, :k]
    val = np.take_along_axis(d, idx, 1)
    assert np.array_equal(val, np.sort(d, axis=1)[:, :k])
    return val, idx


def restate(R, G, k):
    """Every intermediate of the metric: dict(d_gr [M, N], r2_real [N], r2_gen [M], cnt_gen [M], cnt_real [N], dmin_gen [M],
    dmin_real [N], covered [N], precision, recall, density, coverage)."""
    M, N = G.shape[0], R.shape[0]
    d_gr = dist2(G, R)
    r2_real = knn(R, R, k, True)[0][:, k - 1]
    r2_gen = knn(G, G, k, True)[0][:, k - 1] if M > k else np.full(M, np.nan)
    cnt_gen = (d_gr <= r2_real[None, :]).sum(1)
    cnt_real = (d_gr.T <= r2_gen[None, :]).sum(1)
    dmin_real = d_gr.min(0)
    covered = dmin_real <= r2_real
    return dict(d_gr=d_gr, r2_real=r2_real, r2_gen=r2_gen, cnt_gen=cnt_gen, cnt_real=cnt_real, dmin_gen=d_gr.min(1), dmin_real=dmin_real,
                covered=covered, precision=int((cnt_gen > 0).sum()) / M, recall=int((cnt_real > 0).sum()) / N,
                density=int(cnt_gen.sum()) / (k * M), coverage=int(covered.sum()) / N, nearest_k=k, n_real=N, n_gen=M)


def decision_margin(R, G, k, ref=None):
    """The smallest |d2 - threshold| / band over every decision of the restatement: d2(G_m, R_n) against r2_real[n] and (when the
    generated set has radii) against r2_gen[m], and dmin_real[n] against r2_real[n]."""
    ref = ref or restate(R, G, k)
    b = band(G, R)
    worst = (np.abs(ref['d_gr'] - ref['r2_real'][None, :]) / b).min()
    if G.shape[0] > k:
        worst = min(worst, (np.abs(ref['d_gr'] - ref['r2_gen'][:, None]) / b).min())
    arg = ref['d_gr'].argmin(0)
    worst = min(worst, (np.abs(ref['dmin_real'] - ref['r2_real']) / b[arg, np.arange(R.shape[0])]).min())
    return float(worst)


@functools.lru_cache(maxsize=None)
def case(M, N, D, k):
    """(R, G, restatement) of one shape, computed once and shared; leave it unchanged."""
    R, G = latent(M, N, D, seed_of(M, N))
    return R, G, restate(R, G, k)


def duplicates():
    """latent(40, 60, 48, 7) with R[30:] = R[:30] and G[:10] = R[:10]: every real row has a copy, ten generated rows are real rows."""
    R, G = latent(40, 60, 48, 7)
    R, G = R.copy(), G.copy()
    R[30:] = R[:30]
    G[:10] = R[:10]
    return R, G
