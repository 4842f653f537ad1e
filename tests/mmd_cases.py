"""The polynomial-kernel MMD^2 (Kernel Inception distance) restated in numpy float64, its error band, and the inputs of
tests/test_mmd_host.py and tests/test_mmd_gpu.py.

Restatement: per subset gather the rows, t = gamma (A @ B^T) + coef0, k = t multiplied degree - 1 times by t, then
P_xx = sum over positions i < j of k(x_i, x_j), P_yy likewise, S_xy = sum over all (i, j) of k(x_i, y_j), and
mmd2 = 2 P_xx / (m (m - 1)) + 2 P_yy / (m (m - 1)) - 2 S_xy / m^2.

Band (derived, not tuned; u = 2^-53, p = degree).  The inputs are fp32, so every product a_d b_d is exact in fp64.
  - A D-term fp64 dot product in any order errs by at most D u sum_d |a_d b_d| (first order).
  - t = fma(gamma, dot, coef0) multiplies that by |gamma| and adds one rounding: with T = |gamma| sum_d |a_d||b_d| + |coef0| >= |t|,
    |t_computed - t| <= (D + 1) u T.  (A restatement that rounds gamma * dot and the sum separately has D + 2 here.)
  - k = t^p by p - 1 multiplications: the relative error of t enters p times, each multiplication adds u:
    |k_computed - k| <= (p (D + 2) + p - 1) u T^p <= p (D + p + 2) u T^p for p >= 1.
  - Adding n such terms in any order adds at most n u sum |k|  <= n u sum T^p.
  band = u (p (D + p + 2) + n) sum_ij T_ij^p over the terms of the sum, n their number: the constant of the issue, re-derived.
The kernel and the restatement are each within one band of the true sum, so |kernel - restatement| <= 2 band.  The band of mmd2 is
the same linear combination of the three bands, that of the mean over subsets their mean; for the standard deviation over subsets
|std(a) - std(b)| <= max_s |a_s - b_s| (std is 1-Lipschitz in the maximum norm), so its band is the largest mmd2 band."""
import functools

import numpy as np

from prdc_cases import integer_sets, latent  # noqa: F401  (the tests take both from here)

U = 2.0 ** -53

SHAPES = [(2, 2, 1, 1, 2), (7, 5, 3, 2, 3), (70, 90, 36, 3, 64), (130, 129, 100, 4, 65), (300, 257, 2048, 3, 129), (200, 200, 64, 5, 200)]
INTEGER_SHAPES = [(35, 17, 4), (16, 16, 5), (130, 70, 9)]


def seed_of(NX, NY):
    return 1000 * NX + NY + 17


def sets(NX, NY, D):
    """-> (X [NX, D], Y [NY, D]) float32: prdc_cases.latent's real and generated sets."""
    X, Y = latent(NY, NX, D, seed_of(NX, NY))
    return X, Y


def tables(NX, NY, S, m, seed=0):
    """The index tables of evaluation/mmd.py: per subset choice(NX, m, replace=False), then choice(NY, m, replace=False)."""
    rs = np.random.RandomState(seed)
    ix, iy = np.empty((S, m), np.int32), np.empty((S, m), np.int32)
    for s in range(S):
        ix[s] = rs.choice(NX, m, replace=False)
        iy[s] = rs.choice(NY, m, replace=False)
    return ix, iy


def kernel_matrix(A, B, degree, gamma, coef0, dtype=np.float64):
    A, B = np.asarray(A, dtype), np.asarray(B, dtype)
    t = dtype(gamma) * (A @ B.T) + dtype(coef0)
    k = t.copy()
    for _ in range(degree - 1):
        k = k * t
    return k


def bound_matrix(A, B, degree, gamma, coef0):
    """T_ij^p, T_ij = |gamma| sum_d |a_d||b_d| + |coef0|."""
    T = abs(gamma) * (np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(B, np.float64)).T) + abs(coef0)
    return T ** degree


def sums(X, Y, ix, iy, degree=3, gamma=None, coef0=1.0, dtype=np.float64, upper=None):
    """-> [S, 3] (P_xx, P_yy, S_xy).  `upper`: the mask of the pairs of a symmetric product (default i < j by position)."""
    D = X.shape[1]
    gamma = 1.0 / D if gamma is None else gamma
    S, m = ix.shape
    up = np.triu(np.ones((m, m), bool), 1) if upper is None else upper
    out = np.empty((S, 3), dtype)
    for s in range(S):
        A, B = X[ix[s]], Y[iy[s]]
        out[s, 0] = kernel_matrix(A, A, degree, gamma, coef0, dtype)[up].sum()
        out[s, 1] = kernel_matrix(B, B, degree, gamma, coef0, dtype)[up].sum()
        out[s, 2] = kernel_matrix(A, B, degree, gamma, coef0, dtype).sum()
    return out


def bands(X, Y, ix, iy, degree=3, gamma=None, coef0=1.0):
    """-> [S, 3]: the band of each sum."""
    D = X.shape[1]
    gamma = 1.0 / D if gamma is None else gamma
    S, m = ix.shape
    up = np.triu(np.ones((m, m), bool), 1)
    out = np.empty((S, 3))
    for s in range(S):
        A, B = X[ix[s]], Y[iy[s]]
        for c, (P, Q, mask, n) in enumerate(((A, A, up, m * (m - 1) // 2), (B, B, up, m * (m - 1) // 2), (A, B, slice(None), m * m))):
            out[s, c] = U * (degree * (D + degree + 2) + n) * bound_matrix(P, Q, degree, gamma, coef0)[mask].sum()
    return out


def weights(m):
    """mmd2 = sums @ weights(m)."""
    return np.array([2.0 / (m * (m - 1)), 2.0 / (m * (m - 1)), -2.0 / (m * m)])


def mmd2(sums_, m):
    return np.asarray(sums_, np.float64) @ weights(m)


def mmd2_band(bands_, m):
    return np.asarray(bands_) @ np.abs(weights(m))


def published(X, Y, ix, iy):
    """The estimate as StyleGAN2-ADA's metrics/kernel_inception_distance.py writes it (degree 3, gamma 1 / D, coef0 1): per subset
    a = k(x, x) + k(y, y), b = k(x, y), t += (a.sum() - trace(a)) / (m - 1) - 2 b.sum() / m; KID = t / S / m."""
    S, m = ix.shape
    D = X.shape[1]
    t = 0.0
    for s in range(S):
        x, y = X[ix[s]].astype(np.float64), Y[iy[s]].astype(np.float64)
        a = (x @ x.T / D + 1) ** 3 + (y @ y.T / D + 1) ** 3
        b = (x @ y.T / D + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
    return t / S / m


@functools.lru_cache(maxsize=None)
def case(NX, NY, D, S, m):
    """(X, Y, ix, iy, sums, bands) of one shape at the default kernel, computed once and shared; leave it unchanged."""
    X, Y = sets(NX, NY, D)
    ix, iy = tables(NX, NY, S, m)
    return X, Y, ix, iy, sums(X, Y, ix, iy), bands(X, Y, ix, iy)
