"""The Kernel Inception distance (KID) of a generated set against a real set in Inception feature space: the unbiased estimate of the
squared maximum mean discrepancy with the polynomial kernel k(a, b) = (a.b / dim + 1)^3 of Binkowski et al. 2018 ("Demystifying MMD
GANs"), the distance that limited-data GAN work reports where the test split has a few thousand images and FID is biased.  The
reference has no such metric.  With a subset of m rows x_i of the real features and m rows y_j of the generated ones,

    mmd2 = 2 P_xx / (m (m - 1)) + 2 P_yy / (m (m - 1)) - 2 S_xy / m^2,
    P_xx = sum_{i<j} k(x_i, x_j),   P_yy likewise,   S_xy = sum_{i,j} k(x_i, y_j)            (i, j positions in the subset)

and KID is the mean of mmd2 over `num_subsets` subsets drawn without replacement; its standard deviation over the subsets (ddof 0) is
reported with it.  The estimate is unbiased, so it may be negative; it is reported as it is.  The defaults are the published ones
(StyleGAN2-ADA, torch-fidelity): 100 subsets of min(n_real, n_gen, 1000) rows, degree 3, gamma 1 / dim, coef0 1.

One pass of csrc/t2i_mmd.hip (K.poly_mmd_sums) forms the three sums of every subset in fp64 from the rows in place: no m x m matrix
and no gathered subset is written.  The estimates are formed on the host in float64."""
import numpy as np
import torch

from .. import kernels as K
from .prdc import _Rows

MAX_SUBSETS = 10000


def subset_tables(rs, n_real, n_gen, num_subsets, m):
    """-> (ix, iy) int32 [num_subsets, m]: per subset rs.choice(n_real, m, replace=False), then rs.choice(n_gen, m, replace=False)."""
    ix, iy = np.empty((num_subsets, m), np.int32), np.empty((num_subsets, m), np.int32)
    for s in range(num_subsets):
        ix[s] = rs.choice(n_real, m, replace=False)
        iy[s] = rs.choice(n_gen, m, replace=False)
    return ix, iy


def estimates(sums, m):
    """The per-subset mmd2 (float64 [S]) from host sums [S, 3] = (P_xx, P_yy, S_xy)."""
    sums = np.asarray(sums, np.float64)
    return 2.0 * sums[:, 0] / (m * (m - 1)) + 2.0 * sums[:, 1] / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)


class KernelDistance(object):
    def __init__(self, dim, device, num_subsets=100, max_subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0):
        if int(dim) < 1:
            raise ValueError('KernelDistance: dim must be positive, got %r' % (dim,))
        if int(num_subsets) != num_subsets or not 1 <= int(num_subsets) <= MAX_SUBSETS:
            raise ValueError('KernelDistance: num_subsets must be in 1..%d, got %r' % (MAX_SUBSETS, num_subsets))
        if int(max_subset_size) != max_subset_size or int(max_subset_size) < 2:
            raise ValueError('KernelDistance: max_subset_size must be at least 2, got %r' % (max_subset_size,))
        if int(degree) != degree or not 1 <= int(degree) <= K.MMD_MAX_DEGREE:
            raise ValueError('KernelDistance: degree must be in 1..%d, got %r' % (K.MMD_MAX_DEGREE, degree))
        gamma = 1.0 / int(dim) if gamma is None else float(gamma)
        if not (np.isfinite(gamma) and np.isfinite(float(coef0))):
            raise ValueError('KernelDistance: gamma and coef0 must be finite, got %r and %r' % (gamma, coef0))
        self.dim, self.device = int(dim), torch.device(device)
        self.num_subsets, self.max_subset_size, self.seed = int(num_subsets), int(max_subset_size), int(seed)
        self.degree, self.gamma, self.coef0 = int(degree), gamma, float(coef0)
        self.real, self.gen = _Rows(self.dim, self.device, 'KernelDistance'), _Rows(self.dim, self.device, 'KernelDistance')

    def add_real(self, feat):
        self.real.add(feat, 'add_real')

    def add_gen(self, feat):
        self.gen.add(feat, 'add_gen')

    def tables(self):
        """-> (ix, iy, m): the host index tables of finalize(), from a private RandomState(seed); the global stream is not touched."""
        m = min(self.real.n, self.gen.n, self.max_subset_size)
        ix, iy = subset_tables(np.random.RandomState(self.seed), self.real.n, self.gen.n, self.num_subsets, m)
        return ix, iy, m

    def finalize(self):
        """-> dict(kid, kid_std, subsets, subset_size, n_real, n_gen, degree, gamma, coef0)."""
        for name, rows in (('real', self.real), ('generated', self.gen)):
            if rows.n < 2:
                raise ValueError('KernelDistance.finalize: %d %s rows, the estimate needs at least 2' % (rows.n, name))
            if not bool(torch.isfinite(rows.rows()).all()):
                raise ValueError('KernelDistance.finalize: a %s feature is not finite' % name)
        ix, iy, m = self.tables()
        sums = K.poly_mmd_sums(self.real.rows(), self.gen.rows(), torch.from_numpy(ix).to(self.device), torch.from_numpy(iy).to(self.device),
                               degree=self.degree, gamma=self.gamma, coef0=self.coef0, check_indices=False)      # (the tables are ours)
        mmd2 = estimates(sums.cpu().numpy(), m)
        return dict(kid=float(np.mean(mmd2)), kid_std=float(np.std(mmd2)), subsets=self.num_subsets, subset_size=m, n_real=self.real.n,
                    n_gen=self.gen.n, degree=self.degree, gamma=self.gamma, coef0=self.coef0)
