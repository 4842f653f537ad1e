"""Precision, recall, density and coverage of a generated set against a real set in Inception feature space: the k-nearest-neighbour
manifold estimates of Kynkaanniemi et al. 2019 ("Improved precision and recall metric for assessing generative models") and their
outlier-robust variants of Naeem et al. 2020 ("Reliable fidelity and diversity metrics for generative models", the `prdc` package).
The reference has no such metric.  With R the real features [N, dim], G the generated ones [M, dim], d2 the squared Euclidean distance
and r2_X[i] the squared distance from X[i] to its k-th nearest OTHER row of X:

    precision = mean_m [ exists n: d2(G_m, R_n) <= r2_R[n] ]          recall   = mean_n [ exists m: d2(R_n, G_m) <= r2_G[m] ]
    density   = sum_m #{n: d2(G_m, R_n) <= r2_R[n]} / (k M)           coverage = mean_n [ min_m d2(R_n, G_m) <= r2_R[n] ]

Four passes of csrc/t2i_knn.hip (K.knn_dist2 twice, K.ball_counts twice): every distance is formed in fp64 and no N x M matrix is
written.  The ratios are formed on the host from integer counts.  nearest_k = 5 is the prdc package's default for all four numbers;
nearest_k = 3 reproduces the precision and recall of Kynkaanniemi et al."""
import numpy as np
import torch

from .. import kernels as K


def manifold_passes(real, gen, nearest_k):
    """The four kernel passes on device tensors real [N, dim] and gen [M, dim] (float32, contiguous): -> (cnt_gen int32 [M],
    cnt_real int32 [N], covered bool [N]) on the device.  Only enqueues work: the chain can be captured in a graph."""
    k = int(nearest_k)
    r2_real = K.knn_dist2(real, real, k, exclude_self=True)[:, k - 1].contiguous()
    r2_gen = K.knn_dist2(gen, gen, k, exclude_self=True)[:, k - 1].contiguous()
    cnt_gen, _ = K.ball_counts(gen, real, r2_real)
    cnt_real, dmin_real = K.ball_counts(real, gen, r2_gen)
    return cnt_gen, cnt_real, dmin_real <= r2_real


def ratios(cnt_gen, cnt_real, covered, nearest_k):
    """The four numbers from host integer / bool arrays."""
    cnt_gen, cnt_real, covered = np.asarray(cnt_gen), np.asarray(cnt_real), np.asarray(covered)
    M, N = cnt_gen.shape[0], cnt_real.shape[0]
    return dict(precision=int(np.count_nonzero(cnt_gen > 0)) / M, recall=int(np.count_nonzero(cnt_real > 0)) / N,
                density=int(cnt_gen.astype(np.int64).sum()) / (int(nearest_k) * M), coverage=int(np.count_nonzero(covered)) / N,
                nearest_k=int(nearest_k), n_real=N, n_gen=M)


class _Rows(object):
    """[n, dim] float32 rows on the device; the buffer doubles when it is full."""

    def __init__(self, dim, device, owner='ManifoldMetrics'):
        self.dim, self.device, self.n, self.buf, self.owner = dim, device, 0, None, owner

    def add(self, feat, name):
        if feat.dim() != 2 or feat.shape[1] != self.dim:
            raise ValueError('%s.%s: features must be [n, %d], got %s' % (self.owner, name, self.dim, tuple(feat.shape)))
        feat = feat.detach().to(device=self.device, dtype=torch.float32)
        need = self.n + feat.shape[0]
        if self.buf is None or need > self.buf.shape[0]:
            grown = torch.empty((max(need, 2 * (0 if self.buf is None else self.buf.shape[0]), 256), self.dim), dtype=torch.float32,
                                device=self.device)
            if self.n:
                grown[:self.n] = self.buf[:self.n]
            self.buf = grown
        self.buf[self.n:need] = feat
        self.n = need

    def rows(self):
        return self.buf[:self.n]                          # (the leading rows of a contiguous buffer are contiguous)


class ManifoldMetrics(object):
    def __init__(self, dim, device, nearest_k=5):
        if int(nearest_k) != nearest_k or not 1 <= int(nearest_k) <= K.KNN_MAX_K:
            raise ValueError('ManifoldMetrics: nearest_k must be in 1..%d, got %r' % (K.KNN_MAX_K, nearest_k))
        if int(dim) < 1:
            raise ValueError('ManifoldMetrics: dim must be positive, got %r' % (dim,))
        self.dim, self.device, self.nearest_k = int(dim), torch.device(device), int(nearest_k)
        self.real, self.gen = _Rows(self.dim, self.device), _Rows(self.dim, self.device)

    def add_real(self, feat):
        self.real.add(feat, 'add_real')

    def add_gen(self, feat):
        self.gen.add(feat, 'add_gen')

    def finalize(self):
        """-> dict(precision, recall, density, coverage, nearest_k, n_real, n_gen)."""
        k = self.nearest_k
        for name, rows in (('real', self.real), ('generated', self.gen)):
            if rows.n < k + 1:
                raise ValueError('ManifoldMetrics.finalize: %d %s rows, nearest_k = %d needs at least %d' % (rows.n, name, k, k + 1))
            if not bool(torch.isfinite(rows.rows()).all()):
                raise ValueError('ManifoldMetrics.finalize: a %s feature is not finite' % name)
        cnt_gen, cnt_real, covered = manifold_passes(self.real.rows(), self.gen.rows(), k)
        return ratios(cnt_gen.cpu().numpy(), cnt_real.cpu().numpy(), covered.cpu().numpy(), k)
