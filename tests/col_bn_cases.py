"""The column reductions and the batch-norm family of csrc/t2i_aux.hip restated in plain float64 NumPy, one statement per line, with
the planner of their first stage (col_reduce_plan, bn_group_plan, bn_fuse_rows) and the inputs and shape lists of
tests/test_col_bn_host.py and tests/test_col_bn_gpu.py.

Every restatement takes float64 arrays (the tests hand it the float32 / bf16 inputs of the kernel, widened exactly) and follows the
definition, not the kernel: no chunks, no Chan merges, no three-coefficient form of dx.  The host test holds the forward, the
backward and the moving averages to float64 autograd of the oracle's batch norm, so that the GPU test does not compare a kernel
with a copy of itself; it also holds plan() / group_plan() to the library's workspace queries on every shape listed here, so that
the chunk count each case says it reaches is the one the library really uses."""
import numpy as np
import torch

EPS, DECAY, ALPHA = 1e-5, 0.9, 0.25
ACTS = ('none', 'relu', 'lrelu')


def f64(t):
    """a float32 / bfloat16 tensor or array widened to float64 NumPy (exact)"""
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def relerr(got, ref):
    """max-norm relative error"""
    got, ref = f64(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


class Report(object):
    """The measured errors of one case against their bounds: all printed (pytest -s), all failures reported together."""

    def __init__(self, case):
        self.case, self.seen, self.bad = case, [], []

    def check(self, name, err, tol):
        self.seen.append((name, err, tol))
        if not err <= tol:
            self.bad.append((name, err, tol))

    def done(self):
        print('  case %s: %s' % (self.case, ', '.join('%s %.2e/%.0e' % t for t in self.seen)))
        assert not self.bad, (self.case, self.bad)


# ---- the planner (col_reduce_plan, bn_group_plan, bn_fuse_rows) ---------------------------------------------------------------
def plan(rows, C, wgs=768, cap=192):
    """-> (column tiles of 64, row chunks, rows per chunk) of a column reduction over [rows, C]"""
    ctiles = (C + 63) // 64
    want = wgs // ctiles
    want = max(want, 1)
    want = min(want, (rows + 63) // 64)
    want = min(want, cap)
    want = max(want, 1)
    rpc = (rows + want - 1) // want
    nchunks = max((rows + rpc - 1) // rpc, 1)
    return ctiles, nchunks, rpc


def group_plan(rows_g, C, groups, wgs=768, cap=192):
    """-> (column tiles, chunks PER GROUP, rows per chunk): all groups together get about the partial rows of one pass"""
    ctiles, ncg, rpc = plan(rows_g, C, wgs, cap)
    gcap = max(cap // groups, 1)
    if ncg > gcap:
        rpc = (rows_g + gcap - 1) // gcap
        ncg = (rows_g + rpc - 1) // rpc
    return ctiles, ncg, rpc


def fuse_rows(rows_g, ctiles, groups):
    """-> (rows per workgroup, workgroups per group) of the fused normalisation / dx kernels"""
    want = 1024 // (ctiles * groups)
    want = max(want, 1)
    want = min(want, (rows_g + 15) // 16)
    rpb = (rows_g + want - 1) // want
    return rpb, (rows_g + rpb - 1) // rpb


FUSE_MAX_CHUNKS = 64


def fused(ncg):
    """the second stage runs in the consumer's prologue (tuning bn_fuse = 1, the default)"""
    return ncg <= FUSE_MAX_CHUNKS


def chunk_bounds(rows_g, nchunks, rpc, groups=1):
    """[(first row, last row)] of every chunk, in the order of the partial rows: chunks never straddle a group"""
    out = []
    for g in range(groups):
        for k in range(nchunks):
            first = g * rows_g + k * rpc
            last = min(g * rows_g + (k + 1) * rpc, (g + 1) * rows_g) - 1
            assert first <= last, (rows_g, nchunks, rpc, g, k)
            out.append((first, last))
    return out


def ws_bytes(rows, C):
    return plan(rows, C)[1] * C * 8


def grouped_ws_bytes(rows_g, C, groups):
    return (groups * group_plan(rows_g, C, groups)[1] * C * 2 + groups * 3 * C) * 4


# ---- reductions ---------------------------------------------------------------------------------------------------------------
def _acc(a):
    a = np.asarray(a)
    return a.astype(np.int64) if np.issubdtype(a.dtype, np.integer) else a.astype(np.float64)


def col_sum(a):
    a = _acc(a)
    return a.reshape(-1, a.shape[-1]).sum(0)


def col_sum_sq(a):
    a = _acc(a)
    return (a * a).reshape(-1, a.shape[-1]).sum(0)


def col_sum_prod(a, b, center=None):
    """sum over rows of a * (b - center)"""
    a, b = _acc(a), _acc(b)
    d = b if center is None else b - _acc(center)
    return (a * d).reshape(-1, a.shape[-1]).sum(0)


def act_grad(y, act, alpha=ALPHA):
    """d act / d input from the activation's OUTPUT: 1, or alpha (lrelu) / 0 (relu) where y <= 0"""
    y = np.asarray(y, np.float64)
    if act == 'none':
        return np.ones_like(y)
    return np.where(y > 0.0, 1.0, alpha if act == 'lrelu' else 0.0)


def apply_act(z, act, alpha=ALPHA):
    if act == 'none':
        return z
    return np.where(z > 0.0, z, (alpha if act == 'lrelu' else 0.0) * z)


# ---- statistics and finalize --------------------------------------------------------------------------------------------------
def bn_stats(x):
    """x [rows, C] -> (sum, M2 = sum (x - mean)^2)"""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    return x.sum(0), ((x - mean) ** 2).sum(0)


def bn_finalize(s, m2, n, gamma, beta, moving_mean=None, moving_var=None, updates=1, moving_groups=0, eps=EPS, decay=DECAY):
    """s, m2 [groups, C] (or [C]) -> dict(mean, rstd, var, scale, shift [groups, C], moving_mean, moving_var [C]).  The moving averages
    take every group's statistics in group order, `updates` sequential steps each; moving_groups > 0: only the first that many groups."""
    s, m2 = np.atleast_2d(np.asarray(s, np.float64)), np.atleast_2d(np.asarray(m2, np.float64))
    mean = s / n
    var = m2 / n
    rstd = 1.0 / np.sqrt(var + eps)
    scale = np.asarray(gamma, np.float64) * rstd
    shift = np.asarray(beta, np.float64) - mean * scale
    out = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift)
    if moving_mean is not None:
        mm, mv = np.array(moving_mean, np.float64), np.array(moving_var, np.float64)
        unbiased = var * (n / max(n - 1, 1))
        for g in range(s.shape[0]):
            if moving_groups and g >= moving_groups:
                break
            for _ in range(updates):
                mm = decay * mm + (1.0 - decay) * mean[g]
                mv = decay * mv + (1.0 - decay) * unbiased[g]
        out.update(moving_mean=mm, moving_var=mv)
    return out


def bn_forward(x, gamma, beta, groups=1, act='none', alpha=ALPHA, **kw):
    """x [groups * rows_g, C], statistics per group -> bn_finalize's dict + y"""
    x = np.asarray(x, np.float64)
    C = x.shape[-1]
    xg = x.reshape(groups, -1, C)
    n = xg.shape[1]
    stats = [bn_stats(xg[g]) for g in range(groups)]
    out = bn_finalize(np.stack([s for s, _ in stats]), np.stack([m for _, m in stats]), n, gamma, beta, **kw)
    xhat = (xg - out['mean'][:, None, :]) * out['rstd'][:, None, :]
    z = xhat * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    out['y'] = apply_act(z, act, alpha).reshape(x.shape)
    return out


# ---- backward -----------------------------------------------------------------------------------------------------------------
def bn_backward(dy, y, x, mean, rstd, gamma, groups=1, act='none', alpha=ALPHA):
    """dy, x [groups * rows_g, C]; y the activation's output or None; mean, rstd [groups, C] as the forward stored them.
    -> dict(dx, dgamma, dbeta (summed over the groups), gmask = dy * act'(y), and per group and column k_x, mean, xmax = max|x|)"""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    C = x.shape[-1]
    gamma = np.asarray(gamma, np.float64)
    gmask = dy if y is None else dy * act_grad(y, act, alpha)
    gg, xg = gmask.reshape(groups, -1, C), x.reshape(groups, -1, C)
    mean, rstd = np.asarray(mean, np.float64).reshape(groups, 1, C), np.asarray(rstd, np.float64).reshape(groups, 1, C)
    xhat = (xg - mean) * rstd
    mean_g = gg.mean(1, keepdims=True)
    mean_gx = (gg * xhat).mean(1, keepdims=True)
    dx = gamma * rstd * (gg - mean_g - xhat * mean_gx)
    dgamma = (gg * xhat).sum((0, 1))
    dbeta = gg.sum((0, 1))
    k_x = -gamma * rstd * rstd * mean_gx                     # the coefficient of x once dx is expanded: what the cancellation bound needs
    return dict(dx=dx.reshape(x.shape), dgamma=dgamma, dbeta=dbeta, gmask=gmask, k_x=k_x[:, 0, :], mean=mean[:, 0, :],
                xmax=np.abs(xg).max(1))


# ---- tile partials, as a conv epilogue leaves them ---------------------------------------------------------------------------
def tile_partials(x, tile_rows, groups=1):
    """x [groups * rows_g, C] -> (sums, M2 about the tile's own mean) [groups * tiles, C] in float32; the last tile of a group may be short"""
    x = np.asarray(x, np.float64)
    C = x.shape[-1]
    xg = x.reshape(groups, -1, C)
    sums, m2s = [], []
    for g in range(groups):
        for r0 in range(0, xg.shape[1], tile_rows):
            t = xg[g, r0:r0 + tile_rows]
            sums.append(t.sum(0))
            m2s.append(((t - t.mean(0)) ** 2).sum(0))
    return np.stack(sums).astype(np.float32), np.stack(m2s).astype(np.float32)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def marked_integers(rows, C, seed, lo=-3, hi=3, base=1000, span=None, step=1):
    """Small integers (multiples of `step`) with a distinct large one in the first and the last row of every chunk of plan(rows, C):
    a dropped or doubled boundary row moves a column sum by more than any rounding could.  span: the markers are base + 2 step (i % span)."""
    rs = np.random.RandomState(seed)
    a = rs.randint(lo, hi + 1, size=(rows, C)).astype(np.int64) * step
    _, nchunks, rpc = plan(rows, C)
    i = 0
    for first, last in chunk_bounds(rows, nchunks, rpc):
        for r in sorted(set((first, last))):
            m = base + 2 * step * (i if span is None else i % span)
            a[r] = m * np.where(np.arange(C) % 2 == 0, 1, -1)
            a[r, (i * 5) % C] += step                        # and the columns of a marker row differ as well
            i += 1
    return a


def assert_exact_in_f32(*terms):
    """every partial sum, in any order, is an integer below 2^24"""
    for t in terms:
        t = np.abs(np.asarray(t, np.int64)).reshape(-1, t.shape[-1])
        assert int(t.sum(0).max()) < (1 << 24), int(t.sum(0).max())


def gaussian_columns(rows, C, seed, offset=0.0):
    """Gaussian data with per-column means over [-3, 3] (+ offset) and standard deviations over [0.5, 2]; float32"""
    rs = np.random.RandomState(seed)
    mean = np.linspace(-3.0, 3.0, C) if C > 1 else np.array([1.5])
    std = 0.5 + 1.5 * ((np.arange(C) * 7) % 11) / 10.0
    return (offset + mean + std * rs.standard_normal((rows, C))).astype(np.float32)


def affine(C, seed):
    """gamma in [0.5, 1.5], beta Gaussian, non-trivial moving averages; float32"""
    rs = np.random.RandomState(1000 + seed)
    gamma = (0.5 + rs.rand(C)).astype(np.float32)
    beta = rs.standard_normal(C).astype(np.float32)
    mm = rs.standard_normal(C).astype(np.float32)
    mv = (0.5 + rs.rand(C)).astype(np.float32)
    return gamma, beta, mm, mv


def grouped_input(groups, rows_g, C, seed):
    """Groups whose means differ by more than a standard deviation: 2.5 (g % 4) against std <= 2.

    rows_g < 4 is made on purpose, not drawn.  With two rows x = m +- v the exact gradient is dx = +- gamma rstd d eps / (v^2 + eps)
    (d half the difference of the two dy): at v ~ 1 a residual of 1e-5 of its two terms, which no float32 evaluation of any form of
    the formula can give to 1e-4, and y = x scale + shift loses |m| rstd 2^-24.  So v is taken of the size of sqrt(eps)
    (0.003 .. 0.006) and the group means of the size of a few v (0.02 (g % 4)): dx is then as large as its terms and y as its own,
    and both can be held to the same bounds as everywhere else — tight enough to see a wrong coefficient row."""
    if rows_g < 4:
        rs = np.random.RandomState(seed)
        v = 0.003 * (1.0 + rs.rand(groups, 1, C)) * np.where(np.arange(rows_g) % 2 == 0, 1.0, -1.0).reshape(1, rows_g, 1)
        x = 0.02 * (np.arange(groups) % 4).reshape(groups, 1, 1) + 0.004 * np.linspace(-1.0, 1.0, C) + v
        return x.reshape(groups * rows_g, C).astype(np.float32)
    x = gaussian_columns(groups * rows_g, C, seed).astype(np.float64).reshape(groups, rows_g, C)
    x = x + 2.5 * (np.arange(groups) % 4).reshape(groups, 1, 1)
    return x.reshape(groups * rows_g, C).astype(np.float32)


def bf16_round(a):
    return torch.tensor(np.asarray(a, np.float32)).bfloat16().float().numpy()


# ---- the shapes of the GPU file, each with the chunk count it means to reach (asserted against the library by the host test) ------
# (rows, C, chunks): plain reductions and statistics
ROWS_AT_C4 = [(1, 1), (63, 1), (64, 1), (65, 2), (4096, 64), (4097, 65), (12288, 192), (12289, 190)]
REDUCE_CASES = [(r, 4, n) for r, n in ROWS_AT_C4] + [
    (4097, 1, 65), (4097, 3, 65),                # _small
    (65, 5, 2), (4097, 5, 65),                   # scalar stage 1, scalar stage 2
    (65, 8, 2), (4097, 8, 65), (4097, 64, 65),   # _v4, one column tile
    (65, 68, 2), (4097, 68, 65),                 # _v4, the second tile 4 wide
    (4097, 132, 65),                             # three tiles
    (3072, 1024, 48),                            # 16 tiles: want = 768 / 16
    (130, 49216, 1),                             # 769 tiles: want clamps to 1
]
MISALIGNED_CASES = [(4097, 4, 65), (65, 68, 2), (4097, 68, 65)]      # from a base one float into a buffer: _small resp. the scalar kernel
BF16_REDUCE_CASES = [(65, 8, 2), (4097, 8, 65), (65, 68, 2), (4097, 68, 65)]
STATS_CASES = [(r, C, n) for C in (3, 5, 8, 68) for r, n in ROWS_AT_C4]
PARTIALS_CASES = [(1, 4), (17, 8), (193, 68), (5, 6), (64, 3)]       # (chunks, C) of t2i_col_reduce_partials
# (rows, tile_rows, tiles)
TILE_CASES = [(128, 128, 1), (130, 128, 2), (4096, 64, 64), (4160, 64, 65), (12300, 64, 193)]
TILE_GROUPED = [(128, 128), (4096, 64), (4160, 64)]                  # rows_g % tile_rows == 0: these also run with groups = 2
# (groups, rows_g, C, chunks per group, fused by default)
GROUPED_CASES = [
    (1, 7, 8, 1, True),
    (3, 15, 36, 1, True),
    (3, 100, 8, 2, True),
    (3, 101, 8, 2, True),                        # chunks of 51 and 50: the second short, none straddling a group
    (3, 4096, 8, 64, True),                      # the cap for three groups, the last fused count
    (2, 6144, 8, 96, False),                     # the only default route to the unfused grouped path
    (1, 4097, 8, 65, False),
    (200, 2, 4, 1, True),                        # cap clamps to 1; the scribe walks 200 groups
    (3, 20, 1028, 1, True),                      # 17 column tiles, the last 4 wide
    (2, 8200, 132, 96, False),                   # 2 164 800 elements: the unfused apply kernels wrap their grid
]
SINGLE_BWD_CASES = [(7, 8, 1), (4097, 8, 65), (130, 68, 3)]           # bn_bwd_fused and col_reduce + bn_bwd
SCALAR_BWD_CASES = [(15, 6, 1), (130, 6, 3)]                          # bn_bwd alone: bn_bwd_apply_kernel<false>
BF16_GROUPED = [(3, 4096, 8, 64, True), (1, 4097, 8, 65, False)]
# (rows, C, offset, chunks)
LARGE_MEAN_CASES = [(2, 64, 300.0, 1), (32, 8, 1000.0, 1), (1024, 8, 50.0, 16), (4097, 8, 1000.0, 65)]
