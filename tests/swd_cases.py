"""Shared by tests/test_swd_host.py and tests/test_swd_gpu.py: the float64 restatement of the sliced Wasserstein distance of
Laplacian-pyramid patch descriptors (Karras et al., sliced_wasserstein.py).  scipy.ndimage.convolve(mode='mirror') is the
authority for the pyramid; nothing here calls the package's kernels."""
import numpy as np
import scipy.ndimage

K1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
F = np.outer(K1, K1)


def pyr_down(g):
    """[N, H, W, C] float64 -> convolve(g, F, 'mirror')[::2, ::2] per image and channel."""
    return scipy.ndimage.convolve(g, F[np.newaxis, :, :, np.newaxis], mode='mirror')[:, ::2, ::2, :]


def pyr_up_zero_insert(g):
    """[N, h, w, C] -> [N, 2h, 2w, C]: zero-insert, then convolve with 4 F, 'mirror'."""
    n, h, w, c = g.shape
    z = np.zeros((n, 2 * h, 2 * w, c), np.float64)
    z[:, ::2, ::2, :] = g
    return scipy.ndimage.convolve(z, 4.0 * F[np.newaxis, :, :, np.newaxis], mode='mirror')


def _up_axis(g, axis):
    g = np.moveaxis(g, axis, 0)
    h = g.shape[0]
    prev = np.concatenate([g[1:2], g[:-1]], 0)           # g[-1] := g[1]
    nxt = np.concatenate([g[1:], g[h - 1:h]], 0)         # g[h] := g[h-1]
    out = np.empty((2 * h,) + g.shape[1:], np.float64)
    out[0::2] = (prev + 6.0 * g + nxt) / 8.0
    out[1::2] = (g + nxt) / 2.0
    return np.moveaxis(out, 0, axis)


def pyr_up_polyphase(g):
    """The same up-sampling in the polyphase form the kernel uses, axis by axis."""
    return _up_axis(_up_axis(np.asarray(g, np.float64), 1), 2)


def laplacian_pyramid(x, levels):
    """x [N, H, W, C] -> [lap_0, ..., lap_{levels-1}] in float64 (zero-insert + scipy form)."""
    g = [np.asarray(x, np.float64)]
    for _ in range(levels - 1):
        g.append(pyr_down(g[-1]))
    return [g[i] - pyr_up_zero_insert(g[i + 1]) for i in range(levels - 1)] + [g[-1]]


def descriptors(level, pos):
    """level [N, h, w, C], pos int [N, P, 2] (y, x) -> [N P, 49 C], rows flattened (c, dy, dx): numpy fancy indexing."""
    N, h, w, C = level.shape
    P = pos.shape[1]
    d = np.arange(-3, 4)
    n = np.arange(N).reshape(N, 1, 1, 1, 1)
    c = np.arange(C).reshape(1, 1, C, 1, 1)
    y = pos[:, :, 0].reshape(N, P, 1, 1, 1) + d.reshape(1, 1, 1, 7, 1)
    x = pos[:, :, 1].reshape(N, P, 1, 1, 1) + d.reshape(1, 1, 1, 1, 7)
    return level[n, y, x, c].reshape(N * P, 49 * C)


def channel_stats(A, C):
    """-> (mean [C], population std [C]) in float64, per channel over all rows and the channel's 49 columns."""
    a = np.asarray(A, np.float64).reshape(-1, C, 49)
    return a.mean(axis=(0, 2)), a.std(axis=(0, 2))


def standardise(A, C, mean=None, std=None):
    a = np.asarray(A, np.float64).reshape(-1, C, 49)
    if mean is None:
        mean, std = channel_stats(A, C)
    return ((a - mean.reshape(1, C, 1)) / std.reshape(1, C, 1)).reshape(a.shape[0], 49 * C)


def sliced_distance(A, B, dirs_list, C):
    """The level's SWD (not yet x 10^3): mean over the repeats of mean |sort(A d) - sort(B d)| for standardised A, B."""
    a, b = standardise(A, C), standardise(B, C)
    out = []
    for d in dirs_list:
        pa = np.sort(a @ np.asarray(d, np.float64), axis=0)
        pb = np.sort(b @ np.asarray(d, np.float64), axis=0)
        out.append(np.mean(np.abs(pa - pb)))
    return float(np.mean(out))


def projection_bound(A, C, dirs):
    """Per entry [rows, S]: (D + 2) 2^-24 sum_j |a^_j d_j| — D fused multiply-adds and the rounding of the standardised operand."""
    a = np.abs(standardise(A, C))
    D = a.shape[1]
    return (D + 2) * 2.0 ** -24 * (a @ np.abs(np.asarray(dirs, np.float64)))


def images(seed, n, side_h, side_w, c):
    """float32 [n, h, w, c] in [-1, 1]: smooth structure plus noise, so that every pyramid level carries signal."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:side_h, 0:side_w]
    base = np.sin(yy / 5.0 + seed)[..., None] * np.cos(xx / 3.0)[..., None] * np.array([0.5, 0.3, -0.4, 0.2])[:c]
    return np.clip(base[None] + rng.normal(0, 0.3, (n, side_h, side_w, c)), -1, 1).astype(np.float32)
