"""Shared by tests/test_msssim_host.py and tests/test_msssim_gpu.py: the float64 restatement of the multi-scale structural
similarity (Karras et al., ms_ssim.py = the TensorFlow-compression msssim) and the seeded input families.
scipy.signal.convolve(mode='valid', method='direct') with the 2-D window is the authority for the moments,
scipy.ndimage.convolve(mode='reflect') for the downsample; nothing here calls the package's kernels."""
import functools

import numpy as np
import scipy.ndimage
import scipy.signal

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_VAL, K1, K2 = 255.0, 0.01, 0.03
C1, C2 = (K1 * MAX_VAL) ** 2, (K2 * MAX_VAL) ** 2
FAMILIES = ('near', 'indep', 'flat', 'neg')


def fspecial_gauss(size, sigma):
    """ms_ssim.py's _FSpecialGauss: the 2-D normalised Gaussian of side `size`."""
    radius = size // 2
    offset = 0.0
    start, stop = -radius, radius + 1
    if size % 2 == 0:
        offset = 0.5
        stop -= 1
    x, y = np.mgrid[offset + start:stop, offset + start:stop]
    g = np.exp(-((x ** 2 + y ** 2) / (2.0 * sigma ** 2)))
    return g / g.sum()


def window_2d(h, w, filter_size=11, filter_sigma=1.5):
    """The window of a scale of size h x w: side min(filter_size, h, w), sigma scaled with the side."""
    size = min(filter_size, h, w)
    return fspecial_gauss(size, size * filter_sigma / filter_size)


def ssim_scale(a, b, filter_size=11, filter_sigma=1.5):
    """a, b [N, H, W, C] (levels 0..255) -> (ssim [N], cs [N]) in float64: _SSIMForMultiScale with its convolutions done directly."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    win = window_2d(a.shape[1], a.shape[2], filter_size, filter_sigma)[np.newaxis, :, :, np.newaxis]

    def blur(x):
        return scipy.signal.convolve(x, win, mode='valid', method='direct')
    mu1, mu2 = blur(a), blur(b)
    s11, s22, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    v1, v2 = 2.0 * s12 + C2, s11 + s22 + C2
    ssim = np.mean(((2.0 * mu1 * mu2 + C1) * v1) / ((mu1 * mu1 + mu2 * mu2 + C1) * v2), axis=(1, 2, 3))
    return ssim, np.mean(v1 / v2, axis=(1, 2, 3))


def downsample_scipy(x):
    """[N, H, W, C] -> [N, ceil(H/2), ceil(W/2), C]: ms_ssim.py's 2 x 2 box filter with 'reflect' edges, every other pixel."""
    x = np.asarray(x, np.float64)
    return scipy.ndimage.convolve(x, np.ones((1, 2, 2, 1)) / 4.0, mode='reflect')[:, ::2, ::2, :]


def downsample(x):
    """The same as taps: out[i, j] = ((x[2i, 2j] + x[2i, j']) + (x[i', 2j] + x[i', j'])) * 0.25 with i' = min(2i + 1, H - 1),
    j' = min(2j + 1, W - 1), in x's own precision and in this association (what the kernel computes, bit for bit, in float32)."""
    x = np.asarray(x)
    H, W = x.shape[1], x.shape[2]
    i0, j0 = np.arange(0, H, 2), np.arange(0, W, 2)
    i1, j1 = np.minimum(i0 + 1, H - 1), np.minimum(j0 + 1, W - 1)
    top = x[:, i0][:, :, j0] + x[:, i0][:, :, j1]
    bottom = x[:, i1][:, :, j0] + x[:, i1][:, :, j1]
    return (top + bottom) * x.dtype.type(0.25)


def scales(a, b, n_scales=len(WEIGHTS)):
    """-> (ssim [n_scales, N], cs [n_scales, N], the image pairs per scale): float64 throughout, scipy's downsample."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ssim, cs, imgs = [], [], []
    for l in range(n_scales):
        imgs.append((a, b))
        s, c = ssim_scale(a, b)
        ssim.append(s)
        cs.append(c)
        if l + 1 < n_scales:
            a, b = downsample_scipy(a), downsample_scipy(b)
    return np.stack(ssim), np.stack(cs), imgs


def combine(ssim, cs, weights=WEIGHTS):
    """-> (values [N], clamped): prod_{l < L-1} max(cs_l, 0)^w_l * max(ssim_{L-1}, 0)^w_{L-1}; ms_ssim.py without the clamp
    returns NaN for a negative base."""
    base = np.concatenate([cs[:-1], ssim[-1:]], 0)
    w = np.asarray(weights, np.float64).reshape(-1, 1)
    return np.prod(np.maximum(base, 0.0) ** w, axis=0), int(np.count_nonzero(base < 0))


def msssim(a, b):
    """-> dict(values [N], clamped, cs_levels [5], ssim [5, N], cs [5, N])."""
    ssim, cs, _ = scales(a, b)
    values, clamped = combine(ssim, cs)
    return dict(values=values, clamped=clamped, cs_levels=cs.mean(axis=1), ssim=ssim, cs=cs)


def _levels(x):
    return np.clip(np.round(x), 0, 255).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pairs(family, seed, n, h, w, c):
    """(a, b): float32 [n, h, w, c] of integer levels 0..255 (so the 2 x 2 means stay exact in float32 through four downsamples).
    near: a blocky random image + N(0, 20) against itself + N(0, 25); indep: two independent uniform images; flat: level 200
    against 200 + {-1, 0, 1}; neg: the blocky image against 255 - itself.  Cached: do not modify the arrays."""
    rng = np.random.RandomState(seed)
    blocks = rng.randint(0, 256, size=(n, (h + 3) // 4, (w + 3) // 4, c)).astype(np.float64)
    blocky = np.repeat(np.repeat(blocks, 4, axis=1), 4, axis=2)[:, :h, :w, :]
    if family == 'near':
        a = _levels(blocky + rng.normal(0, 20, (n, h, w, c)))
        b = _levels(a + rng.normal(0, 25, (n, h, w, c)))
    elif family == 'indep':
        a = rng.randint(0, 256, size=(n, h, w, c)).astype(np.float32)
        b = rng.randint(0, 256, size=(n, h, w, c)).astype(np.float32)
    elif family == 'flat':
        a = np.full((n, h, w, c), 200.0, np.float32)
        b = (200 + rng.randint(-1, 2, size=(n, h, w, c))).astype(np.float32)
    elif family == 'neg':
        a = _levels(blocky + rng.normal(0, 20, (n, h, w, c)))
        b = (255.0 - a).astype(np.float32)
    else:
        raise ValueError(family)
    for x in (a, b):
        x.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def scale_reference(family, seed, shape):
    """The single-scale reference of pairs(family, seed, *shape), computed once: (ssim [N], cs [N])."""
    a, b = pairs(family, seed, *shape)
    return ssim_scale(a, b)


@functools.lru_cache(maxsize=None)
def msssim_reference(family, seed, shape):
    a, b = pairs(family, seed, *shape)
    return msssim(a, b)
