"""Multi-scale structural similarity (MS-SSIM) between pairs of images — the diversity metric of Karras et al., "Progressive growing
of GANs" (their ms_ssim.py, which is the TensorFlow-compression msssim), measured between pairs of GENERATED images: the only
metric here that looks at the variation within the generated set (a generator that ignores z scores 1).  The reference has no
such metric; like evaluation/imd.py and evaluation/swd.py it is an addition.  Everything heavy runs in csrc/t2i_msssim.hip:

  per scale l = 0..4 of size h x w (halved, rounding up, from scale to scale), with the window g = K.msssim_window(h, w) of side
  S = min(11, h, w) and sigma = 1.5 S / 11, one t2i_ssim_scale call gives per pair cs_l = mean(v1 / v2) and
  ssim_l = mean((2 mu1 mu2 + c1) v1 / ((mu1^2 + mu2^2 + c1) v2)) over the valid (h - S + 1) x (w - S + 1) x C map (fp64 moments),
  and, except at the last scale, the 2 x 2 means that are the next scale's images;
  msssim = prod_{l < 4} max(cs_l, 0)^w_l * max(ssim_4, 0)^w_4 on the host in float64.  ms_ssim.py raises a negative base to a
  fractional power and returns NaN; the clamp at 0 is tf.image.ssim_multiscale's, and `clamped` counts the (pair, scale) entries
  it changed.

Images are file levels 0..255 held as floats (c1 = (0.01 max_val)^2, c2 = (0.03 max_val)^2); quantize() maps a generator's
[-1, 1] output to them."""
import numpy as np
import torch

from .. import kernels as K

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
K1, K2 = 0.01, 0.03


def quantize(x):
    """[-1, 1] -> file levels: clamp(round(x * 127.5 + 127.5), 0, 255), the multiply and the add as separate fp32 operations,
    round-half-to-even (numpy's float32 arithmetic and np.round give the same bits).  One elementwise pass."""
    return torch.clamp(torch.round(torch.add(torch.mul(x, 127.5), 127.5)), 0.0, 255.0)


def scale_sides(H, W, scales):
    """[(h, w)] per scale: halved, rounding up."""
    sides = []
    for _ in range(scales):
        sides.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return sides


def combine(cs, ssim, weights=WEIGHTS):
    """cs, ssim float64 [scales, pairs] -> (values float64 [pairs], clamped): prod_{l < L-1} max(cs_l, 0)^w_l * max(ssim_{L-1}, 0)^w_{L-1}
    and the number of (pair, scale) entries the clamp changed."""
    cs, ssim = np.asarray(cs, np.float64), np.asarray(ssim, np.float64)
    w = np.asarray(weights, np.float64).reshape(-1, 1)
    base = np.concatenate([cs[:-1], ssim[-1:]], 0)
    clamped = int(np.count_nonzero(base < 0))
    return np.prod(np.maximum(base, 0.0) ** w, axis=0), clamped


class MultiScaleSSIM(object):
    """MultiScaleSSIM((H, W, C), device): add(a, b) per batch of device float32 [n, H, W, C] pairs, then finalize() ->
    dict(values float64 [pairs], mean, std, cs_levels: the mean cs per scale, clamped, sides: (h, w) per scale)."""

    def __init__(self, shape, device, max_val=255.0, weights=WEIGHTS, filter_size=11, filter_sigma=1.5):
        H, W, C = (int(s) for s in shape)
        self.weights = tuple(float(w) for w in weights)
        scales = len(self.weights)
        if scales < 1 or min(H, W) < 1 << (scales - 1):
            raise ValueError('MS-SSIM over %d scales needs images of at least %d x %d, got %d x %d' % (
                scales, 1 << max(scales - 1, 0), 1 << max(scales - 1, 0), H, W))
        if not 1 <= C <= 4:
            raise ValueError('MS-SSIM takes images of 1 to 4 channels, got %d' % C)
        if not (float(max_val) > 0 and int(filter_size) >= 1 and float(filter_sigma) > 0):
            raise ValueError('MS-SSIM needs positive max_val, filter_size and filter_sigma (got %r, %r, %r)' % (max_val, filter_size, filter_sigma))
        self.shape, self.device = (H, W, C), torch.device(device)
        self.c1, self.c2 = (K1 * float(max_val)) ** 2, (K2 * float(max_val)) ** 2
        self.sides = scale_sides(H, W, scales)
        self.windows = [K.msssim_window(h, w, filter_size, filter_sigma) for h, w in self.sides]
        self.cs, self.ssim = [], []                       # per add: float64 [scales, n] on the device

    def add(self, a, b, quantized=False):
        """One batch of pairs; quantized=False: a and b are in [-1, 1] and go through quantize() first.  One t2i_ssim_scale call
        per scale (the last one writes no next scale): a linear chain of launches, capturable."""
        H, W, C = self.shape
        if tuple(a.shape) != tuple(b.shape) or tuple(a.shape[1:]) != (H, W, C) or a.shape[0] == 0:
            raise ValueError('MS-SSIM.add: a %s and b %s must both be [n, %d, %d, %d]' % (tuple(a.shape), tuple(b.shape), H, W, C))
        a, b = a.float().contiguous(), b.float().contiguous()
        if not quantized:
            a, b = quantize(a), quantize(b)
        cs, ssim = [], []
        last = len(self.windows) - 1
        for l, win in enumerate(self.windows):
            s, c, a, b = K.ssim_scale(a, b, win, self.c1, self.c2, downsample=l < last)
            ssim.append(s)
            cs.append(c)
        self.cs.append(torch.stack(cs))
        self.ssim.append(torch.stack(ssim))

    def finalize(self):
        if not self.cs:
            raise ValueError('MS-SSIM.finalize: no pairs were added')
        cs = torch.cat(self.cs, 1).cpu().numpy()
        ssim = torch.cat(self.ssim, 1).cpu().numpy()
        values, clamped = combine(cs, ssim, self.weights)
        return dict(values=values, mean=float(np.mean(values)), std=float(np.std(values)), cs_levels=[float(v) for v in cs.mean(axis=1)],
                    clamped=clamped, sides=list(self.sides))
