"""Pillow's 8-bit bilinear resize as the evaluator applies it (reference utils/utils.py prep_incep_img:
`scipy.misc.imresize(img, (299, 299, 3), interp='bilinear')`, which is `PIL.Image.resize(size, BILINEAR)` on the uint8 image,
then `astype(float32) / 127.5 - 1`).

`bilinear_tables` restates Pillow's precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) for one axis: the
filter support is scaled by max(1, in / out), so a downscale is antialiased, and the weights become 22-bit fixed point.  The
HIP kernel (t2i_resample_bilinear) applies the tables; `resize_u8` is the same two fixed-point passes in NumPy (horizontal,
then vertical through an 8-bit intermediate, each rounding with 2^21 and clipping), the host statement the tests hold both
Pillow and the kernel to.

`bicubic_tables` / `resize_u8_bicubic` are the same construction for Pillow's BICUBIC (a = -0.5, support 2): the stage-size
image stores of preprocess/stage_images.py.  Its negative lobes make some coefficients negative, and the 8-bit intermediate
clip then matters; the passes above already clip, as Pillow does."""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    """Pillow's bicubic_filter: the cubic convolution kernel with a = -0.5, support 2 (Keys)."""
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def bilinear_tables(in_size, out_size):
    """-> (bounds int32 [out, 2] = (first input index, tap count), coeffs int32 [out, ksize]) for one axis."""
    return _tables('bilinear_tables', _bilinear, 1.0, in_size, out_size)


@functools.lru_cache(maxsize=None)
def bicubic_tables(in_size, out_size):
    """bilinear_tables for Pillow's BICUBIC (support 2, negative lobes: coefficients may be negative)."""
    return _tables('bicubic_tables', _bicubic, 2.0, in_size, out_size)


def _tables(what, filt, filter_support, in_size, out_size):
    if in_size <= 0 or out_size <= 0:
        raise ValueError('%s: sizes must be positive, got %d -> %d' % (what, in_size, out_size))
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)      # int(): truncation toward zero, as the C cast
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = sum(w)                                     # left-to-right, as Pillow's loop
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            coeffs[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coeffs


def _pass(img, bounds, coeffs, axis):
    """One fixed-point pass of int64 arithmetic (Pillow's int32 never overflows for normalised weights) along `axis`."""
    out = np.full(img.shape[:axis] + (bounds.shape[0],) + img.shape[axis + 1:], 1 << (PRECISION_BITS - 1), np.int64)
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    dst = np.moveaxis(out, axis, 0)
    for o, (x0, n) in enumerate(bounds):
        for i in range(n):
            dst[o] += src[x0 + i] * int(coeffs[o, i])
    return np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _resize(what, tables, img, out_h, out_w):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError('%s expects a uint8 [H, W, C] image, got %s %s' % (what, img.dtype, img.shape))
    tmp = _pass(img, *tables(img.shape[1], out_w), axis=1)
    return _pass(tmp, *tables(img.shape[0], out_h), axis=0)


def resize_u8(img, out_h, out_w):
    """uint8 [H, W, C] -> uint8 [out_h, out_w, C]: Image.fromarray(img).resize((out_w, out_h), Image.BILINEAR)."""
    return _resize('resize_u8', bilinear_tables, img, out_h, out_w)


def resize_u8_bicubic(img, out_h, out_w):
    """uint8 [H, W, C] -> uint8 [out_h, out_w, C]: Image.fromarray(img).resize((out_w, out_h), Image.BICUBIC), which is what the
    reference's preprocessing calls (`scipy.misc.imresize(uint8_img, [s, s], 'bicubic')` passes a uint8 image to Pillow
    unchanged)."""
    return _resize('resize_u8_bicubic', bicubic_tables, img, out_h, out_w)


def to_rgb(img):
    """prep_incep_img's grayscale branch: a 2-D image is np.resize-d to [h, w, 3], which repeats the FLATTENED pixels
    cyclically (it does not replicate channels).  Other images are returned unchanged."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = np.resize(img, (img.shape[0], img.shape[1], 3))
    return img


def prep_incep_img(img, size=299):
    """Host statement of reference utils/utils.py prep_incep_img for a uint8 image: float32 [size, size, 3] in [-1, 1]."""
    return resize_u8(to_rgb(img), size, size).astype(np.float32) / 127.5 - 1.
