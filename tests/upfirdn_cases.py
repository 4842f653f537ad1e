"""The resampling operator of DESIGN.md section 4.41 (csrc/t2i_resample.hip) restated in float64 numpy by its definition, the
parameters of its adjoint, and the case table of tests/test_upfirdn_host.py and tests/test_upfirdn_gpu.py.

Per axis, for x of extent H, taps f[0..n) ROUNDED TO FLOAT32 FIRST (the kernel gets float32 taps), factors u, d, pads p0, p1:
  z[j] = x[j / u] where 0 <= j < H u and u divides j, else 0            (zero insertion)
  pad z by p0 in front and p1 behind, a negative pad cropping           (extent H u + p0 + p1)
  v[i] = sum_t g[n - 1 - t] z[i + t],  g = f or f reversed when flip    (VALID, true convolution: a loop over the taps)
  y[o] = v[o d]                                                         (every d-th sample)
applied along H and along W of [B,H,W,C]."""
import functools

import numpy as np
import torch

TILE = 8                          # kernels.UPFIRDN_TILE, asserted by the tests that import both

UD = ((1, 1), (2, 1), (1, 2), (2, 2))
TAPS = {
    'n1': (1.5,),
    'box2': (1.0, 1.0),
    'tri3': (1.0, 2.0, 1.0),
    'bin4': (1.0, 3.0, 3.0, 1.0),
    'asym5': (0.5, -1.0, 2.0, 3.0, 0.25),                     # a wrong flip or tap order shows
    'oct8': (1.0, -2.0, 3.0, 4.0, 5.0, -1.0, 2.0, 0.5),
}
PADS = ('helper', (0, 0), (-1, 0), (3, -1), 'big')
EXTENTS = ((1, 1), (2, 3), (5, 7), (TILE - 1, TILE), (TILE, TILE + 1), (TILE + 1, 2 * TILE + 1), (2 * TILE + 1, TILE - 1))
CHANNELS = (1, 3, 4, 20, 68)


def extent(H, u, d, p0, p1, n):
    """The extent formula of DESIGN.md section 4.41; < 1 means the shape has no output."""
    return (H * u + p0 + p1 - n) // d + 1 if H * u + p0 + p1 - n >= 0 else 0


def adjoint_params(H, Ho, n, u, d, p0, flip):
    """(u', d', p0', p1', flip') of the adjoint of an operator that took extent H to Ho: it returns extent H exactly."""
    return d, u, n - 1 - p0, H * u - Ho * d + p0 - u + 1, not flip


def helper_pads(n, u, d):
    """The publication's pads: upsample_2d's where u = 2, else downsample_2d's (factor d), p = n - factor."""
    if u == 2:
        p = n - 2
        return (p + 1) // 2 + 1, p // 2
    p = n - d
    return (p + 1) // 2, p // 2


def pads_of(pad, n, u, d):
    if pad == 'helper':
        return helper_pads(n, u, d)
    if pad == 'big':
        return n + 2, n + 1
    return pad


def _axis(x, axis, g32, u, d, p0, p1):
    x = np.moveaxis(x, axis, 0)
    H, rest = x.shape[0], x.shape[1:]
    z = np.zeros((H * u,) + rest)
    z[::u] = x                                                   # zero insertion
    for front, p in ((True, p0), (False, p1)):                   # pad or crop
        if p >= 0:
            blk = np.zeros((p,) + rest)
            z = np.concatenate([blk, z] if front else [z, blk], 0)
        else:
            z = z[-p:] if front else z[:z.shape[0] + p]
    n = len(g32)
    Lo = z.shape[0] - n + 1
    assert Lo >= 1, 'no output'
    v = np.zeros((Lo,) + rest)
    for t in range(n):                                           # VALID true convolution
        v += float(g32[n - 1 - t]) * z[t:t + Lo]
    return np.moveaxis(v[::d], 0, axis)                          # decimation


def ref_upfirdn2d(x, taps, u, d, p0, p1, flip=False):
    """x [B,H,W,C] (any float array / tensor) -> float64 numpy [B,Ho,Wo,C].  p1: an integer or a pair (along H, along W)."""
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    g = np.asarray(taps, dtype=np.float32)                       # rounded to fp32 first
    if flip:
        g = g[::-1]
    p1h, p1w = p1 if isinstance(p1, (tuple, list)) else (p1, p1)
    return _axis(_axis(x, 1, g, u, d, p0, p1h), 2, g, u, d, p0, p1w)


def _axis_torch(x, axis, g32, u, d, p0, p1):
    if u == 2:                                                   # zero insertion
        x = torch.stack([x, torch.zeros_like(x)], axis + 1).flatten(axis, axis + 1)
    for front, p in ((True, p0), (False, p1)):                   # pad or crop
        if p >= 0:
            shape = list(x.shape)
            shape[axis] = p
            blk = x.new_zeros(shape)
            x = torch.cat([blk, x] if front else [x, blk], axis)
        else:
            x = x.narrow(axis, -p if front else 0, x.shape[axis] + p)
    n = len(g32)
    Lo = x.shape[axis] - n + 1
    assert Lo >= 1, 'no output'
    v = 0
    for t in range(n):                                           # VALID true convolution
        v = v + float(g32[n - 1 - t]) * x.narrow(axis, t, Lo)
    return v.index_select(axis, torch.arange(0, Lo, d))          # decimation


def ref_torch(x, taps, u, d, p0, p1, flip=False, axes=(1, 2)):
    """The same statements on a torch tensor of any float dtype, along `axes` ((2, 3) for NCHW): differentiable to any order."""
    g = np.asarray(taps, dtype=np.float32)
    if flip:
        g = g[::-1]
    return _axis_torch(_axis_torch(x, axes[0], g, u, d, p0, p1), axes[1], g, u, d, p0, p1)


def helper_taps(k, up):
    """The float32 taps of upsample_2d (2 k / sum k) or downsample_2d (k / sum k) with factor 2"""
    k = np.asarray(k, dtype=np.float64)
    return tuple(float(t) for t in ((2.0 if up else 1.0) * k / k.sum()).astype(np.float32))


def bound(taps, x):
    """(n^2 + 2) 2^-24 (sum |g|)^2 max |x|: at most n^2 products and one intermediate rounding (derived, not measured)."""
    n = len(taps)
    s = float(np.abs(np.asarray(taps, dtype=np.float32).astype(np.float64)).sum())
    return (n * n + 2) * 2.0 ** -24 * s * s * float(np.abs(np.asarray(x)).max())


def _valid(H, W, n, u, d, p0, p1):
    return extent(H, u, d, p0, p1, n) >= 1 and extent(W, u, d, p0, p1, n) >= 1


PART = []                          # per case: 'taps_pads' or 'extents', the part of the table it belongs to


def _cases():
    out = []
    # every (u, d) x taps x pads at 3 x 5 x 7 x 3, both flips alternating; a combination without an output is not a case
    k = 0
    for u, d in UD:
        for name, f in TAPS.items():
            for pad in PADS:
                p0, p1 = pads_of(pad, len(f), u, d)
                if _valid(5, 7, len(f), u, d, p0, p1):
                    out.append(((3, 5, 7, 3), name, u, d, p0, p1, bool(k % 2)))
                    PART.append('taps_pads')
                    k += 1
    # every extent x channel count x (u, d) with the binomial filter at the helpers' pads, and the asymmetric one at (3, -1)
    for (H, W) in EXTENTS:
        for C in CHANNELS:
            for u, d in UD:
                for name, pad in (('bin4', 'helper'), ('asym5', (3, -1))):
                    p0, p1 = pads_of(pad, len(TAPS[name]), u, d)
                    if _valid(H, W, len(TAPS[name]), u, d, p0, p1):
                        out.append(((1 if C != 3 else 3, H, W, C), name, u, d, p0, p1, name == 'asym5'))
                        PART.append('extents')
    return out


CASES = _cases()


def case_id(c):
    shape, name, u, d, p0, p1, flip = c
    return '%s-%s-u%dd%d-p%d_%d%s' % ('x'.join(str(s) for s in shape), name, u, d, p0, p1, '-flip' if flip else '')


def inputs(shape, seed=0):
    rs = np.random.RandomState(4100 + seed + sum(shape) * 7 + shape[3])
    return torch.tensor(rs.standard_normal(shape), dtype=torch.float32)


def adjoint_of(c):
    """(u', d', p0', (p1' along H, along W), flip') of the adjoint of case c"""
    shape, name, u, d, p0, p1, flip = c
    n = len(TAPS[name])
    Ho, Wo = out_shape(c)[1:3]
    ua, da, p0a, p1h, fa = adjoint_params(shape[1], Ho, n, u, d, p0, flip)
    return ua, da, p0a, (p1h, adjoint_params(shape[2], Wo, n, u, d, p0, flip)[3]), fa


def out_shape(c):
    (B, H, W, C), name, u, d, p0, p1, _ = c
    n = len(TAPS[name])
    return (B, extent(H, u, d, p0, p1, n), extent(W, u, d, p0, p1, n), C)


@functools.lru_cache(maxsize=None)
def reference(i):
    """(x, forward reference, g, adjoint reference, adjoint parameters) of CASES[i]: computed once and never written to"""
    shape, name, u, d, p0, p1, flip = CASES[i]
    f = TAPS[name]
    x, g = inputs(shape), inputs(out_shape(CASES[i]), seed=1)
    y = ref_upfirdn2d(x, f, u, d, p0, p1, flip)
    adj = adjoint_of(CASES[i])
    return x, y, g, ref_upfirdn2d(g, f, *adj), adj
