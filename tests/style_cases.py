"""Restatements for the style-based generator's layer (csrc/t2i_style.hip): the operator's forward and backward in
numpy, generic over the dtype and with two-pass moments; the case table of tests/test_style_gpu.py; and a float64 torch restatement of the
style-based PGGAN generator on top of oracle/torch_pggan.py's layers.  Test infrastructure only."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHUNK = 64                       # kernels.ADAIN_CHUNK_ROWS (tests/test_style_gpu.py asserts the two agree)
ACTS = (None, 'relu', 'lrelu')   # lrelu: slope 0.2
ALPHA = 0.2
EPS = 1e-8
KINK = 1e-3                      # inputs keep |x + strength * noise| at least this far from the kink of relu / lrelu


def act_np(p, act):
    if act is None:
        return p
    return np.where(p > 0, p, (0.0 if act == 'relu' else ALPHA) * p)


def dact_np(p, act):
    if act is None:
        return np.ones_like(p)
    return np.where(p > 0, 1.0, 0.0 if act == 'relu' else ALPHA).astype(p.dtype)


def forward(x, ys, yb, noise, strength, act, dtype, eps=EPS, one_pass=False):
    """-> (y, cache) in `dtype`.  Moments in two passes: the mean, then the mean of the squared deviations (one_pass: E[u^2] - mu^2,
    the form the kernel must NOT use; kept to show what it costs)."""
    c = lambda a: None if a is None else np.asarray(a).astype(dtype)
    x, ys, yb, noise, strength = c(x), c(ys), c(yb), c(noise), c(strength)
    p = x if noise is None else x + strength[None, None, None, :] * noise[..., None]
    u = act_np(p, act)
    mu = u.mean(axis=(1, 2), keepdims=True, dtype=dtype)
    if one_pass:
        var = (u * u).mean(axis=(1, 2), keepdims=True, dtype=dtype) - mu * mu
    else:
        var = ((u - mu) ** 2).mean(axis=(1, 2), keepdims=True, dtype=dtype)
    rstd = (1.0 / np.sqrt(var + dtype(eps))).astype(dtype)
    uh = (u - mu) * rstd
    y = uh * (1.0 + ys[:, None, None, :]) + yb[:, None, None, :]
    return y.astype(dtype), (p, uh, rstd, ys, noise)


def backward(g, cache, act, dtype):
    """-> (dx, dstrength or None, dys, dyb) for the cotangent g of y."""
    p, uh, rstd, ys, noise = cache
    g = np.asarray(g).astype(dtype)
    dyb = g.sum(axis=(1, 2), dtype=dtype)
    dys = (g * uh).sum(axis=(1, 2), dtype=dtype)
    n = dtype(p.shape[1] * p.shape[2])
    du = rstd * (1.0 + ys[:, None, None, :]) * (g - (dyb / n)[:, None, None, :] - uh * (dys / n)[:, None, None, :])
    dx = (du * dact_np(p, act)).astype(dtype)
    dstrength = None if noise is None else (dx * noise[..., None]).sum(axis=(0, 1, 2), dtype=dtype)
    return dx, dstrength, dys, dyb


def inputs(shape, noise, act, seed=0, mean=0.0):
    """float32 inputs of a case: x ~ N(mean, 1.3^2) + a per-channel offset, ys, yb, g, and (with noise) a standard-normal image and strengths
    in [-0.6, 0.6].  x is moved so that no pre-activation lies within KINK of 0: the derivative of relu / lrelu there is a convention,
    and float32 and float64 must agree on the side."""
    B, H, W, C = shape
    rng = np.random.default_rng(1000 * seed + 7 * B + 31 * H + 131 * W + 1009 * C + (3 if noise else 0))
    x = (mean + 1.3 * rng.standard_normal(shape) + 0.5 * rng.standard_normal((1, 1, 1, C))).astype(np.float32)
    ys = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
    yb = (0.5 * rng.standard_normal((B, C))).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    nz = st = None
    if noise:
        nz = rng.standard_normal((B, H, W)).astype(np.float32)
        st = rng.uniform(-0.6, 0.6, (C,)).astype(np.float32)
    if act is not None:
        p = x.astype(np.float64) if nz is None else x.astype(np.float64) + st.astype(np.float64) * nz.astype(np.float64)[..., None]
        near = np.abs(p) < KINK
        x = np.where(near, x + np.float32(4 * KINK) * np.where(p >= 0, 1, -1), x).astype(np.float32)
    return dict(x=x, ys=ys, yb=yb, g=g, noise=nz, strength=st)


MAPS = ((1, 1), (4, 4), (3, 5), (8, 8), (33, 31), (64, 64), (7, 9), (1, CHUNK), (5, 13), (3, 43))      # ..., chunk - 1, chunk, chunk + 1, 2 chunk + 1 rows
CHANNELS = (1, 3, 4, 20, 64, 68)


def _table():
    cases = []
    i = 0
    for hw in MAPS:                                        # every map x every channel count; batch, activation and noise walk along
        for C in CHANNELS:
            cases.append(((1, 3)[(i + i // 6) % 2],) + hw + (C, ACTS[i % 3], bool((i // 3) % 2)))
            i += 1
    for C in (64, 68):                                     # the largest map under every activation, with and without noise
        for act in ACTS:
            for nz in (False, True):
                cases.append((3 if nz else 1, 64, 64, C, act, nz))
    for act in ACTS:                                       # the generator's first block
        for nz in (False, True):
            cases.append((1 if nz else 3, 4, 4, 512, act, nz))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c); out.append(c)
    return tuple(out)


CASES = _table()                 # (B, H, W, C, act, noise)


def case_id(c):
    return '%dx%dx%dx%d-%s-%s' % (c[0], c[1], c[2], c[3], c[4] or 'none', 'noise' if c[5] else 'plain')


def group_of(c):
    return '%s-%s' % (c[4] or 'none', 'noise' if c[5] else 'plain')


def evaluate(inp, act, dtype, one_pass=False):
    y, cache = forward(inp['x'], inp['ys'], inp['yb'], inp['noise'], inp['strength'], act, dtype, one_pass=one_pass)
    dx, dstrength, dys, dyb = backward(inp['g'], cache, act, dtype)
    return dict(y=y, dx=dx, dstrength=dstrength, dys=dys, dyb=dyb)


FLOORS = dict(y=1e-5, dys=1e-5, dyb=1e-5, dstrength=1e-5, dx=1e-4)       # tests/test_pggan.py's layer-norm bounds
MARGIN = 8.0


def relerr(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def tolerances(ref64, ref32):
    """Per tensor: max(floor, 8 e32), e32 = the float32 numpy evaluation's error against float64, relative to the largest reference entry."""
    return {k: max(FLOORS[k], MARGIN * relerr(ref32[k], ref64[k])) for k in FLOORS if ref64[k] is not None}


@functools.lru_cache(maxsize=None)
def reference(i):
    """(inputs, float64 results, tolerances) of case i; computed once, shared, never modified."""
    B, H, W, C, act, nz = CASES[i]
    inp = inputs((B, H, W, C), nz, act)
    r64 = evaluate(inp, act, np.float64)
    return inp, r64, tolerances(r64, evaluate(inp, act, np.float32))


# ---- the style-based generator, float64 torch (PGGAN(style_dim=D)) -----------------------------------------------------------------
def style_generator(V, cfg, z, cond, stages, t, alpha, ca_noise, style_dim, mapping_layers=4, style_noise=None, w_override=None):
    """-> (img NHWC, mean, log_sigma, w).  oracle/torch_pggan.generator with every conv -> layer_norm(relu) pair replaced by
    conv -> noise -> relu -> instance norm -> style; style_noise: list of [B,H,W] images, one per style block in order, or None."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_pggan as PG
    from oracle.torch_step import lrelu, relu
    V.enter('g_net/conv_stage_0')
    mean = lrelu(V.dense(cond, cfg.compressed, 'he'))
    log_sigma = lrelu(V.dense(cond, cfg.compressed, 'he'))
    code = mean if ca_noise is None else mean + torch.exp(log_sigma) * ca_noise
    zc = torch.cat([z, code], 1)
    x = V.dense(zc, 4 * 4 * cfg.nf(0), 'he')
    x = V.ln(x)
    x = x.reshape(-1, 4, 4, cfg.nf(0)).permute(0, 3, 1, 2)
    # the mapping network: pixel norm of [z, c], then dense + lrelu layers
    V.enter('g_net/mapping')
    w = zc / torch.sqrt((zc * zc).mean(1, keepdim=True) + 1e-8)
    for _ in range(mapping_layers):
        w = lrelu(V.dense(w, style_dim, 'he'))
    if w_override is not None:
        w = w_override(w)
    blocks = [0]

    def style(x, scope):
        k = blocks[0]
        blocks[0] += 1
        name = V._name('StyleMod')
        C = x.shape[1]
        nz = None if style_noise is None else style_noise[k]
        if nz is not None:
            s = V._get(name + '/noise_strength', (C,), 'zeros')
            x = x + s.view(1, -1, 1, 1) * nz[:, None, :, :]
        kern = V._get(name + '/style/kernel', (style_dim, 2 * C), 'he')
        bias = V._get(name + '/style/bias', (2 * C,), 'zeros')
        sty = w @ kern + bias
        u = relu(x)
        mu = u.mean((2, 3), keepdim=True)
        var = ((u - mu) ** 2).mean((2, 3), keepdim=True)
        return (u - mu) / torch.sqrt(var + EPS) * (1.0 + sty[:, :C, None, None]) + sty[:, C:, None, None]

    V.enter('g_net/conv_stage_0')                          # re-entered: only Conv and StyleMod layers follow, whose counts start here
    x = style(V.conv(x, cfg.nf(0), 3, 1, 'SAME', 'he'), None)
    x = style(V.conv(x, cfg.nf(0), 3, 1, 'SAME', 'he'), None)
    x_iden = None
    for i in range(1, stages):
        if i == stages - 1 and t:
            x_iden = PG._to_rgb(V, 'g_net', x, stages - 2, cfg)
            x_iden = F.interpolate(x_iden, scale_factor=2, mode='nearest')
        V.enter('g_net/conv_stage_%d' % i)
        x = F.interpolate(x, scale_factor=2, mode='nearest')
        x = style(V.conv(x, cfg.nf(i), 3, 1, 'SAME', 'he'), None)
        x = style(V.conv(x, cfg.nf(i), 3, 1, 'SAME', 'he'), None)
    x = PG._to_rgb(V, 'g_net', x, stages - 1, cfg)
    if t:
        x = (1.0 - alpha) * x_iden + alpha * x
    return x.permute(0, 2, 3, 1), mean, log_sigma, w


def style_block_sizes(stages):
    """The map extents of the style blocks in order: two per conv stage."""
    return [4 * 2 ** i for i in range(stages) for _ in range(2)]
