"""Restatements for the weight-demodulated convolution (csrc/t2i_modconv.hip): every entry point's forward and
backward in numpy, generic over the dtype; the layer in float64 torch, once by its definition (explicit per-sample filters W s d, a
grouped convolution) and once factorised; the case tables of tests/test_modconv_gpu.py; and a float64 torch restatement of
PGGAN(style_dim=D, modulated_conv=True) on top of oracle/torch_pggan.py's layers.  Test infrastructure only."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHUNK = 64                       # kernels.MODCONV_CHUNK_ROWS (tests/test_modconv_gpu.py asserts the two agree)
ACTS = (None, 'relu', 'lrelu')   # lrelu: slope 0.2
ALPHA = 0.2
EPS = 1e-8
KINK = 1e-3                      # epilogue inputs keep every pre-activation at least this far from the kink of relu / lrelu
MARGIN = 8.0
FLOORS = dict(q=1e-5, d=1e-5, ds=1e-5, dW=1e-5, xs=1e-5, dx=1e-4, out=1e-5, dc=1e-4, dd=1e-5, dbias=1e-5, dstrength=1e-5)


def relerr(got, ref):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def tolerances(ref64, ref32):
    """Per tensor: max(floor, 8 e32), e32 = the float32 numpy evaluation's error against float64, relative to the largest reference entry
    (DESIGN.md section 4.42's rule)."""
    return {k: max(FLOORS[k], MARGIN * relerr(ref32[k], ref64[k])) for k in ref64 if ref64[k] is not None}


def act_np(p, act):
    return p if act is None else np.where(p > 0, p, (0.0 if act == 'relu' else ALPHA) * p)


def dact_np(p, act):
    return np.ones_like(p) if act is None else np.where(p > 0, 1.0, 0.0 if act == 'relu' else ALPHA).astype(p.dtype)


# ---- the demodulation coefficients ----------------------------------------------------------------------------------------------------
def coef(W, s, gd, dtype, eps=EPS):
    """W [T,Cin,Cout], s [B,Cin], gd [B,Cout] -> q, d and the backward's ds, dW, in `dtype`."""
    W, s, gd = (np.asarray(a).astype(dtype) for a in (W, s, gd))
    q = (W * W).sum(0, dtype=dtype)
    d = (1.0 / np.sqrt((s * s) @ q + dtype(eps))).astype(dtype)
    e = dtype(-0.5) * d * d * d * gd
    ds = dtype(2.0) * s * (e @ q.T)
    dW = dtype(2.0) * W * ((s * s).T @ e)[None]
    return dict(q=q, d=d, ds=ds.astype(dtype), dW=dW.astype(dtype))


COEF_CASES = tuple((T, ci, co, B) for T in (1, 9) for (ci, co), B in (
    ((1, 1), 1), ((3, 4), 3), ((4, 3), 1), ((20, 20), 3), ((64, 68), 1), ((68, 64), 3), ((130, 20), 1), ((20, 130), 3), ((64, 64), 3), ((130, 130), 1)))


def coef_inputs(case, zero_row=False):
    T, ci, co, B = case
    rng = np.random.default_rng(17 + 1000 * T + 7 * ci + 131 * co + B)
    W = (rng.standard_normal((T, ci, co)) / np.sqrt(T * ci)).astype(np.float32)
    s = (1.0 + 0.5 * rng.standard_normal((B, ci))).astype(np.float32)
    if zero_row:
        s[B - 1] = 0.0
    gd = rng.standard_normal((B, co)).astype(np.float32)
    return W, s, gd


@functools.lru_cache(maxsize=None)
def coef_reference(i):
    inp = coef_inputs(COEF_CASES[i])
    r64 = coef(*inp, np.float64)
    return inp, r64, tolerances(r64, coef(*inp, np.float32))


# ---- the scale pass ---------------------------------------------------------------------------------------------------------------------
def scale(x, s, g, dtype):
    """x, g [B,H,W,C], s [B,C] -> xs = x s, dx = g s, ds = sum over (h, w) of g x."""
    x, s, g = (np.asarray(a).astype(dtype) for a in (x, s, g))
    return dict(xs=x * s[:, None, None, :], dx=g * s[:, None, None, :], ds=(g * x).sum((1, 2), dtype=dtype))


MAPS = ((1, 1), (4, 4), (3, 5), (7, 9), (8, 8), (5, 13), (3, 43), (33, 31))          # 63, 64, 65 and 129 rows among them: chunk - 1 .. 2 chunk + 1
CHANNELS = (1, 3, 4, 20, 64, 68)
SCALE_CASES = tuple(((1, 3)[(i + j) % 2],) + hw + (C,) for i, hw in enumerate(MAPS) for j, C in enumerate(CHANNELS))


def scale_inputs(case):
    B, H, W, C = case
    rng = np.random.default_rng(23 + 7 * B + 31 * H + 131 * W + 1009 * C)
    return (rng.standard_normal((B, H, W, C)).astype(np.float32), (1.0 + 0.5 * rng.standard_normal((B, C))).astype(np.float32),
            rng.standard_normal((B, H, W, C)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def scale_reference(i):
    inp = scale_inputs(SCALE_CASES[i])
    r64 = scale(*inp, np.float64)
    return inp, r64, tolerances(r64, scale(*inp, np.float32))


# ---- the epilogue -----------------------------------------------------------------------------------------------------------------------
def epilogue(c, d, bias, noise, strength, g, act, dtype):
    """out = act(d c + bias + strength noise) and, for the cotangent g, dc, dd, dbias, dstrength (None where the input is None)."""
    cv = lambda a: None if a is None else np.asarray(a).astype(dtype)
    c, d, bias, noise, strength, g = (cv(a) for a in (c, d, bias, noise, strength, g))
    p = c if d is None else c * d[:, None, None, :]
    if bias is not None:
        p = p + bias
    if noise is not None:
        p = p + strength * noise[..., None]
    gp = dact_np(p, act) * g
    return dict(out=act_np(p, act).astype(dtype), dc=(gp if d is None else gp * d[:, None, None, :]).astype(dtype),
                dd=None if d is None else (gp * c).sum((1, 2), dtype=dtype), dbias=None if bias is None else gp.sum((0, 1, 2), dtype=dtype),
                dstrength=None if noise is None else (gp * noise[..., None]).sum((0, 1, 2), dtype=dtype))


def _epilogue_table():
    out, i = [], 0
    for hw in MAPS:                                        # every map x every channel count; the options walk along
        for C in CHANNELS:
            out.append(((1, 3)[(i + i // 6) % 2],) + hw + (C, ACTS[i % 3], bool((i // 3) % 2), bool((i // 2) % 2), bool((i + i // 4) % 2)))
            i += 1
    for act in ACTS:                                       # every activation with everything present and with everything absent
        for full in (True, False):
            out.append((3, 7, 9, 68, act, full, full, full))
            out.append((1, 3, 43, 3, act, full, not full, full))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c); uniq.append(c)
    return tuple(uniq)


EPI_CASES = _epilogue_table()    # (B, H, W, C, act, noise, d given, bias given)


def epi_id(c):
    return '%dx%dx%dx%d-%s%s%s%s' % (c[0], c[1], c[2], c[3], c[4] or 'none', '-noise' if c[5] else '', '-d' if c[6] else '', '-bias' if c[7] else '')


def epi_inputs(case):
    """float32 inputs; c is moved so that no pre-activation lies within KINK of 0 (the side of the kink must not depend on the precision)."""
    B, H, W, C, act, nz, has_d, has_b = case
    rng = np.random.default_rng(29 + 7 * B + 31 * H + 131 * W + 1009 * C + (3 if nz else 0) + (5 if has_d else 0) + (11 if has_b else 0))
    c = (1.3 * rng.standard_normal((B, H, W, C))).astype(np.float32)
    d = rng.uniform(0.5, 2.0, (B, C)).astype(np.float32) if has_d else None
    bias = (0.5 * rng.standard_normal((C,))).astype(np.float32) if has_b else None
    noise = rng.standard_normal((B, H, W)).astype(np.float32) if nz else None
    strength = rng.uniform(-0.6, 0.6, (C,)).astype(np.float32) if nz else None
    g = rng.standard_normal((B, H, W, C)).astype(np.float32)
    if act is not None:
        f = np.float64
        dd = np.ones((B, 1, 1, C)) if d is None else d.astype(f)[:, None, None, :]
        p = c.astype(f) * dd + (0.0 if bias is None else bias.astype(f)) + (0.0 if noise is None else strength.astype(f) * noise.astype(f)[..., None])
        near = np.abs(p) < KINK
        c = np.where(near, c + (np.float32(4 * KINK) / dd.astype(np.float32)) * np.where(p >= 0, 1, -1), c).astype(np.float32)
    return c, d, bias, noise, strength, g


@functools.lru_cache(maxsize=None)
def epi_reference(i):
    inp, act = epi_inputs(EPI_CASES[i]), EPI_CASES[i][4]
    r64 = epilogue(*inp, act, np.float64)
    return inp, r64, tolerances(r64, epilogue(*inp, act, np.float32))


# ---- the layer, float64 torch -----------------------------------------------------------------------------------------------------------
def _t_act(p, act):
    import torch
    return p if act is None else torch.where(p > 0, p, (0.0 if act == 'relu' else ALPHA) * p)


def layer_definition(x, W, s, bias, noise, strength, act=None, demodulate=True, eps=EPS):
    """The definition: per-sample filters W'[b] = W s[b] (d[b] with demodulate), one convolution per sample (a grouped convolution), bias,
    noise, activation.  x [B,H,W,Cin] NHWC, W [kh,kw,Cin,Cout], s [B,Cin]; torch tensors of one dtype -> [B,H,W,Cout]."""
    import torch
    import torch.nn.functional as F
    B, H, Wd, Cin = x.shape
    kh, kw, _, Cout = W.shape
    Wp = W[None] * s[:, None, None, :, None]                                       # [B,kh,kw,Cin,Cout]
    if demodulate:
        Wp = Wp * torch.rsqrt((Wp * Wp).sum((1, 2, 3), keepdim=True) + eps)
    filt = Wp.permute(0, 4, 3, 1, 2).reshape(B * Cout, Cin, kh, kw)
    xin = x.permute(0, 3, 1, 2).reshape(1, B * Cin, H, Wd)
    pt, pl = (kh - 1) // 2, (kw - 1) // 2                                          # TF 'SAME' at stride 1: the odd pixel goes bottom / right
    y = F.conv2d(F.pad(xin, (pl, kw - 1 - pl, pt, kh - 1 - pt)), filt, groups=B).reshape(B, Cout, H, Wd).permute(0, 2, 3, 1)
    if bias is not None:
        y = y + bias
    if noise is not None:
        y = y + strength * noise[..., None]
    return _t_act(y, act)


def layer_factorised(x, W, s, bias, noise, strength, act=None, demodulate=True, eps=EPS):
    """What the package computes: act(d conv(x s, W) + bias + strength noise), d = rsqrt(sum_i s^2 q + eps), q = sum over the taps of W^2."""
    import torch
    import torch.nn.functional as F
    kh, kw, Cin, Cout = W.shape
    pt, pl = (kh - 1) // 2, (kw - 1) // 2
    xs = (x * s[:, None, None, :]).permute(0, 3, 1, 2)
    y = F.conv2d(F.pad(xs, (pl, kw - 1 - pl, pt, kh - 1 - pt)), W.permute(3, 2, 0, 1)).permute(0, 2, 3, 1)
    if demodulate:
        y = y * torch.rsqrt((s * s) @ (W * W).sum((0, 1)) + eps)[:, None, None, :]
    if bias is not None:
        y = y + bias
    if noise is not None:
        y = y + strength * noise[..., None]
    return _t_act(y, act)


LAYER_CASES = ((1, 4, 4, 8, 8), (3, 5, 7, 20, 12), (2, 8, 8, 64, 68))              # (B, H, W, Cin, Cout), 3x3, w_dim 6
W_DIM = 6


def layer_inputs(case):
    """float32 arrays: x, the style vector w, weights, biases, noise_strength, style kernel and bias, a noise image and a cotangent."""
    B, H, W, Cin, Cout = case
    rng = np.random.default_rng(41 + 7 * B + 31 * H + 131 * W + 1009 * Cin + 17 * Cout)
    f = lambda a: a.astype(np.float32)
    return dict(x=f(rng.standard_normal((B, H, W, Cin))), w=f(rng.standard_normal((B, W_DIM))),
                weights=f(rng.standard_normal((3, 3, Cin, Cout)) * np.sqrt(2.0 / (9 * Cin))), biases=f(0.3 * rng.standard_normal((Cout,))),
                noise_strength=f(rng.uniform(-0.5, 0.5, (Cout,))), kernel=f(rng.standard_normal((W_DIM, Cin)) * 0.3),
                bias=f(0.2 * rng.standard_normal((Cin,))), noise=f(rng.standard_normal((B, H, W))), g=f(rng.standard_normal((B, H, W, Cout))))


def layer_reference(case, act=None, with_grads=True):
    """float64, by the definition: the output and (with_grads) the gradient of sum(out g) to x, w and the five variables."""
    import torch
    inp = layer_inputs(case)
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=k not in ('noise', 'g')) for k, v in inp.items()}
    s = 1.0 + t['w'] @ t['kernel'] + t['bias']
    out = layer_definition(t['x'], t['weights'], s, t['biases'], t['noise'], t['noise_strength'], act)
    if not with_grads:
        return inp, out.detach().numpy(), None
    names = ('x', 'w', 'weights', 'biases', 'noise_strength', 'kernel', 'bias')
    grads = torch.autograd.grad((out * t['g']).sum(), [t[k] for k in names])
    return inp, out.detach().numpy(), {k: g.numpy() for k, g in zip(names, grads)}


# ---- PGGAN(style_dim=D, modulated_conv=True), float64 torch -------------------------------------------------------------------------------
def modconv_generator(V, cfg, z, cond, stages, t, alpha, ca_noise, style_dim, mapping_layers=4, style_noise=None):
    """-> (img NHWC, mean, log_sigma, w).  tests/style_cases.style_generator with every conv -> style block pair replaced by one
    weight-demodulated convolution (by its definition) + bias + noise + relu; style_noise: list of [B,H,W] images, one per layer, or None."""
    import torch
    import torch.nn.functional as F
    from oracle import torch_pggan as PG
    from oracle.torch_step import lrelu
    V.enter('g_net/conv_stage_0')
    mean = lrelu(V.dense(cond, cfg.compressed, 'he'))
    log_sigma = lrelu(V.dense(cond, cfg.compressed, 'he'))
    code = mean if ca_noise is None else mean + torch.exp(log_sigma) * ca_noise
    zc = torch.cat([z, code], 1)
    x = V.ln(V.dense(zc, 4 * 4 * cfg.nf(0), 'he')).reshape(-1, 4, 4, cfg.nf(0))                 # NHWC from here on
    V.enter('g_net/mapping')
    w = zc / torch.sqrt((zc * zc).mean(1, keepdim=True) + 1e-8)
    for _ in range(mapping_layers):
        w = lrelu(V.dense(w, style_dim, 'he'))
    blocks = [0]

    def modconv(x, f):
        k = blocks[0]
        blocks[0] += 1
        name = V._name('ModConv')
        Cin = x.shape[3]
        W = V._get(name + '/weights', (3, 3, Cin, f), 'he')
        b = V._get(name + '/biases', (f,), 'zeros')
        nz = None if style_noise is None else style_noise[k]
        st = V._get(name + '/noise_strength', (f,), 'zeros') if nz is not None else None
        kern = V._get(name + '/style/kernel', (style_dim, Cin), 'he')
        bias = V._get(name + '/style/bias', (Cin,), 'zeros')
        return layer_definition(x, W, 1.0 + w @ kern + bias, b, nz, st, 'relu')

    up = lambda x: F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='nearest').permute(0, 2, 3, 1)
    rgb = lambda x, stage: PG._to_rgb(V, 'g_net', x.permute(0, 3, 1, 2), stage, cfg).permute(0, 2, 3, 1)
    V.enter('g_net/conv_stage_0')                          # re-entered: only ModConv layers follow, whose count starts here
    x = modconv(modconv(x, cfg.nf(0)), cfg.nf(0))
    x_iden = None
    for i in range(1, stages):
        if i == stages - 1 and t:
            x_iden = up(rgb(x, stages - 2))
        V.enter('g_net/conv_stage_%d' % i)
        x = up(x)
        x = modconv(modconv(x, cfg.nf(i)), cfg.nf(i))
    x = rgb(x, stages - 1)
    if t:
        x = (1.0 - alpha) * x_iden + alpha * x
    return x, mean, log_sigma, w


def modconv_variables(cfg, stages, trans, style_dim, mapping_layers=4, noise=True):
    """[(name, shape)] of the restatement's g_net variables in creation order (the model has g_net/mapping/w_avg besides, not trainable)."""
    import torch
    from oracle import torch_pggan as PG
    V = PG.Vars()
    B = 2
    nz = [torch.zeros(B, s, s, dtype=torch.float64) for s in block_sizes(stages)] if noise else None
    modconv_generator(V, cfg, torch.zeros(B, cfg.z_dim, dtype=torch.float64), torch.zeros(B, cfg.embed_dim, dtype=torch.float64), stages, trans, 0.5,
                      None, style_dim, mapping_layers, nz)
    return [(n, tuple(v.shape)) for n, v in V.P.items()]


def block_sizes(stages):
    """The map extents of the modulated convolutions in order: two per conv stage."""
    return [4 * 2 ** i for i in range(stages) for _ in range(2)]
