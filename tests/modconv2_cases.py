"""Restatements for the second-order entry points of the weight-demodulated convolution (csrc/t2i_modconv.hip):
the backward of every first-order backward in numpy, generic over the dtype, over the case tables of tests/modconv_cases.py (imported, not
repeated), and the composed layer's path-length gradient in float64 torch by the definition.  Test infrastructure only."""
import functools

import numpy as np

import modconv_cases as MC

EPI_CASES, SCALE_CASES, COEF_CASES, LAYER_CASES = MC.EPI_CASES, MC.SCALE_CASES, MC.COEF_CASES, MC.LAYER_CASES
# the first-order floors: 1e-4 for planes, 1e-5 for [B,C] sums and the W term
FLOORS = dict(gg=1e-4, gc=1e-4, gx=1e-4, gd=1e-5, gs=1e-5, ggd=1e-5, gdd=1e-5, gW=1e-5)


def tolerances(ref64, ref32):
    """MC.tolerances' rule with this file's floors: max(floor, 8 e32)."""
    return {k: max(FLOORS[k], MC.MARGIN * MC.relerr(ref32[k], ref64[k])) for k in ref64 if ref64[k] is not None}


# ---- the epilogue -----------------------------------------------------------------------------------------------------------------------
def epilogue2(c, d, bias, noise, strength, g, vc, vd, act, dtype):
    """The first backward gave dc = m g d and dd = sum_r m g c, m = act'(p).  For the cotangents vc of dc and vd of dd (each may be None):
    gg = m (d vc + c vd) to g, gc = m g vd to c, gd = sum_r m g vc to d."""
    cv = lambda a: None if a is None else np.asarray(a).astype(dtype)
    c, d, bias, noise, strength, g, vc, vd = (cv(a) for a in (c, d, bias, noise, strength, g, vc, vd))
    assert vd is None or d is not None
    dfull = None if d is None else d[:, None, None, :]
    p = c if d is None else c * dfull
    if bias is not None:
        p = p + bias
    if noise is not None:
        p = p + strength * noise[..., None]
    m = MC.dact_np(p, act).astype(dtype)
    gg = np.zeros_like(c)
    if vc is not None:
        gg = gg + (vc if d is None else dfull * vc)
    if vd is not None:
        gg = gg + c * vd[:, None, None, :]
    return dict(gg=(m * gg).astype(dtype), gc=None if vd is None else (m * g * vd[:, None, None, :]).astype(dtype),
                gd=None if (vc is None or d is None) else (m * g * vc).sum((1, 2), dtype=dtype))


def epi_cotangents(case):
    B, H, W, C = case[:4]
    rng = np.random.default_rng(7919 + 7 * B + 31 * H + 131 * W + 1009 * C + len(MC.epi_id(case)))
    vc = rng.standard_normal((B, H, W, C)).astype(np.float32)
    vd = rng.standard_normal((B, C)).astype(np.float32) if case[6] else None
    return vc, vd


@functools.lru_cache(maxsize=None)
def epi_reference(i):
    case = EPI_CASES[i]
    inp, (vc, vd) = MC.epi_inputs(case), epi_cotangents(case)
    r64 = epilogue2(*inp, vc, vd, case[4], np.float64)
    return inp, (vc, vd), r64, tolerances(r64, epilogue2(*inp, vc, vd, case[4], np.float32))


# ---- the scale pass ---------------------------------------------------------------------------------------------------------------------
def scale2(x, s, g, vx, vs, dtype):
    """The first backward gave dx = g s and ds = sum_r g x.  For the cotangents vx of dx and vs of ds (each may be None):
    gg = s vx + x vs to g, gx = g vs to x, gs = sum_r vx g to s."""
    cv = lambda a: None if a is None else np.asarray(a).astype(dtype)
    x, s, g, vx, vs = (cv(a) for a in (x, s, g, vx, vs))
    gg = np.zeros_like(x)
    if vx is not None:
        gg = gg + s[:, None, None, :] * vx
    if vs is not None:
        gg = gg + x * vs[:, None, None, :]
    return dict(gg=gg.astype(dtype), gx=None if vs is None else (g * vs[:, None, None, :]).astype(dtype),
                gs=None if vx is None else (vx * g).sum((1, 2), dtype=dtype))


def scale_cotangents(case):
    B, H, W, C = case
    rng = np.random.default_rng(104729 + 7 * B + 31 * H + 131 * W + 1009 * C)
    return rng.standard_normal((B, H, W, C)).astype(np.float32), rng.standard_normal((B, C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scale_reference(i):
    inp, (vx, vs) = MC.scale_inputs(SCALE_CASES[i]), scale_cotangents(SCALE_CASES[i])
    r64 = scale2(*inp, vx, vs, np.float64)
    return inp, (vx, vs), r64, tolerances(r64, scale2(*inp, vx, vs, np.float32))


# ---- the coefficients -------------------------------------------------------------------------------------------------------------------
def coef2(W, s, gd, vs, dtype, eps=MC.EPS):
    """The first backward gave ds = 2 s sum_o q e, e = -d^3 gd / 2, with d an input of its own.  For the cotangent vs of ds, with
    r = sum_i vs s q:  ggd = -d^3 r to gd, gdd = -3 d^2 gd r to d, gs = 2 vs sum_o q e to s, gW = 4 W sum_b vs s e to W."""
    W, s, gd, vs = (np.asarray(a).astype(dtype) for a in (W, s, gd, vs))
    q = (W * W).sum(0, dtype=dtype)
    d = (1.0 / np.sqrt((s * s) @ q + dtype(eps))).astype(dtype)
    e = dtype(-0.5) * d * d * d * gd
    r = (vs * s) @ q
    return dict(ggd=(-(d * d * d) * r).astype(dtype), gdd=(dtype(-3.0) * d * d * gd * r).astype(dtype), gs=(dtype(2.0) * vs * (e @ q.T)).astype(dtype),
                gW=(dtype(4.0) * W * ((vs * s).T @ e)[None]).astype(dtype))


def coef_cotangent(case):
    T, ci, co, B = case
    return np.random.default_rng(15485863 + 1000 * T + 7 * ci + 131 * co + B).standard_normal((B, ci)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def coef_reference(i):
    inp, vs = MC.coef_inputs(COEF_CASES[i]), coef_cotangent(COEF_CASES[i])
    r64 = coef2(*inp, vs, np.float64)
    return inp, vs, r64, tolerances(r64, coef2(*inp, vs, np.float32))


# ---- the layer, float64 torch -------------------------------------------------------------------------------------------------------------
LAYER_NAMES = ('x', 'w', 'weights', 'biases', 'noise_strength', 'kernel', 'bias')


def layer_path_length(case, fn=None, act=None):
    """float64: J = d sum(out g) / dw [B, w_dim] by `fn` (MC.layer_definition by default) and the gradient of sum(J^2) to x, w and the five
    variables (zeros where the sum does not depend on one: biases and noise_strength without a curved activation)."""
    import torch
    inp = MC.layer_inputs(case)
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=k not in ('noise', 'g')) for k, v in inp.items()}
    s = 1.0 + t['w'] @ t['kernel'] + t['bias']
    out = (fn or MC.layer_definition)(t['x'], t['weights'], s, t['biases'], t['noise'], t['noise_strength'], act)
    J, = torch.autograd.grad((out * t['g']).sum(), [t['w']], create_graph=True)
    grads = torch.autograd.grad((J * J).sum(), [t[k] for k in LAYER_NAMES], allow_unused=True)
    return inp, J.detach().numpy(), {k: (np.zeros(t[k].shape) if g is None else g.numpy()) for k, g in zip(LAYER_NAMES, grads)}
