"""Spectral normalisation, restated in float64 (numpy) for tests/test_spectral_*.py and tests/test_pggan_sn_gpu.py: the power
iteration, W = raw / sigma, the gradient transform and the TF-flavoured Adam step of optim.py's docstring; and the test arena.

A variable of shape [..., C] is the row-major matrix M [R, C], C its last dimension.  nrm(x) = x / max(|x|, 1e-12).

    t = M u;  v = nrm(t);  s = M^T v;  sigma = |s|;  u = nrm(s);  W = raw / max(sigma, 1e-12)
    dL/draw = (G - <G, W> v u^T) / sigma          (u, v constants)"""
from collections import OrderedDict

import numpy as np

TINY = 1e-12
SEED = 20180215
WARMUP = 15

# name -> shape, in arena order.  [40, 1]: C = 1, sigma = |w|.  [7, 5]: 35 elements, a padded slot.  [4, 4, 128, 64]: R = 2048 rows, 16 work
# items, so the column sums take more than one partial; [3, 3, 64, 128]: 9 work items of 64 rows.  The bias and gamma are not normalised.
ARENA = OrderedDict([
    ('d_net/a/weights', (1, 1, 3, 16)),
    ('d_net/b/weights', (3, 3, 16, 32)),
    ('d_net/a/biases', (16,)),
    ('d_net/c/weights', (4, 4, 32, 8)),
    ('d_net/fc/kernel', (40, 1)),
    ('d_net/b/gamma', (32,)),
    ('d_net/odd/kernel', (7, 5)),
    ('d_net/rgb/weights', (1, 1, 16, 3)),
    ('d_net/one/weights', (1, 1, 1, 1)),
    ('d_net/d/weights', (3, 3, 64, 128)),
    ('d_net/e/weights', (4, 4, 128, 64)),
])
NORMALISED = [n for n, s in ARENA.items() if len(s) >= 2]
ALONE = 'd_net/b/weights'


def matrix_shape(shape):
    C = int(shape[-1])
    return int(np.prod(shape)) // C, C


def arena_values(seed=SEED):
    """name -> float32 array, He-scaled Gaussians (the critic's initialisation); biases small, gamma near 1."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for n, s in ARENA.items():
        if len(s) >= 2:
            R, _ = matrix_shape(s)
            out[n] = (rng.standard_normal(s) * np.sqrt(2.0 / R)).astype(np.float32)
        elif n.endswith('gamma'):
            out[n] = (1.0 + 0.1 * rng.standard_normal(s)).astype(np.float32)
        else:
            out[n] = (0.1 * rng.standard_normal(s)).astype(np.float32)
    return out


def arena_grads(seed=SEED + 1):
    rng = np.random.default_rng(seed)
    return OrderedDict((n, rng.standard_normal(s).astype(np.float32)) for n, s in ARENA.items())


def nrm(x):
    return x / max(float(np.sqrt(np.sum(x * x))), TINY)


def first_u(C, rng):
    return nrm(rng.standard_normal(C))


def iterate(M, u, iterations=1):
    """-> (u, v, sigma) after `iterations` power iterations of the [R, C] float64 matrix M from u [C]."""
    M, u = np.asarray(M, np.float64), np.asarray(u, np.float64)
    v, sigma = None, None
    for _ in range(iterations):
        v = nrm(M @ u)
        s = M.T @ v
        sigma = float(np.sqrt(np.sum(s * s)))
        u = nrm(s)
    return u, v, sigma


def normalised(raw, sigma):
    return np.asarray(raw, np.float64) / max(sigma, TINY)


def grad_raw(G, W, u, v, sigma):
    """dL/draw from G = dL/dW for W = raw / sigma, sigma = v^T raw u with u, v constants; G, W of the variable's or the matrix's shape."""
    G, W = np.asarray(G, np.float64), np.asarray(W, np.float64)
    shape = G.shape
    R, C = matrix_shape(shape)
    G2, W2 = G.reshape(R, C), W.reshape(R, C)
    return ((G2 - np.sum(G2 * W2) * np.outer(v, u)) / sigma).reshape(shape)


def adam_tf(w, g, v, t, lr, beta1=0.0, beta2=0.99, eps=1e-8, m=None, grad_scale=1.0, grad_mult=1.0, lr_mult=1.0):
    """optim.AdamTF: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); m, v updates; w -= lr_t m / (sqrt(v) + eps), epsilon outside the bias
    correction.  -> (w, m, v), float64."""
    w, g, v = np.asarray(w, np.float64), np.asarray(g, np.float64) * grad_scale * grad_mult, np.asarray(v, np.float64)
    m = np.zeros_like(w) if m is None else np.asarray(m, np.float64)
    lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t) * lr_mult
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return w - lr_t * m / (np.sqrt(v) + eps), m, v


def relerr(got, ref, floor=1e-30):
    """max-norm relative error per tensor"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), floor))
