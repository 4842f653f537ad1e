"""The row-wise kernels, the fade-in, the conditioning augmentation and the WGAN critic head of csrc/t2i_aux.hip restated in plain
float64 NumPy, one statement per line, with the inputs of tests/test_row_heads_host.py and tests/test_row_heads_gpu.py.

Every restatement takes float64 arrays (the tests hand it the float32 inputs of the kernel, widened exactly) and follows the
definition, not the kernel: no chunks, no vector paths, no fixed summation order.  The host tests check the restatements of the
head and of the conditioning augmentation against float64 autograd of the reference's expressions (oracle/torch_step.py), so that
the GPU tests do not compare a kernel with a copy of itself."""
import numpy as np
import torch

D_HEAD_KEYS = ('D_loss', 'D_loss_real', 'D_loss_fake', 'D_loss_mismatch', 'wdist', 'wdist2', 'real_gp', 'real_gp2', 'reg_loss',
               'balance_loss', 'kt_grad', 'kt')


def f64(t):
    """a float32 tensor / array widened to float64 NumPy (exact)"""
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


# ---- the critic head (reference models/wgancls/model.py:72-92) -------------------------------------------------------------
def d_head(logits, s1, s2, kt, gp_coeff):
    """logits [3B] (fake | real | mismatch), slopes [B] each, kt a float (1.0 where the model has none)
    -> ({key: float} over D_HEAD_KEYS, dD_loss/dlogits [3B], dD_loss/ds1 [B], dD_loss/ds2 [B])"""
    B = s1.size
    fake = logits[:B].mean()
    real = logits[B:2 * B].mean()
    mis = logits[2 * B:].mean()
    wdist = real - fake
    wdist2 = real - mis
    h1 = np.maximum(0.0, s1 - 1.0)
    h2 = np.maximum(0.0, s2 - 1.0)
    gp1 = (h1 ** 2).mean()
    gp2 = (h2 ** 2).mean()
    reg = (logits[2 * B:] ** 2).mean()
    bal = kt * wdist2 - wdist
    D_loss = -wdist - kt * wdist2 + gp_coeff * (gp1 + gp2)
    scal = dict(D_loss=D_loss, D_loss_real=real, D_loss_fake=fake, D_loss_mismatch=mis, wdist=wdist, wdist2=wdist2, real_gp=gp1,
                real_gp2=gp2, reg_loss=reg, balance_loss=bal ** 2, kt_grad=2.0 * bal * wdist2, kt=kt)
    seed_l = np.concatenate([np.full(B, 1.0 / B), np.full(B, -(1.0 + kt) / B), np.full(B, kt / B)])
    seed_s1 = gp_coeff * 2.0 * h1 / B
    seed_s2 = gp_coeff * 2.0 * h2 / B
    return scal, seed_l, seed_s1, seed_s2


HINGE_AT_ONE = {'s1': 0, 's2': -1}          # where head_inputs puts a slope of exactly 1.0


def head_inputs(B, seed=0):
    """float32 (logits [3B], s1 [B], s2 [B]).  The three logit groups have means -3 | 5 | 1 (a swapped group shows); the two slope
    vectors are drawn apart (U(0.2, 2.6) and U(0.1, 1.9): a swapped pair shows) and each holds an active hinge, an inactive one and
    one at exactly 1.0 where B allows it.  B = 1 holds one hinge per vector: the seed picks which kinds."""
    rs = np.random.RandomState(700 + 13 * B + seed)
    logits = np.concatenate([rs.standard_normal(B) - 3.0, rs.standard_normal(B) + 5.0, rs.standard_normal(B) + 1.0])
    s1, s2 = rs.uniform(0.2, 2.6, B), rs.uniform(0.1, 1.9, B)
    if B >= 3:
        s1[0], s1[1], s1[2] = 1.0, 0.4, 1.9
        s2[-1], s2[0], s2[1] = 1.0, 2.3, 0.7
    else:
        s1[0], s2[-1] = ((1.0, 1.8), (0.6, 1.0), (1.7, 0.3), (2.2, 1.4))[seed % 4]
    return logits.astype(np.float32), s1.astype(np.float32), s2.astype(np.float32)


# ---- conditioning augmentation (reference models/wgancls/model.py:117-127) -------------------------------------------------
def ca_kl_terms(mean, log_sigma):
    """the summands of the KL term, each >= 0"""
    return -log_sigma + 0.5 * (-1.0 + np.exp(2.0 * log_sigma) + mean ** 2)


def ca_fwd(mean, log_sigma, eps):
    code = mean + np.exp(log_sigma) * eps
    kl = ca_kl_terms(mean, log_sigma).mean()
    return code, kl


def ca_bwd(mean, log_sigma, eps, dcode, dkl):
    """(dmean, dlog_sigma) for the cotangents dcode (array or None) and dkl (float or None) of (code, kl)"""
    n = mean.size
    dcode = np.zeros_like(mean) if dcode is None else dcode
    dkl = 0.0 if dkl is None else dkl
    dmean = dcode + dkl * mean / n
    dls = dcode * eps * np.exp(log_sigma) + dkl * (np.exp(2.0 * log_sigma) - 1.0) / n
    return dmean, dls


def ca_inputs(n, seed=0):
    """float32 (mean ~ N(0,1), log_sigma ~ U(-3, 1), eps ~ N(0,1)), flat [n]"""
    rs = np.random.RandomState(4000 + n % 997 + seed)
    return rs.standard_normal(n).astype(np.float32), rs.uniform(-3.0, 1.0, n).astype(np.float32), rs.standard_normal(n).astype(np.float32)


# ---- fade-in ---------------------------------------------------------------------------------------------------------------
def lerp(a, b, t, mode):
    if mode == 0:
        return (1.0 - t) * a + t * b
    if mode == 1:
        return t * a
    return (1.0 - t) * a


# ---- per-sample kernels ----------------------------------------------------------------------------------------------------
def row_moments(a, b=None):
    """a, b [B, per] -> (s1 [B], s2 [B], sum |a| [B], sum |a b| [B]): the sums and the sums of the absolute terms that bound them"""
    b = a if b is None else b
    return a.sum(1), (a * b).sum(1), np.abs(a).sum(1), np.abs(a * b).sum(1)


def row_fma2(a, alpha, b=None, gamma=None, delta=None):
    out = a * alpha[:, None]
    if b is not None:
        out = out + b * gamma[:, None]
    if delta is not None:
        out = out + delta[:, None]
    return out


def pool2_sum(x, scale):
    B, H, W, C = x.shape
    return scale * x.reshape(B, H // 2, 2, W // 2, 2, C).sum((2, 4))


def upscale2(x, scale):
    return scale * x.repeat(2, axis=1).repeat(2, axis=2)


def layer_norm(x, gamma, beta, dy, eps=1e-12):
    """tf.contrib.layers.layer_norm(begin_norm_axis=1, begin_params_axis=-1), two-pass variance, by float64 autograd
    -> (y, dx, dgamma, dbeta) for the cotangent dy; all arguments float64 torch tensors"""
    x, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    dims = tuple(range(1, x.dim()))
    mu = x.mean(dims, keepdim=True)
    var = ((x - mu) ** 2).mean(dims, keepdim=True)
    y = (x - mu) / torch.sqrt(var + eps) * gamma + beta
    dx, dgamma, dbeta = torch.autograd.grad(y, [x, gamma, beta], dy)
    return y.detach(), dx, dgamma, dbeta


# ---- gradient penalty ------------------------------------------------------------------------------------------------------
def gp_slopes(g):
    """g [B, per] -> (sum g^2 [B], its root)"""
    ss = (g ** 2).sum(1)
    return ss, np.sqrt(ss)


def row_scale(g, coef):
    return coef[:, None] * g


def row_scale_div(g, num, den):
    """the slope norm's backward with its guard: coefficient num / max(den, 1e-30) where den > 0, else 0 (1e-30 as float32 holds it)"""
    floor = float(np.float32(1e-30))
    coef = np.where(den > 0, num / np.maximum(den, floor), 0.0)
    return coef[:, None] * g


def interp(eps, g, x):
    return eps[:, None] * g + (1.0 - eps[:, None]) * x


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def gaussian(shape, seed, offset=0.5, scale=1.7):
    """float32 N(offset, scale^2)"""
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(shape) * scale + offset).astype(np.float32)


def integers(shape, seed, lo=-8, hi=8):
    """float32 small integers: sums and products with power-of-two scalars are exact in float32"""
    return np.random.RandomState(seed).randint(lo, hi + 1, shape).astype(np.float32)


POW2 = (1.0, -2.0, 0.5, -1.0, 2.0)


def pow2_rows(B, stride):
    """float32 [B] from POW2; with strides 1, 5 and 25 the triple (alpha, gamma, delta) of a row differs from every other row's below
    B = 125, and neighbouring rows always differ in alpha"""
    return np.array([POW2[(r // stride) % 5] for r in range(B)], np.float32)
