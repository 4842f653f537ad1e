"""The kernels behind the published IS / FID / IMD figures — csrc/t2i_eval.hip (InceptionV3's pools and concatenation, the FID Gram
accumulator) and csrc/t2i_incep_train.hip (pool + dropout, the softmax head, the gradient scatter, RMSProp) — restated in plain
NumPy, one statement per line, with the case tables of tests/test_incep_kernels_host.py and tests/test_incep_kernels_gpu.py.

Every restatement follows the definition, not the kernel: no chunks, no vector paths, no fixed summation order.  They take the
float32 inputs of the kernel and widen them exactly to float64, except where the definition itself names a float32 rounding (the
Gram accumulator's differences, the dropout's floor(keep + u), the scatter's three operations).  The host tests check each against
an independent float64 statement, so that the GPU tests do not compare a kernel with a copy of itself.

The tables name the smallest shapes that reach each dispatch branch.  Two things they cannot reach:
  * the `q hi` word of the dropout's Philox counter: it is non-zero only from quad 2^32 on, a [B, D] of at least 2^34 elements;
  * device-side label validation: head_fwd_kernel indexes LDS with labels[b] unchecked, so a label outside [0, C) is an
    out-of-bounds access, and no test may pass one."""
import numpy as np
import torch

from ada_cases import philox4x32_10, u01

EPS32 = float(np.finfo(np.float32).eps)
MAX_SCATTER_BRANCHES = 8                  # T2I_MAX_SCATTER_BRANCHES (the host test checks it against the header)
POOL_MAX, POOL_AVG = 0, 1                 # T2I_POOL_MAX, T2I_POOL_AVG


def f64(t):
    """a float32 tensor / array widened to float64 NumPy (exact)"""
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


# ---- measured errors against their bounds ------------------------------------------------------------------------------------
def relerr(got, ref):
    """max-norm relative error over the whole array"""
    got, ref = f64(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def relerr_cols(got, ref, floor=0.0):
    """[..., C]: the largest over columns c of (column c's max error) / max(column c's own max |ref|, floor), so that a wrong
    column of a rare class is not hidden behind the scale of a frequent one.  A column whose reference is all zero (and whose
    floor is 0) must be all zero."""
    got, ref = f64(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    C = ref.shape[-1]
    err = np.abs(got - ref).reshape(-1, C).max(0)
    scale = np.maximum(np.abs(ref).reshape(-1, C).max(0), floor)
    return float(np.where(err == 0.0, 0.0, err / np.maximum(scale, 1e-300)).max())


def relerr_rows(got, ref, floor=0.0):
    """[B, ...]: the same per leading row"""
    got, ref = f64(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    B = ref.shape[0]
    return relerr_cols(got.reshape(B, -1).T, ref.reshape(B, -1).T, floor)


def mismatches(got, ref):
    """how many elements differ bit for bit from the float64 reference (0 = equal); shapes must agree"""
    got, ref = f64(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return int((got != ref).sum())


class Report(object):
    """The measured errors of one case against their bounds: all printed (pytest -s), all failures reported together."""

    def __init__(self, case):
        self.case, self.seen, self.bad = case, [], []

    def check(self, name, err, tol):
        self.seen.append((name, err, tol))
        if not err <= tol:
            self.bad.append((name, err, tol))

    def exact(self, name, got, ref):
        """bit for bit: the measured figure is the number of differing elements, the bound 0"""
        self.check(name, float(mismatches(got, ref)), 0.0)

    def done(self):
        print('  case %s: %s' % (self.case, ', '.join('%s %.2e/%.0e' % t for t in self.seen)))
        assert not self.bad, (self.case, self.bad)


# ---- t2i_pool2d ----------------------------------------------------------------------------------------------------------------
def tf_geometry(n, k, s, padding):
    """one axis of tf.nn.max_pool / avg_pool -> (output length, pad before, pad after); SAME puts the odd pixel after"""
    if padding == 'SAME':
        out = -(-n // s)
        total = max((out - 1) * s + k - n, 0)
        return out, total // 2, total - total // 2
    return (n - k) // s + 1, 0, 0


def pool_sum_count(x, KH, KW, SH, SW, padding):
    """x [B, H, W, C] -> (float64 sum of the in-bounds taps [B, Ho, Wo, C], their number [Ho, Wo])"""
    x = f64(x)
    B, H, W, C = x.shape
    Ho, pt, _ = tf_geometry(H, KH, SH, padding)
    Wo, pl, _ = tf_geometry(W, KW, SW, padding)
    total = np.zeros((B, Ho, Wo, C))
    count = np.zeros((Ho, Wo), np.int64)
    for oy in range(Ho):
        for ox in range(Wo):
            for i in range(KH):
                for j in range(KW):
                    iy, ix = oy * SH - pt + i, ox * SW - pl + j
                    if 0 <= iy < H and 0 <= ix < W:
                        total[:, oy, ox] += x[:, iy, ix]
                        count[oy, ox] += 1
    return total, count


def pool(x, KH, KW, SH, SW, padding, op):
    """TF max / average pooling of x [B, H, W, C] -> float64 [B, Ho, Wo, C].  MAX ignores out-of-bounds taps; AVG divides by the
    number of in-bounds taps."""
    if op == POOL_AVG:
        total, count = pool_sum_count(x, KH, KW, SH, SW, padding)
        return total / count[None, :, :, None]
    x = f64(x)
    B, H, W, C = x.shape
    Ho, pt, _ = tf_geometry(H, KH, SH, padding)
    Wo, pl, _ = tf_geometry(W, KW, SW, padding)
    out = np.full((B, Ho, Wo, C), -np.inf)
    for oy in range(Ho):
        for ox in range(Wo):
            for i in range(KH):
                for j in range(KW):
                    iy, ix = oy * SH - pt + i, ox * SW - pl + j
                    if 0 <= iy < H and 0 <= ix < W:
                        out[:, oy, ox] = np.maximum(out[:, oy, ox], x[:, iy, ix])
    return out


def avg_quotient_f32(total, count):
    """the IEEE float32 quotient np.float32(sum) / np.float32(count), where the sum is exact in float32"""
    return total.astype(np.float32) / count.astype(np.float32)[None, :, :, None]


# (B, H, W, KH, KW, SH, SW, padding)
POOL_GEOMETRIES = (
    (1, 5, 7, 3, 2, 1, 2, 'SAME'),        # rectangular window
    (2, 6, 5, 1, 3, 2, 1, 'VALID'),       # rectangular window
    (1, 4, 4, 5, 5, 1, 1, 'SAME'),        # window larger than the map: every output has padded taps
    (1, 3, 9, 3, 3, 3, 4, 'SAME'),        # the largest admitted strides
    (3, 8, 8, 3, 3, 1, 1, 'SAME'),        # Inception's in-block average
    (1, 9, 9, 3, 3, 2, 2, 'VALID'),       # its reduction pools
    (1, 8, 8, 8, 8, 1, 1, 'VALID'),       # global pool, 1x1 output
    (2, 9, 8, 4, 4, 3, 3, 'SAME'),        # kept from tests/test_eval_gpu.py
)

# (name, C, slice (ld, c0) or None, x offset by one float, the kernel form it must reach)
POOL_CLASSES = (
    ('c3', 3, None, False, 'scalar'),
    ('c8', 8, None, False, 'vector'),
    ('c12', 12, None, False, 'vector'),                 # 576 work items on the 3x8x8 case: a ragged last block
    ('c8_ld12_c4', 8, (12, 4), False, 'vector'),
    ('c8_ld13_c4', 8, (13, 4), False, 'scalar'),        # by ld
    ('c8_ld16_c2', 8, (16, 2), False, 'scalar'),        # by c0
    ('c8_xoff', 8, None, True, 'scalar'),               # by the alignment of x
)
POOL_KINDS = ('negative', 'integer')
SENTINEL = 7.0                                          # what a slice test fills the wider buffer with


def pool_form(C, ld, c0, x_aligned16=True):
    """the form pool2d_launch / channel_slice_copy_launch pick (the table's last column is checked against this on the host)"""
    return 'vector' if C % 4 == 0 and ld % 4 == 0 and c0 % 4 == 0 and x_aligned16 else 'scalar'


def pool_input(shape, kind, seed):
    """float32 [B, H, W, C].  'negative': a Gaussian cut at 2.5 sigma, minus 3, so every value is negative and a padded tap read as
    0 wins every maximum it enters.  'integer': integers in -4..4, whose window sums are exact in float32."""
    rs = np.random.RandomState(seed)
    if kind == 'negative':
        return (np.minimum(rs.standard_normal(shape), 2.5) - 3.0).astype(np.float32)
    return rs.randint(-4, 5, shape).astype(np.float32)


def pool_seed(g, C):
    return 1000 + 37 * POOL_GEOMETRIES.index(tuple(g)) + C


# ---- t2i_channel_slice_copy ------------------------------------------------------------------------------------------------------
def slice_copy(x, y, c0):
    """x [rows, C] into channels [c0, c0 + C) of a copy of y [rows, ld]"""
    out = np.array(y)
    out[..., c0:c0 + x.shape[-1]] = x
    return out


# (rows, C, ld, c0, x offset by one float, form); rows * C / 4 is never a multiple of 256
SLICE_COPY_CASES = (
    (70, 8, 13, 5, False, 'scalar'),
    (70, 8, 16, 2, False, 'scalar'),
    (70, 8, 16, 4, True, 'scalar'),
    (70, 3, 10, 5, False, 'scalar'),
    (131, 8, 16, 8, False, 'vector'),     # 262 float4: a ragged second block
    (37, 64, 256, 64, False, 'vector'),   # 592 float4: a ragged third block
)


# ---- t2i_gram_accumulate ---------------------------------------------------------------------------------------------------------
def gram(X, s, G0, sum0):
    """X [n, d], s [d] float32; G0 [d, d], sum0 [d] float64 -> (G0 + (X - s)^T (X - s), sum0 + (X - s).sum(0)).  The differences
    are taken in float32 first, as the header states; everything after that is float64."""
    diff = (np.asarray(X, np.float32) - np.asarray(s, np.float32)[None, :]).astype(np.float64)
    return np.asarray(G0, np.float64) + diff.T @ diff, np.asarray(sum0, np.float64) + diff.sum(0)


GRAM_DIMS = (1, 31, 32, 33, 64, 65, 100)
# row counts of the calls into one accumulator: below, at and one past the 64-row flush, an odd tail, several calls
GRAM_SEQUENCES = ((1,), (2,), (64,), (65,), (63, 1), (17, 130))
GRAM_FLUSH = 64                           # kGramFlush: rows summed in float32 before each float64 flush


def gram_inputs(d, seq, seed=0):
    """integer-valued (X of each call float32 [n_i, d] in -8..8, s float32 [d] in +-1..3 (never 0), G0 [d, d] and sum0 [d] float64
    in -50..50, never 0): every float32 difference, every product and every sum below is exact"""
    rs = np.random.RandomState(5000 + 101 * d + 7 * GRAM_SEQUENCES.index(tuple(seq)) + seed)
    Xs = [rs.randint(-8, 9, (n, d)).astype(np.float32) for n in seq]
    s = (rs.randint(1, 4, d) * rs.choice([-1, 1], d)).astype(np.float32)
    G0 = (rs.randint(1, 51, (d, d)) * rs.choice([-1, 1], (d, d))).astype(np.float64)
    sum0 = (rs.randint(1, 51, d) * rs.choice([-1, 1], d)).astype(np.float64)
    return Xs, s, G0, sum0


# ---- t2i_pool_dropout ------------------------------------------------------------------------------------------------------------
def dropout_mask(seed, step, B, D, keep):
    """float32 [B, D] of 0 / 1: the four elements of quad q = (b * D + d) // 4 take the four words of Philox4x32-10 with counter
    (q lo, q hi, step lo, step hi) and key (seed lo, seed hi); u = (r >> 8) * 2^-24; mask = floor(fl32(keep + u))"""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    q = np.arange(B * D // 4, dtype=np.uint64)
    lo = np.uint64(0xffffffff)
    counter = np.stack([q & lo, q >> np.uint64(32), np.full_like(q, step & 0xffffffff), np.full_like(q, step >> 32)], -1)
    key = np.array([seed & 0xffffffff, seed >> 32], np.uint64)
    u = u01(philox4x32_10(counter, key))
    total = np.float32(keep) + u
    assert total.dtype == np.float32
    return np.floor(total).reshape(B, D)


def pool_mean(x):
    """x [B, HW, D] -> (float64 sum over HW [B, D], float64 mean)"""
    total = f64(x).sum(1)
    return total, total / x.shape[1]


# (B, HW, D, keep)
DROPOUT_SHAPES = (
    (1, 1, 4, 0.8),
    (3, 5, 172, 0.8),                     # 129 quads: less than one block
    (5, 4, 1028, 0.5),                    # 1285 quads: a ragged sixth block
    (2, 64, 2048, 0.8),                   # the workload's map and width
    (3, 5, 172, 1.0),                     # keep = 1: the mask is all ones
)
DROPOUT_STREAMS = ((5, 10), (2 ** 32 + 5, 10), (5, 2 ** 32 + 10), (2 ** 63 + 1, 2 ** 40))      # (seed, step)


# ---- t2i_softmax_ce_head ---------------------------------------------------------------------------------------------------------
def head(y, W, b, labels):
    """logits = y W + b, softmax, mean sparse cross-entropy through a stable log-softmax (an underflowed label probability stays a
    finite loss), accuracy by the first maximum, and the gradients of the loss: dz = (prob - onehot) / B, dW, db, dy"""
    y, W, b = f64(y), f64(W), f64(b)
    labels = np.asarray(labels).astype(np.int64)
    B = len(y)
    rows = np.arange(B)
    logits = y @ W + b
    shifted = logits - logits.max(1, keepdims=True)
    logp = shifted - np.log(np.exp(shifted).sum(1, keepdims=True))
    prob = np.exp(logp)
    loss = float(np.mean(-logp[rows, labels]))
    correct = int((np.argmax(logits, 1) == labels).sum())
    acc = correct / B
    dz = prob.copy()
    dz[rows, labels] -= 1.0
    dz /= B
    return dict(logits=logits, prob=prob, loss=loss, acc=acc, correct=correct, dz=dz, dW=y.T @ dz, db=dz.sum(0), dy=dz @ W.T)


# (B, D, C).  The last two are the admitted corners: (D + C) * 4 = 65536 bytes of LDS in the forward kernel, and B * C * 4 = 65536
# in the backward kernel
HEAD_SHAPES = ((1, 1, 1), (1, 64, 2), (3, 63, 3), (2, 65, 5), (5, 257, 7), (64, 2048, 50), (16, 2048, 1000), (2, 16380, 4), (16, 8, 1024))
HEAD_KINDS = ('unit', 'wide')
HEAD_ACCUMULATE_SHAPES = ((3, 63, 3), (5, 257, 7), (64, 2048, 50))
HEAD_LDS_LIMIT = 65536                    # bytes of dynamic LDS a launch gets without hipFuncAttributeMaxDynamicSharedMemorySize


def head_inputs(B, D, C, kind):
    """float32 (y [B, D], W [D, C], b [C]) and int32 labels [B].
    'unit': logits about N(0, 1).  'wide': W scaled so that logits are about N(0, 30^2), spanning +-60 at two sigma; where B >= 4
    row 2 is labelled with its smallest logit, whose probability underflows in float32 (the host test asserts that one does).
    Labels hold class 0 (row 0) and class C - 1 (row 1).  Where B, C >= 2 the last row of y is zero and the bias has its maximum
    twice, at classes t and C - 1 with t = (C - 1) // 2: that row's logits are the bias exactly, in any arithmetic, its maximum is a
    tie, and its label is the first of the two, t — right only by the first maximum (at B = 2, where row 1 is that row, the
    second, C - 1: wrong only by the first maximum)."""
    rs = np.random.RandomState(900 + 7 * B + 3 * D + C + (0 if kind == 'unit' else 1))
    y = rs.standard_normal((B, D)).astype(np.float32)
    W = (rs.standard_normal((D, C)) * ((1.0 if kind == 'unit' else 30.0) / np.sqrt(D))).astype(np.float32)
    b = (0.1 * rs.standard_normal(C)).astype(np.float32)
    labels = rs.randint(0, C, B).astype(np.int32)
    labels[0] = 0
    if B >= 2:
        labels[1] = C - 1
    if B >= 2 and C >= 2:
        t = (C - 1) // 2
        y[B - 1] = 0.0
        b[t] = b[C - 1] = np.float32(2.0)
        labels[B - 1] = t if B >= 3 else C - 1
    if kind == 'wide' and B >= 4:
        labels[2] = int(np.argmin(f64(y[2]) @ f64(W) + f64(b)))
    return y, W, b, labels


def head_dz_floor(B, y):
    """The scale below which a column of dW or db is not held to a relative bound: float32 has no normal number under 2^-126, so
    an entry of dz may be off by that much absolutely, a sum over B rows of y dz by B max|y| 2^-126; at the 1e-5 bound that is the
    error of a column of scale B max|y| 2^-126 / 1e-5."""
    return B * max(float(np.abs(y).max()), 1.0) * 2.0 ** -126 / 1e-5



# ---- t2i_pooled_grad_scatter -----------------------------------------------------------------------------------------------------
def scatter(g, mask, keep, HW, c0s, widths):
    """g, mask [B, D] -> [g[:, c0:c0 + w] * mask[:, c0:c0 + w] / keep / HW broadcast over the HW pixels, as [B, HW, w], per branch],
    in the dtype of g with keep and HW rounded to it: float32 in gives the kernel's three roundings in the header's order"""
    t = g.dtype.type
    full = g * mask / t(keep) / t(HW)
    return [np.broadcast_to(full[:, None, c0:c0 + w], (g.shape[0], HW, w)).copy() for c0, w in zip(c0s, widths)]


INCEPTION_WIDTHS = (320, 384, 384, 384, 384, 192)       # the six branch outputs of Mixed_7c
# (B, HW, D, widths, c0s)
SCATTER_CASES = (
    (1, 1, 4, (4,), (0,)),
    (2, 3, 24, (4, 12, 8), (0, 4, 16)),
    (2, 3, 24, (8, 4), (16, 0)),                                              # out of order, not covering D
    (3, 64, 2048, INCEPTION_WIDTHS, tuple(int(c) for c in np.cumsum((0,) + INCEPTION_WIDTHS[:-1]))),
    # the most branches, a width of 4 beside one of 512 in a shared grid sized for the widest: 6 work items against 768
    (2, 3, 564, (512, 4) + (8,) * (MAX_SCATTER_BRANCHES - 2), (0, 512) + tuple(516 + 8 * i for i in range(MAX_SCATTER_BRANCHES - 2))),
)
SCATTER_KEEPS = (0.8, 1.0)


# ---- t2i_rmsprop_tf --------------------------------------------------------------------------------------------------------------
def rmsprop(w, g, ms, mom, lr, rho, momentum, eps):
    """TF's ApplyRMSProp -> (w, ms, mom) after one step"""
    ms = ms + (g * g - ms) * (1.0 - rho)
    mom = momentum * mom + lr * g / np.sqrt(ms + eps)
    w = w - mom
    return w, ms, mom


RMSPROP_GRID_CAP = 2048 * 256             # elements one pass of the capped grid covers: beyond it the grid-stride loop wraps
RMSPROP_SIZES = (1, 255, 257, 1003, RMSPROP_GRID_CAP + 257)
RMSPROP_PARAMS = ((0.9, 0.0, 1e-10), (0.9, 0.9, 1e-10), (0.5, 0.9, 1.0))      # (rho, momentum, eps)
RMSPROP_LR = 5e-5
RMSPROP_STEPS = 3
# (n, (rho, momentum, eps), ms starts at zero)
RMSPROP_CASES = tuple((n, p, False) for n in RMSPROP_SIZES for p in RMSPROP_PARAMS) + ((1003, RMSPROP_PARAMS[1], True),)


def rmsprop_inputs(n, seed=0):
    """float32 w [n] and RMSPROP_STEPS gradients [n]: magnitudes 10^U(-4, 1), one element in eight exactly zero, and a sign that is
    drawn per element and kept over the steps — momentum * mom + lr g / sqrt(ms + eps) then adds terms of one sign.  w is N(0, 1)
    moved 0.25 away from zero, far above any |mom| (at most lr * sqrt(1 / (1 - rho)) / (1 - momentum), about 1.6e-3), so w - mom
    does not cancel either.  A per-element relative bound is then one float32 can meet: a cancelling sum has no relative accuracy
    in any arithmetic."""
    rs = np.random.RandomState(7000 + n % 9973 + seed)
    w = rs.standard_normal(n)
    w = (w + np.where(w < 0, -0.25, 0.25)).astype(np.float32)
    sign = rs.choice([-1.0, 1.0], n)
    gs = []
    for _ in range(RMSPROP_STEPS):
        g = sign * 10.0 ** rs.uniform(-4.0, 1.0, n)
        g[rs.randint(0, 8, n) == 0] = 0.0
        gs.append(g.astype(np.float32))
    return w, gs


RMSPROP_MIXED_CASES = ((1003, RMSPROP_PARAMS[1]), (1003, RMSPROP_PARAMS[2]))      # (n, (rho, momentum, eps))


def rmsprop_mixed_inputs(n, seed=0):
    """What rmsprop_inputs keeps away from: a fresh sign per element and step, so that momentum * mom + lr g / sqrt(ms + eps)
    changes sign and cancels, and w ~ N(0, 1e-8), of the size of mom, so that w - mom crosses zero.  A result of such a sum is
    held relative to the sum of its absolute terms (rmsprop_abs_terms), not to itself."""
    rs = np.random.RandomState(7500 + n % 9973 + seed)
    w = (1e-4 * rs.standard_normal(n)).astype(np.float32)
    gs = []
    for _ in range(RMSPROP_STEPS):
        g = rs.choice([-1.0, 1.0], n) * 10.0 ** rs.uniform(-4.0, 1.0, n)
        g[rs.randint(0, 8, n) == 0] = 0.0
        gs.append(g.astype(np.float32))
    return w, gs


def rmsprop_abs_terms(w_abs, mom_abs, g, ms, lr, momentum, eps):
    """The sums of the absolute values of every term that has entered w and mom, one step on: unrolled, mom is a sum of
    momentum^k lr g / sqrt(ms + eps) over the steps so far and w is w0 minus every mom.  ms is the step's new ms; start from
    (|w0|, 0).  -> (w_abs + mom_abs', momentum mom_abs + |lr g / sqrt(ms + eps)|)"""
    mom_abs = momentum * mom_abs + np.abs(lr * g / np.sqrt(ms + eps))
    return w_abs + mom_abs, mom_abs
