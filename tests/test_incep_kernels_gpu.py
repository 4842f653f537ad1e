"""The kernels of csrc/t2i_eval.hip and csrc/t2i_incep_train.hip behind the IS / FID / IMD figures against their restatements
(tests/incep_kernel_cases.py), at the smallest shapes that reach every dispatch branch of each.

Bounds.  A figure printed as n/0e+00 is a count of elements that differ bit for bit from the reference: it must be 0.
  pool2d MAX      bit-equal on both input kinds
  pool2d AVG      integer inputs: bit-equal to the float32 IEEE quotient fl32(sum) / fl32(count) (the sum is exact);
                  negative Gaussian: 4 eps_f32 of max|ref| (tests/test_eval_gpu.py's bound)
  slice forms     every channel outside [c0, c0 + C) keeps its sentinel bit for bit
  gram            integer inputs: G and sum equal the float64 restatement, the added G0 / sum0 included
  pool_dropout    mask bit-equal to the Philox statement for every (shape, seed, step); pre bit-equal to the float32 quotient on
                  integers, within 1e-6 of max otherwise; y bit-equal to pre / fl32(keep) * mask in float32
  softmax head    logits, prob, dy per row, dW and db per class column: 1e-5 of their own scale (the project's forward bound); loss
                  1e-5 relative; accuracy exact; a repeated call bit-equal.  A column's scale is its own max|ref| (for db, |db[c]|),
                  never less than what float32's smallest normal number allows (head_dz_floor).  The (shape, check) pairs that
                  miss 1e-5 are listed in HEAD_STATED with the bound they get and their measured value; every other one is held
                  to 1e-5.  accumulate: base + reference within the same bound plus the one float32 rounding of the sum,
                  eps_f32 / 2 of max|base + ref|
  scatter         bit-equal to g * mask / fl32(keep) / fl32(HW) in float32 in that order; the guard row after each output untouched
  rmsprop         per element |got - ref| <= 1e-6 |ref| + 1e-12 after every step (tests/test_incep_train_gpu.py's bound); the
                  printed figure is the largest |got - ref| / (1e-6 |ref| + 1e-12), bound 1.  Those inputs keep mom and w from
                  cancelling; two cases where mom changes sign and w crosses zero hold mom and w to 1e-6 of the sum of their
                  absolute terms + 1e-12 instead
  slice copy      exact
pytest -s prints every measured figure beside its bound."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import incep_kernel_cases as IC  # noqa: E402
from incep_kernel_cases import Report, f64  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'
FWD = 1e-5                                # the project's forward bound (tests/test_kernels_gpu.py)
AVG = 4 * IC.EPS32
PRE = 1e-6


def _sid(s):
    return 'x'.join(str(v) for v in s) if isinstance(s, tuple) else str(s)


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEVICE).contiguous()


def dev_off(a):
    """the same values as a contiguous view that starts one float into a larger buffer: 4-byte aligned, not 16"""
    a = np.asarray(a, np.float32)
    buf = torch.zeros(a.size + 7, dtype=torch.float32, device=DEVICE)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- t2i_pool2d ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', IC.POOL_CLASSES, ids=[c[0] for c in IC.POOL_CLASSES])
@pytest.mark.parametrize('g', IC.POOL_GEOMETRIES, ids=_sid)
def test_pool2d_every_geometry_and_form(K, g, cls):
    B, H, W, KH, KW, SH, SW, padding = g
    name, C, sl, xoff, _ = cls
    r = Report('pool2d %s %s' % (_sid(g), name))
    for kind in IC.POOL_KINDS:
        x = IC.pool_input((B, H, W, C), kind, IC.pool_seed(g, C))
        xd = dev_off(x) if xoff else dev(x)
        total, count = IC.pool_sum_count(x, KH, KW, SH, SW, padding)
        refs = {K.POOL_MAX: IC.pool(x, KH, KW, SH, SW, padding, IC.POOL_MAX), K.POOL_AVG: total / count[None, :, :, None]}
        for op, tag in ((K.POOL_MAX, 'max'), (K.POOL_AVG, 'avg')):
            if sl is None:
                got = K.pool2d(xd, KH, KW, SH, SW, padding, op)
            else:
                ld, c0 = sl
                buf = torch.full(tuple(refs[op].shape[:3]) + (ld,), IC.SENTINEL, device=DEVICE)
                K.pool2d(xd, KH, KW, SH, SW, padding, op, out=buf, c0=c0)
                got = buf[..., c0:c0 + C]
                outside = torch.cat([buf[..., :c0], buf[..., c0 + C:]], -1)
                r.check('%s %s outside' % (kind, tag), float((bits(outside) != bits(torch.full_like(outside, IC.SENTINEL))).sum()), 0.0)
            assert tuple(got.shape) == refs[op].shape
            if op == K.POOL_MAX:
                r.exact('%s max' % kind, got, refs[op])
            elif kind == 'integer':
                r.exact('integer avg', got, IC.avg_quotient_f32(total, count).astype(np.float64))
            else:
                r.check('negative avg', IC.relerr(got, refs[op]), AVG)
    r.done()


# ---- t2i_channel_slice_copy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', IC.SLICE_COPY_CASES, ids=_sid)
def test_channel_slice_copy_every_form(K, case):
    rows, C, ld, c0, xoff, _ = case
    rs = np.random.RandomState(rows + C + ld + c0)
    x = rs.standard_normal((rows, C)).astype(np.float32)
    y = rs.standard_normal((rows, ld)).astype(np.float32)
    out = dev(y)
    K.channel_slice_copy(dev_off(x) if xoff else dev(x), out, c0)
    r = Report('slice_copy %s' % _sid(case))
    want = torch.from_numpy(IC.slice_copy(x, y, c0))
    r.check('bits', float((bits(out) != bits(want)).sum()), 0.0)
    r.done()


# ---- t2i_gram_accumulate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', IC.GRAM_DIMS)
def test_gram_accumulate_integers_equal_float64(K, d):
    r = Report('gram d=%d' % d)
    for seq in IC.GRAM_SEQUENCES:
        Xs, s, G0, sum0 = IC.gram_inputs(d, seq)
        G, sm = dev(G0, torch.float64), dev(sum0, torch.float64)
        sd = dev(s)
        ref_G, ref_s = G0, sum0
        for X in Xs:
            K.gram_accumulate(dev(X), sd, sm, G)
            ref_G, ref_s = IC.gram(X, s, ref_G, ref_s)
        tag = '+'.join(str(n) for n in seq)
        r.exact('n=%s G' % tag, G, ref_G)
        r.exact('n=%s sum' % tag, sm, ref_s)
    r.done()


# ---- t2i_pool_dropout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', IC.DROPOUT_SHAPES, ids=_sid)
def test_pool_dropout_mask_is_the_philox_statement(K, shape):
    B, HW, D, keep = shape
    r = Report('pool_dropout %s' % _sid(shape))
    rs = np.random.RandomState(B * HW + D)
    xs = {'integer': rs.randint(-4, 5, (B, HW, D)).astype(np.float32), 'gaussian': (rs.standard_normal((B, HW, D)) + 0.5).astype(np.float32)}
    for i, (seed, step) in enumerate(IC.DROPOUT_STREAMS):
        kind = ('integer', 'gaussian')[i % 2]
        x = xs[kind]
        pre, mask, y = K.pool_dropout(dev(x).view(B, HW, 1, D), keep, seed=seed, step=step)
        want = IC.dropout_mask(seed, step, B, D, keep)
        tag = 's%d' % i
        r.check('%s mask' % tag, float((bits(mask) != bits(torch.from_numpy(want))).sum()), 0.0)
        total, mean = IC.pool_mean(x)
        if kind == 'integer':
            assert np.abs(x).sum(1).max() < 2 ** 24
            r.exact('%s pre' % tag, pre, (total.astype(np.float32) / np.float32(HW)).astype(np.float64))
        else:
            r.check('%s pre' % tag, IC.relerr(pre, mean), PRE)
        p32, m32 = pre.cpu().numpy(), mask.cpu().numpy()
        r.check('%s y' % tag, float((bits(y) != bits(torch.from_numpy(p32 / np.float32(keep) * m32))).sum()), 0.0)
        if keep == 1.0:
            r.check('%s ones' % tag, float((m32 != 1.0).sum()), 0.0)
            r.check('%s y=pre' % tag, float((bits(y) != bits(pre)).sum()), 0.0)
    r.done()


# ---- t2i_softmax_ce_head ---------------------------------------------------------------------------------------------------------
# The stated exceptions of this module, in the form of WINO3_STATED (tests/test_kernels_gpu.py): (shape, check) -> (the bound it
# gets, the value measured for it on an MI355X).  Every other check of every shape is held to the plain FWD.
# prob[c] = exp(logit[c] - max) / se, so an absolute error d in a logit difference is a relative error d in the probability, and a
# column of dW or db of a class that is nowhere likely is made of such probabilities alone.  At the 'wide' logits of these shapes
# (max|logits| 80 .. 135) float32's spacing alone is 7.6e-6, each of the two logits of a difference carries half of it, and a
# D-long float32 dot product adds its own: a few times 1e-5 of such a column's scale is what the format gives.
HEAD_STATED = {
    ((16, 2048, 1000), 'wide dW/col'): (5e-5, 2.66e-5),
    ((16, 8, 1024), 'wide dW/col'): (4e-5, 1.61e-5),
    ((2, 16380, 4), 'wide dW/col'): (3e-5, 1.36e-5),
    ((16, 8, 1024), 'wide db/col'): (3e-5, 1.31e-5),
    ((64, 2048, 50), 'wide db/col'): (3e-5, 1.26e-5),       # here the column sum of dz cancels as well
}


def _bound(shape, check):
    return HEAD_STATED.get((tuple(shape), check), (FWD, None))[0]


def _head_checks(r, shape, tag, out, ref, y):
    B = shape[0]
    floor = IC.head_dz_floor(B, y)
    r.check('%s logits' % tag, IC.relerr(out['logits'], ref['logits']), FWD)
    r.check('%s prob' % tag, IC.relerr(out['prob'], ref['prob']), FWD)
    r.check('%s dy/row' % tag, IC.relerr_rows(out['dy'], ref['dy'], floor), _bound(shape, '%s dy/row' % tag))
    r.check('%s dW/col' % tag, IC.relerr_cols(out['dW'], ref['dW'], floor), _bound(shape, '%s dW/col' % tag))
    r.check('%s db/col' % tag, IC.relerr_cols(f64(out['db'])[None, :], ref['db'][None, :], floor), _bound(shape, '%s db/col' % tag))
    loss = float(out['loss'])
    r.check('%s loss' % tag, abs(loss - ref['loss']) / abs(ref['loss']) if ref['loss'] else (0.0 if loss == 0.0 else np.inf), FWD)
    r.check('%s acc' % tag, abs(float(out['acc']) - float(np.float32(ref['correct']) / np.float32(B))), 0.0)     # the float32 quotient


@pytest.mark.parametrize('shape', IC.HEAD_SHAPES, ids=_sid)
def test_softmax_ce_head_every_shape(K, shape):
    B, D, C = shape
    r = Report('head %s' % _sid(shape))
    for kind in IC.HEAD_KINDS:
        y, W, b, labels = IC.head_inputs(B, D, C, kind)
        ref = IC.head(y, W, b, labels)
        args = (dev(y), dev(W), dev(b), dev(labels, torch.int32))
        out = K.softmax_ce_head(*args)
        _head_checks(r, shape, kind, out, ref, y)
        again = K.softmax_ce_head(*args)
        r.check('%s repeat' % kind, float(sum(int((bits(out[k]) != bits(again[k])).sum()) for k in out)), 0.0)      # no atomics
    r.done()


@pytest.mark.parametrize('shape', IC.HEAD_ACCUMULATE_SHAPES, ids=_sid)
def test_softmax_ce_head_accumulates_into_interior_views(K, shape):
    B, D, C = shape
    r = Report('head accumulate %s' % _sid(shape))
    y, W, b, labels = IC.head_inputs(B, D, C, 'unit')
    ref = IC.head(y, W, b, labels)
    rs = np.random.RandomState(B + D + C)
    pad = 13                                  # the views start 13 floats into their buffers and end 13 before the end
    bufW_h = rs.randint(-2, 3, pad + D * C + pad).astype(np.float32)
    bufb_h = rs.randint(-2, 3, pad + C + pad).astype(np.float32)
    floor = IC.head_dz_floor(B, y)
    for accumulate in (True, False):
        bufW, bufb = dev(bufW_h), dev(bufb_h)
        out = K.softmax_ce_head(dev(y), dev(W), dev(b), dev(labels, torch.int32), dW_out=bufW[pad:pad + D * C].view(D, C),
                                db_out=bufb[pad:pad + C], accumulate=accumulate)
        assert out['dW'].data_ptr() == bufW.data_ptr() + 4 * pad and out['db'].data_ptr() == bufb.data_ptr() + 4 * pad
        tag = 'add' if accumulate else 'set'
        for name, buf, host, want in (('dW', bufW, bufW_h, ref['dW']), ('db', bufb, bufb_h, ref['db'])):
            n = want.size
            base = host[pad:pad + n].astype(np.float64).reshape(want.shape) if accumulate else np.zeros(want.shape)
            got = f64(buf[pad:pad + n]).reshape(want.shape)
            # got = fl32(base + s): one rounding of the sum on top of the bound on s, column by column
            cols = want.reshape(-1, C)
            err = np.abs(got - base - want).reshape(-1, C).max(0)
            tol = _bound(shape, 'accumulate %s/col' % name) * np.maximum(np.abs(cols).max(0), floor) + 0.5 * IC.EPS32 * np.abs(base + want).reshape(-1, C).max(0)
            r.check('%s %s/col' % (tag, name), float((err / tol).max()), 1.0)
            edge = torch.cat([buf[:pad], buf[pad + n:]]).cpu()
            r.check('%s %s edges' % (tag, name), float((bits(edge) != bits(torch.from_numpy(np.concatenate([host[:pad], host[pad + n:]])))).sum()), 0.0)
        r.check('%s dy/row' % tag, IC.relerr_rows(out['dy'], ref['dy'], floor), FWD)
    r.done()


# ---- t2i_pooled_grad_scatter -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('keep', IC.SCATTER_KEEPS)
@pytest.mark.parametrize('case', IC.SCATTER_CASES, ids=lambda c: '%dx%dx%d-%db' % (c[0], c[1], c[2], len(c[3])))
def test_pooled_grad_scatter_every_table(K, case, keep):
    B, HW, D, widths, c0s = case
    r = Report('scatter %dx%dx%d widths %s at %s keep %g' % (B, HW, D, list(widths), list(c0s), keep))
    rs = np.random.RandomState(B * HW + D)
    g = rs.standard_normal((B, D)).astype(np.float32)
    m = np.ones((B, D), np.float32) if keep == 1.0 else (rs.random_sample((B, D)) < keep).astype(np.float32)
    guard = -5.0
    bufs = [torch.full(((B * HW + 1) * w,), guard, device=DEVICE) for w in widths]      # one guard row after each output
    outs = [buf[:B * HW * w].view(B, HW, w) for buf, w in zip(bufs, widths)]
    K.pooled_grad_scatter(dev(g), dev(m), keep, outs, list(c0s), HW)
    for i, (buf, o, want, w) in enumerate(zip(bufs, outs, IC.scatter(g, m, keep, HW, c0s, widths), widths)):
        assert want.dtype == np.float32
        r.check('b%d' % i, float((bits(o) != bits(torch.from_numpy(want))).sum()), 0.0)
        r.check('b%d guard' % i, float((buf[B * HW * w:].cpu() != guard).sum()), 0.0)
    r.done()


# ---- t2i_rmsprop_tf --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', IC.RMSPROP_CASES, ids=lambda c: 'n%d-rho%g-mu%g-eps%g%s' % (c[0], c[1][0], c[1][1], c[1][2], '-ms0' if c[2] else ''))
def test_rmsprop_tf_every_size_and_setting(K, case):
    n, (rho, mu, eps), zero_ms = case
    r = Report('rmsprop n=%d rho=%g momentum=%g eps=%g ms0=%d' % (n, rho, mu, eps, 0 if zero_ms else 1))
    w0, gs = IC.rmsprop_inputs(n)
    w, ms, mom = dev(w0), dev(np.zeros(n) if zero_ms else np.ones(n)), dev(np.zeros(n))
    # the scalars reach the kernel as float32: the reference takes the same values, widened
    lr64, rho64, mu64, eps64 = (float(np.float32(v)) for v in (IC.RMSPROP_LR, rho, mu, eps))
    rw, rms, rmom = w0.astype(np.float64), f64(ms), f64(mom)
    for step, g in enumerate(gs):
        K.rmsprop_tf(w, dev(g), ms, mom, IC.RMSPROP_LR, rho=rho, momentum=mu, eps=eps)
        rw, rms, rmom = IC.rmsprop(rw, g.astype(np.float64), rms, rmom, lr64, rho64, mu64, eps64)
        for name, got, ref in (('w', w, rw), ('ms', ms, rms), ('mom', mom, rmom)):
            r.check('step%d %s' % (step, name), float((np.abs(f64(got) - ref) / (1e-6 * np.abs(ref) + 1e-12)).max()), 1.0)
    r.done()


@pytest.mark.parametrize('case', IC.RMSPROP_MIXED_CASES, ids=lambda c: 'n%d-rho%g-mu%g-eps%g' % (c[0], c[1][0], c[1][1], c[1][2]))
def test_rmsprop_tf_where_the_sums_cancel(K, case):
    """Gradients of a fresh sign per step and w of the size of mom: mom changes sign and w crosses zero.  ms is a sum of one sign and
    keeps the per-element bound; mom and w are held to 1e-6 of the sum of the absolute values of every term that has entered them
    so far (incep_kernel_cases.rmsprop_abs_terms) + 1e-12: the same bound, with the scale a cancelling sum has — an error made
    before a cancellation stays as large as it was.  The printed figure is the largest |got - ref| / bound, bound 1."""
    n, (rho, mu, eps) = case
    r = Report('rmsprop mixed signs n=%d rho=%g momentum=%g eps=%g' % (n, rho, mu, eps))
    w0, gs = IC.rmsprop_mixed_inputs(n)
    w, ms, mom = dev(w0), dev(np.ones(n)), dev(np.zeros(n))
    lr64, rho64, mu64, eps64 = (float(np.float32(v)) for v in (IC.RMSPROP_LR, rho, mu, eps))
    rw, rms, rmom = w0.astype(np.float64), np.ones(n), np.zeros(n)
    w_terms, mom_terms = np.abs(rw), np.zeros(n)
    flips, crossings = 0, 0
    for step, g in enumerate(gs):
        K.rmsprop_tf(w, dev(g), ms, mom, IC.RMSPROP_LR, rho=rho, momentum=mu, eps=eps)
        g64 = g.astype(np.float64)
        nw, rms, nmom = IC.rmsprop(rw, g64, rms, rmom, lr64, rho64, mu64, eps64)
        w_terms, mom_terms = IC.rmsprop_abs_terms(w_terms, mom_terms, g64, rms, lr64, mu64, eps64)
        flips += int((nmom * rmom < 0).sum())
        crossings += int((nw * rw < 0).sum())
        rw, rmom = nw, nmom
        for name, got, ref, scale in (('w', w, rw, w_terms), ('ms', ms, rms, np.abs(rms)), ('mom', mom, rmom, mom_terms)):
            r.check('step%d %s' % (step, name), float((np.abs(f64(got) - ref) / (1e-6 * scale + 1e-12)).max()), 1.0)
    assert flips >= n // 10 and crossings >= n // 10, (flips, crossings)          # the case is what it says
    r.done()
