"""The oldest small kernels of csrc/t2i_aux.hip against their float64 restatements (tests/row_head_cases.py): per-sample moments and
fma (layer norm), the 2x2 pool / x2 upscale, the fade-in with its weight in device memory, the conditioning augmentation, the WGAN
critic head and the gradient-penalty row kernels — at the smallest shapes that reach every path of each (one / several / the capped
number of chunks, vector and scalar bodies, misaligned bases, wrapped grid-stride loops, the second block of a second stage).

Bounds.  On small integers with power-of-two scalars every result is representable in float32 and is held
to the float64 restatement with torch.equal (`exact`): an indexing error has no tolerance to hide in.  Otherwise:
  LIN   1e-6 of max|ref|          the index-only kernels on Gaussian data (one or two roundings per element)
  SUM   1e-5 of sum|terms|        row_moments, slopes^2, kl, the head's means: at most 64 float4 steps per thread, 6 shuffle steps,
                                  4 waves and 64 chunks of float32 accumulation, worst case about 5e-6; normalised by the sum of the
                                  absolute terms because s1 of zero-mean data is a cancelling sum
  DIFF  1e-6 of the sum of the absolute values combined: the head's differences of means
  SEED  1e-7 absolute on the logit seeds, LIN on the slope seeds
  FWD   1e-5 of max|ref|          elementwise results through expf (the project's forward bound, tests/test_kernels_gpu.py)
The measured values beside the bounds are the largest over the cases of a test on an MI355X (pytest -s prints all of them)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import row_head_cases as RC  # noqa: E402
from row_head_cases import relerr  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'
LIN, SUM, DIFF, SEED, FWD = 1e-6, 1e-5, 1e-6, 1e-7, 1e-5
IDS = dict(ids=lambda s: 'x'.join(str(v) for v in s) if isinstance(s, tuple) else str(s))


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def A(K):
    from t2i_amd import autograd
    return autograd


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEVICE).contiguous()


def dev_off(a):
    """the same values as a contiguous view that starts one float into a larger buffer: 4-byte aligned, not 16"""
    a = np.asarray(a, np.float32)
    buf = torch.zeros(a.size + 7, dtype=torch.float32, device=DEVICE)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def put(a, off):
    return dev_off(a) if off else dev(a)


def exact(got, ref64):
    """bit equality with the float64 restatement, which float32 must hold exactly"""
    ref = torch.tensor(np.asarray(ref64), dtype=torch.float64)
    assert torch.equal(ref.float().double(), ref), 'the case is not exactly representable'
    return torch.equal(got.detach().cpu(), ref.float())


# ---- 1. row_moments ----------------------------------------------------------------------------------------------------------
ROW_MOMENT_CASES = [
    (1, 1, ''),                  # the smallest input
    (3, 483, ''),                # scalar body, one chunk
    (65, 96, ''),                # the second block of stage 2
    (2, 8192, ''),               # the last size with one chunk
    (2, 8196, ''),               # the first with two
    (3, 24580, ''),              # 4 chunks, the last one short after per_chunk is rounded to a multiple of 4
    (3, 24581, ''),              # the same on the scalar body
    (2, 524288, ''),             # 64 chunks exactly
    (2, 524296, ''),             # the cap: 64 chunks of more than 8192
    (3, 24580, 'a'),             # per % 4 == 0 from a misaligned base: scalar body
    (3, 24580, 'b'),             # aligned a, misaligned b: the same through b
]


@pytest.mark.parametrize('B,per,off', ROW_MOMENT_CASES)
def test_row_moments(K, B, per, off):
    a = RC.gaussian((B, per), 11 + per)
    b = RC.gaussian((B, per), 12 + per, offset=-0.3, scale=0.9)
    rep = RC.Report('row_moments B %d per %d %s' % (B, per, off or 'aligned'))
    for name, bb in (('aa', None), ('ab', b)):
        if off == 'b' and bb is None:
            continue
        s1, s2 = K.row_moments(put(a, off == 'a'), put(bb, off == 'b') if bb is not None else None)
        torch.cuda.synchronize()
        r1, r2, n1, n2 = RC.row_moments(RC.f64(a), RC.f64(bb) if bb is not None else None)
        rep.check('s1(%s)' % name, float((np.abs(RC.f64(s1) - r1) / n1).max()), SUM)       # measured <= 4.3e-8
        rep.check('s2(%s)' % name, float((np.abs(RC.f64(s2) - r2) / n2).max()), SUM)       # measured <= 1.8e-7
    rep.done()


# ---- 2. row_fma2 -------------------------------------------------------------------------------------------------------------
ROW_FMA_CASES = [
    (3, 483, False),             # scalar body
    (65, 96, False),             # float4 body, many rows
    (3, 24580, False),
    (3, 24580, True),            # misaligned: scalar body at per % 4 == 0
    (5, 524296, False),          # n / 4 > 2048 * 256: the float4 grid wraps
    (9, 65537, False),           # n > 2048 * 256 with an odd per: the scalar grid wraps
]


@pytest.mark.parametrize('B,per,off', ROW_FMA_CASES)
def test_row_fma2(K, B, per, off):
    ai, bi = RC.integers((B, per), 21 + per), RC.integers((B, per), 22 + per)
    ag, bg = RC.gaussian((B, per), 23 + per), RC.gaussian((B, per), 24 + per, offset=-0.2)
    p_al, p_ga, p_de = RC.pow2_rows(B, 1), RC.pow2_rows(B, 5), RC.pow2_rows(B, 25)
    rs = np.random.RandomState(B + per)
    r_al, r_ga, r_de = (rs.uniform(-2.0, 2.0, B).astype(np.float32) for _ in range(3))
    assert len(set(r_al)) == B and len(set(r_ga)) == B and len(set(r_de)) == B
    dai, dbi, dag, dbg = put(ai, off), put(bi, off), put(ag, off), put(bg, off)
    rep = RC.Report('row_fma2 B %d per %d %s' % (B, per, 'misaligned' if off else 'aligned'))
    for with_b in (False, True):
        for with_d in (False, True):
            tag = '%s%s' % ('b' if with_b else '-', 'd' if with_d else '-')
            got = K.row_fma2(dai, dev(p_al), dbi if with_b else None, dev(p_ga) if with_b else None, dev(p_de) if with_d else None)
            ref = RC.row_fma2(RC.f64(ai), RC.f64(p_al), RC.f64(bi) if with_b else None, RC.f64(p_ga) if with_b else None,
                              RC.f64(p_de) if with_d else None)
            assert exact(got, ref), ('integers', tag, B, per)
            got = K.row_fma2(dag, dev(r_al), dbg if with_b else None, dev(r_ga) if with_b else None, dev(r_de) if with_d else None)
            ref = RC.row_fma2(RC.f64(ag), RC.f64(r_al), RC.f64(bg) if with_b else None, RC.f64(r_ga) if with_b else None,
                              RC.f64(r_de) if with_d else None)
            rep.check(tag, relerr(got, ref), LIN)                                           # measured <= 9.3e-8
    rep.done()


# ---- 3. layer norm through its Function --------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 5, 1229, 4), (2, 2, 65537, 4)], **IDS)       # per = 24580 (4 chunks); 524296 (the cap; C % 4 == 0)
def test_layer_norm_forward_and_backward_at_many_chunks(K, A, shape):
    """tests/test_pggan.py's layer-norm check (bounds 1e-5 / 1e-4 / 1e-5) where a sample spans several chunks, with per-sample means
    of 4 standard deviations: the one-pass variance s2 / n - mean^2 restated in float32 NumPy stays at 1.5e-6 ... 2.9e-6 there."""
    B, C = shape[0], shape[-1]
    g = torch.Generator().manual_seed(31 + shape[2])
    centre = 6.8 * torch.tensor([1.0, -1.0, 1.0][:B]).reshape((B,) + (1,) * (len(shape) - 1))
    xs = torch.randn(shape, generator=g) * 1.7 + centre
    gam, bet = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(shape, generator=g)
    xg, gg, bg = xs.cuda().requires_grad_(True), gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
    y = A.LayerNormFn.apply(xg, gg, bg, 1e-12, K.ACT_NONE, 0.0)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    yr, dxr, dgr, dbr = RC.layer_norm(xs.double(), gam.double(), bet.double(), dy.double())
    rep = RC.Report('layer_norm %s' % (shape,))
    rep.check('y', relerr(y, yr.numpy()), 1e-5)                   # measured <= 1.5e-6
    rep.check('dx', relerr(xg.grad, dxr.numpy()), 1e-4)           # measured <= 1.5e-6
    rep.check('dgamma', relerr(gg.grad, dgr.numpy()), 1e-5)       # measured <= 1.4e-6
    rep.check('dbeta', relerr(bg.grad, dbr.numpy()), 1e-5)        # measured <= 1.5e-7
    rep.done()


# ---- 4. pool2_sum / upscale2 -------------------------------------------------------------------------------------------------
RESAMPLE_CASES = [
    ((2, 6, 10, 8), False),      # float4 body
    ((1, 2, 2, 4), False),       # one output pixel of one float4
    ((2, 6, 10, 3), False),      # scalar body
    ((2, 6, 10, 8), True),       # C % 4 == 0 from a misaligned base: scalar body, the same values
    ((1, 4, 10, 12), False),     # B = 1, not square
]


@pytest.mark.parametrize('shape,off', RESAMPLE_CASES, **IDS)
def test_pool2_sum_and_upscale2(K, shape, off):
    xi, xg = RC.integers(shape, 41 + shape[3]), RC.gaussian(shape, 42 + shape[3])
    di, dg = put(xi, off), put(xg, off)
    rep = RC.Report('resample2 %s %s' % (shape, 'misaligned' if off else 'aligned'))
    assert exact(K.pool2_sum(di, 0.25), RC.pool2_sum(RC.f64(xi), 0.25))
    assert exact(K.upscale2(di, 1.0), RC.upscale2(RC.f64(xi), 1.0)) and exact(K.upscale2(di, 2.0), RC.upscale2(RC.f64(xi), 2.0))
    s = float(np.float32(0.3))
    pg, ug = K.pool2_sum(dg, s), K.upscale2(dg, s)
    rep.check('pool', relerr(pg, RC.pool2_sum(RC.f64(xg), s)), LIN)            # measured <= 9.0e-8
    rep.check('upscale', relerr(ug, RC.upscale2(RC.f64(xg), s)), LIN)          # measured <= 3.7e-8
    if off:                                                                   # the scalar body and the float4 body agree bit for bit
        assert torch.equal(pg, K.pool2_sum(dev(xg), s)) and torch.equal(ug, K.upscale2(dev(xg), s))
    # <pool(x), y> == 0.25 <x, up(y)> on integers: every product and sum is exact in float64
    B, H, W, C = shape
    yi = RC.integers((B, H // 2, W // 2, C), 43 + C)
    terms = RC.f64(K.pool2_sum(di, 0.25)) * RC.f64(yi)
    lhs = float(terms.sum())
    rhs = 0.25 * float((RC.f64(xi) * RC.f64(K.upscale2(put(yi, off), 1.0))).sum())
    assert lhs == rhs and float(np.abs(terms).sum()) > 0.0, (lhs, rhs)
    rep.done()


def test_pool2_sum_wrapped_grid(K):
    """(3, 256, 256, 64): 3 * 128 * 128 * 16 float4 outputs > 2048 * 256 threads, the grid-stride loop of the float4 pool wraps"""
    xi = RC.integers((3, 256, 256, 64), 44)
    assert 3 * 128 * 128 * 16 > 2048 * 256
    assert exact(K.pool2_sum(dev(xi), 0.25), RC.pool2_sum(RC.f64(xi), 0.25))


def test_upscale2_wrapped_grid(K):
    """to (1, 512, 512, 3): more scalar outputs than 2048 * 256 threads"""
    xi = RC.integers((1, 256, 256, 3), 45)
    assert 512 * 512 * 3 > 2048 * 256
    assert exact(K.upscale2(dev(xi), 2.0), RC.upscale2(RC.f64(xi), 2.0))


# ---- 5. lerp_dev -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 1031, 600001])            # 600001 > 2048 * 256: the grid wraps
def test_lerp_dev(K, n):
    ai, bi = RC.integers(n, 51 + n), RC.integers(n, 52 + n)
    ag, bg = RC.gaussian(n, 53 + n), RC.gaussian(n, 54 + n, offset=-0.2)
    dai, dbi, dag, dbg = dev(ai), dev(bi), dev(ag), dev(bg)
    rep = RC.Report('lerp_dev n %d' % n)
    for t in (0.0, 1.0, 0.5, 0.3):
        td = dev([t])
        t64 = float(np.float32(t))
        for mode in (0, 1, 2):
            if t != 0.3:
                assert exact(K.lerp_dev(dai, dbi if mode == 0 else None, td, mode), RC.lerp(RC.f64(ai), RC.f64(bi), t64, mode)), (t, mode)
            got = K.lerp_dev(dag, dbg if mode == 0 else None, td, mode)
            rep.check('t%g/m%d' % (t, mode), relerr(got, RC.lerp(RC.f64(ag), RC.f64(bg), t64, mode)), LIN)      # measured <= 7.2e-8
    rep.done()


def test_lerp_dev_follows_the_device_scalar(K):
    """t is read from device memory at run time: overwritten on the device between two launches, the second follows the new value"""
    ai, bi = RC.integers(1031, 55), RC.integers(1031, 56)
    da, db = dev(ai), dev(bi)
    t, nxt = dev([0.5]), dev([0.25])
    first = K.lerp_dev(da, db, t, 0)
    t.copy_(nxt)
    second = K.lerp_dev(da, db, t, 0)
    assert exact(first, RC.lerp(RC.f64(ai), RC.f64(bi), 0.5, 0)) and exact(second, RC.lerp(RC.f64(ai), RC.f64(bi), 0.25, 0))
    assert not torch.equal(first, second)


def test_lerp_dev_function_first_and_second_order(K, A):
    """LerpDevFn against float64 autograd of (1 - t) a + t b: d/da, d/db for a cotangent w, and d <grad_a, v> / dw"""
    n, t = 1031, float(np.float32(0.3))
    a, b, w, v = (RC.gaussian(n, 57 + i) for i in range(4))
    td = dev([t])
    ac, bc, wc = (dev(x).requires_grad_(True) for x in (a, b, w))
    out = A.LerpDevFn.apply(ac, bc, td, 0)
    ga, gb = torch.autograd.grad(out, [ac, bc], wc, create_graph=True)
    gw, = torch.autograd.grad((ga * dev(v)).sum(), wc)
    ar, br, wr = (torch.tensor(RC.f64(x), requires_grad=True) for x in (a, b, w))
    outr = (1.0 - t) * ar + t * br
    gar, gbr = torch.autograd.grad(outr, [ar, br], wr, create_graph=True)
    gwr, = torch.autograd.grad((gar * torch.tensor(RC.f64(v))).sum(), wr)
    rep = RC.Report('LerpDevFn')
    for name, got, ref in (('out', out, outr), ('d/da', ga, gar), ('d/db', gb, gbr), ('d<ga,v>/dw', gw, gwr)):
        rep.check(name, relerr(got, ref.detach().numpy()), LIN)            # measured <= 5.9e-8
    rep.done()


# ---- 6. conditioning augmentation --------------------------------------------------------------------------------------------
CA_SIZES = [1, 1023, 1024, 8192, 8193, 3 * 8192 + 517]       # a partial round; one round exactly; a second round of one element; three and a part


@pytest.mark.parametrize('n', CA_SIZES)
def test_ca_kl_forward_and_backward(K, n):
    mean, ls, eps = RC.ca_inputs(n)
    dm, dl, de = dev(mean), dev(ls), dev(eps)
    code, kl = K.ca_kl_fwd(dm, dl, de)
    rcode, rkl = RC.ca_fwd(RC.f64(mean), RC.f64(ls), RC.f64(eps))
    rep = RC.Report('ca_kl n %d' % n)
    rep.check('code', relerr(code, rcode), FWD)                                # measured <= 1.3e-7
    rep.check('kl', abs(float(kl[0]) - rkl) / rkl, SUM)                        # measured <= 1.1e-7; every term >= 0: sum|terms| = n kl
    dcode = RC.gaussian(n, 61 + n % 89, offset=0.0, scale=1.0)
    dkl = np.float32(0.7)
    for name, dc, dk in (('dcode', dcode, None), ('dkl', None, dkl), ('both', dcode, dkl)):
        gm, gl = K.ca_kl_bwd(dm, dl, de, dev(dc) if dc is not None else None, dev([dk]) if dk is not None else None)
        rm, rl = RC.ca_bwd(RC.f64(mean), RC.f64(ls), RC.f64(eps), RC.f64(dc) if dc is not None else None, float(dk) if dk is not None else None)
        rep.check('dmean(%s)' % name, relerr(gm, rm), FWD)                     # measured <= 6.9e-8
        rep.check('dls(%s)' % name, relerr(gl, rl), FWD)                       # measured <= 1.9e-7
    rep.done()


@pytest.mark.parametrize('shape', [(8, 128), (3 * 8192 + 517,)], **IDS)
def test_ca_sample_kl_function_against_autograd(K, A, shape):
    n = int(np.prod(shape))
    mean, ls, eps = (x.reshape(shape) for x in RC.ca_inputs(n, seed=1))
    w = RC.gaussian(shape, 62, offset=0.0, scale=1.0)
    mc, lc = dev(mean).requires_grad_(True), dev(ls).requires_grad_(True)
    code, kl = A.CaSampleKlFn.apply(mc, lc, dev(eps))
    ((code * dev(w)).sum() + 0.7 * kl.sum()).backward()
    mr, lr = (torch.tensor(RC.f64(x), requires_grad=True) for x in (mean, ls))
    coder = mr + torch.exp(lr) * torch.tensor(RC.f64(eps))
    klr = torch.mean(-lr + 0.5 * (-1.0 + torch.exp(2.0 * lr) + mr ** 2))
    ((coder * torch.tensor(RC.f64(w))).sum() + 0.7 * klr).backward()
    rep = RC.Report('CaSampleKlFn %s' % (shape,))
    rep.check('code', relerr(code, coder.detach().numpy()), FWD)               # measured <= 5.2e-8
    rep.check('kl', abs(float(kl.detach()) - float(klr.detach())) / float(klr.detach()), SUM)      # measured <= 7.6e-8
    rep.check('dmean', relerr(mc.grad, mr.grad.numpy()), FWD)                  # measured <= 3.2e-8
    rep.check('dls', relerr(lc.grad, lr.grad.numpy()), FWD)                    # measured <= 9.5e-8
    rep.done()


# ---- 7. the WGAN critic head -------------------------------------------------------------------------------------------------
KT_CASES = [None, 0.0, 0.37, 1.0]


@pytest.mark.parametrize('gp_coeff', [10.0, 150.0])
@pytest.mark.parametrize('kt', KT_CASES)
@pytest.mark.parametrize('B', [1, 7, 64, 200, 256, 257, 600])
def test_wgan_d_head(K, B, kt, gp_coeff):
    logits, s1, s2 = RC.head_inputs(B, KT_CASES.index(kt))
    ktd = dev([kt]) if kt is not None else None
    ktv = float(np.float32(kt)) if kt is not None else 1.0
    dl, d1, d2 = dev(logits), dev(s1), dev(s2)
    scal, seed_l, seed_s1, seed_s2 = K.wgan_d_head(dl, d1, d2, ktd, gp_coeff)
    torch.cuda.synchronize()
    ref, rl, r1, r2 = RC.d_head(RC.f64(logits), RC.f64(s1), RC.f64(s2), ktv, gp_coeff)
    got = dict(zip(K.D_HEAD_KEYS, (float(v) for v in scal.double().cpu())))
    L = RC.f64(logits)
    mabs = [float(np.abs(L[k * B:(k + 1) * B]).mean()) for k in range(3)]       # mean |logit| of fake | real | mismatch
    wd, wd2, gp = abs(ref['wdist']), abs(ref['wdist2']), ref['real_gp'] + ref['real_gp2']
    # key -> (what the error is a fraction of, bound): means by the mean of their absolute terms, differences (and what is formed
    # from them, to first order) by the sum of the absolute values combined; a normaliser of 0 (no active hinge) asks for exactly 0
    norm = {
        'D_loss_fake': (mabs[0], SUM), 'D_loss_real': (mabs[1], SUM), 'D_loss_mismatch': (mabs[2], SUM),   # measured <= 1.3e-7
        'real_gp': (ref['real_gp'], SUM), 'real_gp2': (ref['real_gp2'], SUM), 'reg_loss': (ref['reg_loss'], SUM),   # measured <= 1.3e-7
        'wdist': (abs(ref['D_loss_real']) + abs(ref['D_loss_fake']), DIFF),                                # measured <= 1.2e-7
        'wdist2': (abs(ref['D_loss_real']) + abs(ref['D_loss_mismatch']), DIFF),                           # measured <= 8.1e-8
        'D_loss': (wd + ktv * wd2 + gp_coeff * gp, DIFF),                                                  # measured <= 1.3e-7
        'balance_loss': ((ktv * wd2 + wd) ** 2, DIFF),                                                     # measured <= 1.7e-7
        'kt_grad': (2.0 * (ktv * wd2 + wd) * wd2, DIFF),                                                   # measured <= 2.2e-7
        'kt': (0.0, 0.0),                                                                                  # kt comes back as given
    }
    rep = RC.Report('wgan_d_head B %d kt %s gp_coeff %g' % (B, kt, gp_coeff))
    for k in K.D_HEAD_KEYS:
        err, (den, tol) = abs(got[k] - ref[k]), norm[k]
        rep.check(k, err / den if den > 0 else err, tol if den > 0 else 0.0)
    rep.check('seed_l', float(np.abs(RC.f64(seed_l) - rl).max()), SEED)                                  # measured <= 1.3e-8 absolute
    rep.check('seed_s1', relerr(seed_s1, r1) if r1.max() > 0 else float(seed_s1.abs().max()), LIN if r1.max() > 0 else 0.0)   # <= 1.1e-7
    rep.check('seed_s2', relerr(seed_s2, r2) if r2.max() > 0 else float(seed_s2.abs().max()), LIN if r2.max() > 0 else 0.0)   # <= 9.2e-8
    # no seed and no penalty where a slope is exactly 1.0 or below it
    assert torch.equal(seed_s1.cpu() == 0, torch.tensor(s1 <= 1.0)) and torch.equal(seed_s2.cpu() == 0, torch.tensor(s2 <= 1.0))
    if B >= 3:
        assert s1[RC.HINGE_AT_ONE['s1']] == 1.0 and s2[RC.HINGE_AT_ONE['s2']] == 1.0 and (s1 > 1).any() and (s1 < 1).any() and (s2 > 1).any() and (s2 < 1).any()
    # the logit seeds land in the caller's buffer and nowhere else
    guard = 8
    buf = torch.full((3 * B + 2 * guard,), -77.0, dtype=torch.float32, device=DEVICE)
    _, into, _, _ = K.wgan_d_head(dl, d1, d2, ktd, gp_coeff, seed_l_into=buf[guard:guard + 3 * B])
    assert into.data_ptr() == buf.data_ptr() + 4 * guard
    assert torch.equal(buf[guard:guard + 3 * B], seed_l) and bool((buf[:guard] == -77.0).all()) and bool((buf[guard + 3 * B:] == -77.0).all())
    # the stacked step's first call, with zero slopes, gives the same logit seeds bit for bit (and no slope seeds)
    zeros = torch.zeros(B, dtype=torch.float32, device=DEVICE)
    zscal, zl, z1, z2 = K.wgan_d_head(dl, zeros, zeros, ktd, gp_coeff)
    assert torch.equal(zl, seed_l) and float(z1.abs().max()) == 0.0 and float(z2.abs().max()) == 0.0
    assert float(zscal[6]) == 0.0 and float(zscal[7]) == 0.0 and float(zscal[1]) == float(scal[1])
    rep.done()


# ---- 8. gradient-penalty rows ------------------------------------------------------------------------------------------------
GP_CASES = [(B, per, False) for per in (105, 12288, 196608) for B in (1, 5)] + [(5, 12288, True)]
#            105 = 5 * 7 * 3: scalar body, rows at unaligned offsets; (5, 12288, True): per % 4 == 0 from a misaligned base


@pytest.mark.parametrize('B,per,off', GP_CASES)
def test_gp_slopes_row_scale_and_interp(K, B, per, off):
    g, x = RC.gaussian((B, per), 71 + per, offset=0.05, scale=0.02), RC.gaussian((B, per), 72 + per)
    gi = RC.integers((B, per), 73 + per)
    rs = np.random.RandomState(74 + B + per)
    coef, num = rs.uniform(-2.0, 2.0, B).astype(np.float32), rs.uniform(-2.0, 2.0, B).astype(np.float32)
    dg = put(g, off)
    rep = RC.Report('gp rows B %d per %d %s' % (B, per, 'misaligned' if off else 'aligned'))
    s = K.gp_slopes(dg)
    ss, sr = RC.gp_slopes(RC.f64(g))
    rep.check('slopes^2', float((np.abs(RC.f64(s) ** 2 - ss) / ss).max()), SUM)             # measured <= 1.2e-7
    rep.check('row_scale', relerr(K.row_scale(dg, dev(coef)), RC.row_scale(RC.f64(g), RC.f64(coef))), LIN)      # measured <= 4.8e-8
    assert exact(K.row_scale(put(gi, off), dev(RC.pow2_rows(B, 1))), RC.row_scale(RC.f64(gi), RC.f64(RC.pow2_rows(B, 1))))
    rep.check('row_scale_div', relerr(K.row_scale_div(dg, dev(num), s), RC.row_scale_div(RC.f64(g), RC.f64(num), RC.f64(s))), LIN)   # <= 9.0e-8
    for name, eps in (('0', np.zeros(B, np.float32)), ('1', np.ones(B, np.float32)), ('u', rs.uniform(0.0, 1.0, B).astype(np.float32))):
        got = K.interp(dev(eps), dg, put(x, off))
        if name != 'u':
            assert torch.equal(got, dev(x) if name == '0' else dev(g)), name
        rep.check('interp(%s)' % name, relerr(got, RC.interp(RC.f64(eps), RC.f64(g), RC.f64(x))), LIN)          # measured <= 9.4e-8
    rep.done()


def test_row_scale_div_guards_zero_and_tiny_slopes(K):
    """the slope norm's backward where the slope is 0 (coefficient 0, not inf: as tests/test_kernels_gpu.py test_gp_golden) and where it
    is a float32 denormal (the clamp at 1e-30 takes over): finite, and the guarded float64 expression row by row"""
    B, per = 5, 105
    g = RC.gaussian((B, per), 75, offset=0.0, scale=1.0)
    g[1] = 0.0
    g[2] = (RC.f64(g[2]) * 1e-39).astype(np.float32)                  # denormal elements; the row's norm is about 1e-38
    den = np.sqrt((RC.f64(g) ** 2).sum(1)).astype(np.float32)
    assert den[1] == 0.0 and 0.0 < den[2] < np.finfo(np.float32).tiny and float(np.abs(g[2]).max()) > 0.0
    num = np.array([-1.0, 0.5, 2.0, 1.5, -0.5], np.float32)
    got = K.row_scale_div(dev(g), dev(num), dev(den))
    ref = RC.row_scale_div(RC.f64(g), RC.f64(num), RC.f64(den))
    assert bool(torch.isfinite(got).all()) and float(got[1].abs().max()) == 0.0 and float(np.abs(ref[2]).max()) > 1e-10
    rep = RC.Report('row_scale_div guards')
    for r in range(B):
        if r != 1:
            rep.check('row %d' % r, relerr(got[r], ref[r]), LIN)               # measured <= 7.1e-8
    rep.done()


def test_interp_wrapped_grid(K):
    """(3, 196608): more elements than 2048 * 256 threads; the per-sample eps must follow the row across the wrap"""
    B, per = 3, 196608
    assert B * per > 2048 * 256
    g, x = RC.integers((B, per), 76), RC.integers((B, per), 77)
    eps = np.array([0.5, 0.0, 1.0], np.float32)
    assert exact(K.interp(dev(eps), dev(g), dev(x)), RC.interp(RC.f64(eps), RC.f64(g), RC.f64(x)))
