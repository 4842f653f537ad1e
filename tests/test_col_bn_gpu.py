"""The column reductions and the batch-norm family of csrc/t2i_aux.hip against their float64 restatements (tests/col_bn_cases.py), at the
smallest shapes that reach every path: the three first stages (scalar, _small for C <= 4, _v4; fp32 and bf16), the plain and the Chan
second stages (scalar and _v4, from shifted chunks and from a conv's tile partials), the fused and the unfused normalisation and dx
kernels, and every clamp of the planner (one-row last chunk, the cap of 192, 64 against 65 chunks per group, groups = 2, more column
tiles than workgroups wanted, more groups than the cap, fewer than 16 rows per group).  tests/test_col_bn_host.py asserts, against the
library's workspace queries, that each shape reaches the chunk count stated beside it in col_bn_cases.

Bounds.  Integer data whose every partial sum stays below 2^24 is held to the int64 restatement with
torch.equal (`exact`): a dropped or doubled boundary row has no tolerance to hide in.  Otherwise, as max|got - ref| / max|ref|:
  SUM    1e-6   column sums of the statistics            (tests/test_kernels_gpu.py test_bn_stats_are_stable_against_a_large_mean)
  M2     1e-5   centred second moments, hence variances  (the same test)
  FWD    1e-5   y, mean, scale, shift                    (FWD_TOL)
  RSTD   5e-6   rstd                                     (test_grouped_batch_norm_equals_one_pass_per_group)
  MOV    1e-6   moving mean and variance
  GRAD   1e-4   dx, dgamma, dbeta                        (GRAD_TOL)
bf16 storage adds one rounding of the stored element, 2^-8 |ref| per element, to FWD resp. GRAD of max|ref| on y and dx; the
reductions keep their fp32 bounds because the kernels sum unrounded values.  With |mean| >> std two derived terms are added, see
test_large_mean.  The measured values beside the bounds are the largest over the cases of a test on an MI355X (pytest -s prints all)."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import col_bn_cases as CB  # noqa: E402
from col_bn_cases import relerr, f64  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'
SUM, M2, FWD, RSTD, MOV, GRAD = 1e-6, 1e-5, 1e-5, 5e-6, 1e-6, 1e-4
BF16 = 2.0 ** -8
EPS, DECAY, ALPHA = CB.EPS, CB.DECAY, CB.ALPHA


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def kind(K, act):
    return {'none': K.ACT_NONE, 'relu': K.ACT_RELU, 'lrelu': K.ACT_LRELU}[act]


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a, np.float32)).to(dtype).to(DEVICE).contiguous()


def dev_off(a):
    """the same values as a contiguous view that starts one float into a larger buffer: 4-byte aligned, not 16"""
    a = np.asarray(a, np.float32)
    buf = torch.zeros(a.size + 7, dtype=torch.float32, device=DEVICE)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def exact(got, ref):
    """bit equality with the integer restatement, which float32 holds exactly"""
    ref = torch.tensor(np.asarray(ref).astype(np.int64))
    assert int(ref.abs().max()) < (1 << 24), 'the case is not exactly representable'
    return torch.equal(got.detach().float().cpu(), ref.float())


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(K, rc, what):
    assert rc == 0, (what, rc, K.lib.t2i_last_error().decode('utf-8', 'replace'))


def scratch(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEVICE)


def maxerr(got, ref):
    """max|got - ref| / max|ref|; a reference that is zero throughout (M2 of one row) demands exactly zero"""
    return relerr(got, ref)


# ---- 1. plain column sums on marked integers ---------------------------------------------------------------------------------
def reduce_inputs(rows, C, bf16=False):
    """a: markers 1000 + 2 i (bf16: 128 + 2 (i % 60), within the integers bf16 holds); a2 for the square form: markers 30 + 2 (i % 48);
    b in [-2, 2], an integer center in [-1, 1]"""
    a = CB.marked_integers(rows, C, 100 + rows + C, base=128, span=60) if bf16 else CB.marked_integers(rows, C, 100 + rows + C)
    a2 = CB.marked_integers(rows, C, 200 + rows + C, base=30, span=48)
    rs = np.random.RandomState(rows * 7 + C)
    b = rs.randint(-2, 3, size=(rows, C)).astype(np.int64)
    center = rs.randint(-1, 2, size=C).astype(np.int64)
    CB.assert_exact_in_f32(a, a2 * a2, a * (np.abs(b) + 1))
    return a, a2, b, center


def check_col_reduce(K, rows, C, put, dtype=torch.float32):
    a, a2, b, center = reduce_inputs(rows, C, bf16=dtype is torch.bfloat16)
    da, da2, db = put(a), put(a2), put(b)
    if dtype is torch.bfloat16:
        da, da2, db = da.to(dtype), da2.to(dtype), db.to(dtype)
        assert torch.equal(da.float().cpu(), torch.tensor(a).float()) and torch.equal(da2.float().cpu(), torch.tensor(a2).float())
    s, none = K.col_reduce(da)
    assert none is None and exact(s, CB.col_sum(a)), ('sum a', rows, C)
    s, sq = K.col_reduce(da2, want_second=True)
    assert exact(s, CB.col_sum(a2)) and exact(sq, CB.col_sum_sq(a2)), ('sum a, sum a a', rows, C)
    s, sp = K.col_reduce(da, db, True)
    assert exact(s, CB.col_sum(a)) and exact(sp, CB.col_sum_prod(a, b)), ('sum a b', rows, C)
    s, sp = K.col_reduce(da, db, True, center=dev(center))
    assert exact(s, CB.col_sum(a)) and exact(sp, CB.col_sum_prod(a, b, center)), ('sum a (b - center)', rows, C)
    base = np.arange(C, dtype=np.int64) % 17 - 8
    acc = dev(base)
    out, _ = K.col_reduce(da, out=acc)
    assert out is acc and exact(acc, base + CB.col_sum(a)), ('accumulate', rows, C)
    torch.cuda.synchronize()


@pytest.mark.parametrize('rows,C,chunks', CB.REDUCE_CASES)
def test_col_reduce_integers(K, rows, C, chunks):
    check_col_reduce(K, rows, C, dev)


@pytest.mark.parametrize('rows,C,chunks', CB.MISALIGNED_CASES)
def test_col_reduce_integers_from_a_misaligned_base(K, rows, C, chunks):
    """C % 4 == 0 but the tensors start one float into a buffer: C = 4 runs _small, C = 68 the scalar kernel over two column tiles"""
    check_col_reduce(K, rows, C, dev_off)


@pytest.mark.parametrize('rows,C,chunks', CB.BF16_REDUCE_CASES)
def test_col_reduce_integers_bf16(K, rows, C, chunks):
    check_col_reduce(K, rows, C, dev, torch.bfloat16)


@pytest.mark.parametrize('chunks,C', CB.PARTIALS_CASES)
def test_col_reduce_partials_integers(K, chunks, C):
    """t2i_col_reduce_partials on partials of its caller's making: _v4 for C % 4 == 0, the scalar second stage otherwise; 193 rows exceed
    the cap of the library's own first stage, which a caller's partials need not obey"""
    rs = np.random.RandomState(chunks * 31 + C)
    p0 = rs.randint(-100, 101, size=(chunks, C)).astype(np.int64)
    p1 = rs.randint(-100, 101, size=(chunks, C)).astype(np.int64)
    p0[0] += 5000; p0[-1] -= 7000; p1[0] -= 3000; p1[-1] += 9000          # the first and the last row of partials, distinctly
    base0, base1 = np.arange(C, dtype=np.int64) - 3, 5 - np.arange(C, dtype=np.int64)
    d0, d1 = dev(p0), dev(p1)
    for accumulate in (0, 1):
        o0, o1 = dev(base0), dev(base1)
        ok(K, K.lib.t2i_col_reduce_partials(ptr(d0), ptr(d1), chunks, C, ptr(o0), ptr(o1), accumulate, stream()), 'two outputs')
        assert exact(o0, p0.sum(0) + accumulate * base0) and exact(o1, p1.sum(0) + accumulate * base1), (chunks, C, accumulate)
        o0 = dev(base0)
        ok(K, K.lib.t2i_col_reduce_partials(ptr(d0), None, chunks, C, ptr(o0), None, accumulate, stream()), 'one output')
        assert exact(o0, p0.sum(0) + accumulate * base0), (chunks, C, accumulate)
    torch.cuda.synchronize()


ACT_SUM_CASES = [(65, 8, 2), (4097, 8, 65), (12289, 4, 190), (4097, 68, 65), (4097, 132, 65)]


@pytest.mark.parametrize('act', CB.ACTS)
@pytest.mark.parametrize('rows,C,chunks', ACT_SUM_CASES)
def test_act_bwd_colsum_integers(K, rows, C, chunks, act):
    """dy in multiples of 4, so that dy * 0.25 is an integer; y in {-1, 0, 1}: zero takes the negative side"""
    assert CB.plan(rows, C)[1] == chunks
    for dtype in (torch.float32, torch.bfloat16):
        if dtype is torch.bfloat16 and (rows, C) not in ((65, 8), (4097, 68)):
            continue
        dy = CB.marked_integers(rows, C, 300 + rows + C, base=128, span=60, step=4) if dtype is torch.bfloat16 else \
            CB.marked_integers(rows, C, 300 + rows + C, step=4)
        rs = np.random.RandomState(rows + 3 * C)
        y = rs.randint(-1, 2, size=(rows, C)).astype(np.int64)
        x2 = rs.randint(-2, 3, size=(rows, C)).astype(np.int64)
        center = rs.randint(-1, 2, size=C).astype(np.int64)
        g = (dy * CB.act_grad(y, act)).astype(np.int64)
        assert np.array_equal(g, dy * CB.act_grad(y, act))
        CB.assert_exact_in_f32(dy * 4)
        ddy, dyy, dx2 = dev(dy, dtype), dev(y, dtype), dev(x2, dtype)
        assert torch.equal(ddy.float().cpu(), torch.tensor(dy).float())
        dx, s = K.act_bwd_colsum(ddy, dyy, kind(K, act), ALPHA)
        assert dx.dtype == dtype and exact(dx, g) and exact(s, CB.col_sum(g)), ('plain', rows, C, act)
        dx, s, s2 = K.act_bwd_colsum(ddy, dyy, kind(K, act), ALPHA, x2=dx2)
        assert exact(dx, g) and exact(s, CB.col_sum(g)) and exact(s2, CB.col_sum_prod(g, x2)), ('x2', rows, C, act)
        dx, s, s2 = K.act_bwd_colsum(ddy, dyy, kind(K, act), ALPHA, x2=dx2, center=dev(center))
        assert exact(dx, g) and exact(s, CB.col_sum(g)) and exact(s2, CB.col_sum_prod(g, x2, center)), ('center', rows, C, act)
        base = np.arange(C, dtype=np.int64) % 13 - 6
        acc = dev(base)
        dx, s = K.act_bwd_colsum(ddy, dyy, kind(K, act), ALPHA, out=acc)
        assert s is acc and exact(dx, g) and exact(acc, base + CB.col_sum(g)), ('accumulate', rows, C, act)
    torch.cuda.synchronize()


# ---- 2. statistics and finalize ------------------------------------------------------------------------------------------------
def check_forward(rep, tag, ref, mean, rstd, scale, shift, mm=None, mv=None, g=None):
    sel = (lambda a: a) if g is None else (lambda a: a[g])
    rep.check(tag + 'mean', maxerr(mean, sel(ref['mean'])), FWD)
    rep.check(tag + 'rstd', maxerr(rstd, sel(ref['rstd'])), RSTD)
    rep.check(tag + 'scale', maxerr(scale, sel(ref['scale'])), FWD)
    rep.check(tag + 'shift', maxerr(shift, sel(ref['shift'])), FWD)
    if mm is not None:
        rep.check(tag + 'mmean', maxerr(mm, ref['moving_mean']), MOV)
        rep.check(tag + 'mvar', maxerr(mv, ref['moving_var']), MOV)


@pytest.mark.parametrize('rows,C,chunks', CB.STATS_CASES)
def test_statistics_and_finalize(K, rows, C, chunks):
    """bn_stats (the scalar, _small and _v4 first stages with shift = 1, the scalar and _v4 Chan second stages), bn_finalize on their
    result, and bn_train_stats (the finalize folded into the second stage), all against float64 of x.  rows = 1: variance 0, the
    unbiased factor n / max(n - 1, 1) clamped.      measured: sum <= 2.1e-7, M2 <= 1.2e-6, mean / scale / shift <= 3.9e-7, rstd <= 3.6e-7, moving <= 3.3e-7, y <= 4.3e-7"""
    x = CB.gaussian_columns(rows, C, 7 * rows + C)
    gamma, beta, mm, mv = CB.affine(C, rows + C)
    rs, rm2 = CB.bn_stats(f64(x))
    ref = CB.bn_finalize(rs, rm2, rows, gamma, beta, mm, mv)
    ref = dict((k, v[0] if v.ndim == 2 else v) for k, v in ref.items())
    rep = CB.Report('stats rows %d C %d (%d chunks)' % (rows, C, chunks))
    dx = dev(x)
    s, m2 = K.bn_stats(dx)
    rep.check('sum', maxerr(s, rs), SUM)
    rep.check('M2', maxerr(m2, rm2), M2)
    assert float(m2.min()) >= 0.0
    if rows == 1:
        assert float(m2.abs().max()) == 0.0 and torch.equal(s.cpu(), torch.tensor(x[0]))
    dmm, dmv = dev(mm), dev(mv)
    mean, rstd, scale, shift = K.bn_finalize(s, m2, rows, dev(gamma), dev(beta), EPS, DECAY, dmm, dmv)
    check_forward(rep, 'fin ', ref, mean, rstd, scale, shift, dmm, dmv)
    dmm, dmv = dev(mm), dev(mv)
    mean, rstd, scale, shift = K.bn_train_stats(dx, dev(gamma), dev(beta), EPS, DECAY, dmm, dmv)
    check_forward(rep, 'train ', ref, mean, rstd, scale, shift, dmm, dmv)
    mean2, rstd2, scale2, shift2 = K.bn_train_stats(dx, dev(gamma), dev(beta), EPS, DECAY)             # without moving averages
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd) and torch.equal(scale2, scale) and torch.equal(shift2, shift)
    y = K.bn_apply(dx, scale, shift)
    ry = CB.bn_forward(f64(x), gamma, beta)['y']
    if rows > 1:
        rep.check('y', maxerr(y, ry), FWD)
    else:            # one row: y = beta behind scale = gamma / sqrt(eps), the cancellation of test_large_mean, held to its derived bound
        bound = FWD * np.abs(ry).max() + 2e-6 * (np.abs(ref['mean']) * np.abs(ref['scale'])).max()
        rep.check('y / bound', float(np.abs(f64(y) - ry).max() / bound), 1.0)
    torch.cuda.synchronize()
    rep.done()


@pytest.mark.parametrize('rows,C', [(4097, 3), (4097, 5), (4097, 8), (65, 68)])
def test_a_constant_column_has_m2_exactly_zero(K, rows, C):
    """every value equals the chunk's first row, so every shifted sum and every difference of chunk means is exactly zero: M2 is 0.0,
    not a small negative number and not NaN, and rstd is rsqrt(eps)"""
    x = CB.gaussian_columns(rows, C, 5)
    x[:, 0] = np.float32(1.7)
    x[:, C - 1] = np.float32(-300.25)
    gamma, beta, mm, mv = CB.affine(C, 5)
    s, m2 = K.bn_stats(dev(x))
    assert float(m2[0]) == 0.0 and float(m2[C - 1]) == 0.0 and bool(torch.isfinite(m2).all()) and float(m2.min()) >= 0.0
    assert maxerr(s, f64(x).sum(0)) <= SUM
    dmm, dmv = dev(mm), dev(mv)
    mean, rstd, scale, shift = K.bn_train_stats(dev(x), dev(gamma), dev(beta), EPS, DECAY, dmm, dmv)
    assert float(mean[0]) == float(np.float32(1.7)) and float(mean[C - 1]) == -300.25
    ref = CB.bn_forward(f64(x), gamma, beta, moving_mean=mm, moving_var=mv)
    assert maxerr(rstd, ref['rstd'][0]) <= RSTD and maxerr(dmv, ref['moving_var']) <= MOV and maxerr(dmm, ref['moving_mean']) <= MOV
    if C % 4 == 0:
        y, gmean, grstd = K.bn_train_fwd_grouped(dev(x), dev(gamma), dev(beta), EPS, DECAY, 1)
        assert float(gmean[0, 0]) == float(np.float32(1.7)) and float(gmean[0, C - 1]) == -300.25
        assert maxerr(gmean, ref['mean']) <= FWD and maxerr(grstd, ref['rstd']) <= RSTD and bool(torch.isfinite(y).all())
    torch.cuda.synchronize()


# ---- 3. tile partials handed in directly ---------------------------------------------------------------------------------------
def raw_fwd_grouped(K, x, rows_g, C, groups, gamma, beta, mm, mv, act, tsum=None, tm2=None, tchunks=0, trows=0, updates=1, mgroups=0):
    """t2i_bn_train_fwd_grouped with every output visible -> (y, stat [4, groups, C] = mean, rstd, scale, shift)"""
    stat = torch.empty((4, groups, C), dtype=torch.float32, device=DEVICE)
    y = torch.empty_like(x)
    need = int(K.lib.t2i_bn_grouped_workspace_bytes(rows_g, C, groups))
    ws = scratch(need)
    ok(K, K.lib.t2i_bn_train_fwd_grouped(ptr(x), rows_g, C, groups, ptr(gamma), ptr(beta), EPS, DECAY, ptr(stat[0]), ptr(stat[1]), ptr(stat[2]),
                                          ptr(stat[3]), ptr(mm), ptr(mv), act, ALPHA, ptr(y), None, ptr(tsum), ptr(tm2), tchunks, trows, updates,
                                          mgroups, ptr(ws), need, 1 if x.dtype is torch.bfloat16 else 0, stream()), 't2i_bn_train_fwd_grouped')
    return y, stat


@pytest.mark.parametrize('C', [8, 68, 6])
@pytest.mark.parametrize('rows,tile_rows,tiles', CB.TILE_CASES)
def test_tile_partials(K, rows, tile_rows, tiles, C):
    """Per-tile sums and M2 about each tile's own mean, made in float64 from x and rounded to fp32 — not by a conv of this library —
    through t2i_bn_stats_tiles, t2i_bn_train_fwd_stats(x = NULL) and, for C % 4 == 0, t2i_bn_train_fwd_grouped(tile_sum = ...), whose
    65 and 193 tiles take the unfused route; C = 6 is the scalar merge.      measured: sum <= 1.2e-7, M2 <= 1.3e-7, rstd <= 1.1e-7, moving <= 2.1e-7, y <= 1.5e-7"""
    gamma, beta, mm, mv = CB.affine(C, rows + C)
    rep = CB.Report('tiles rows %d by %d (%d tiles) C %d' % (rows, tile_rows, tiles, C))
    for groups in (1, 2):
        if groups == 2 and ((rows, tile_rows) not in CB.TILE_GROUPED or C % 4):
            continue
        x = CB.grouped_input(groups, rows, C, rows + tile_rows + C)
        ps, pm = CB.tile_partials(f64(x), tile_rows, groups)
        assert ps.shape == (groups * tiles, C)
        dps, dpm = dev(ps), dev(pm)
        ref = CB.bn_forward(f64(x), gamma, beta, groups, 'lrelu', moving_mean=mm, moving_var=mv)
        tag = 'g%d ' % groups
        if groups == 1:
            s, m2 = torch.empty(C, device=DEVICE), torch.empty(C, device=DEVICE)
            ok(K, K.lib.t2i_bn_stats_tiles(ptr(dps), ptr(dpm), tiles, tile_rows, rows, C, ptr(s), ptr(m2), stream()), 't2i_bn_stats_tiles')
            rs, rm2 = CB.bn_stats(f64(x))
            rep.check('sum', maxerr(s, rs), SUM)
            rep.check('M2', maxerr(m2, rm2), M2)
            out = [torch.empty(C, device=DEVICE) for _ in range(4)]
            dmm, dmv, dgam, dbet = dev(mm), dev(mv), dev(gamma), dev(beta)
            ok(K, K.lib.t2i_bn_train_fwd_stats(None, ptr(dps), ptr(dpm), tiles, tile_rows, rows, C, ptr(dgam), ptr(dbet), EPS, DECAY,
                                                ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(dmm), ptr(dmv), None, 0, 0, stream()),
               't2i_bn_train_fwd_stats')
            check_forward(rep, 'stats ', ref, out[0], out[1], out[2], out[3], dmm, dmv, g=0)
        if C % 4 == 0:
            dmm, dmv = dev(mm), dev(mv)
            dxx, dgam, dbet = dev(x), dev(gamma), dev(beta)
            y, stat = raw_fwd_grouped(K, dxx, rows, C, groups, dgam, dbet, dmm, dmv, K.ACT_LRELU, dps, dpm, tiles, tile_rows)
            check_forward(rep, tag, ref, stat[0], stat[1], stat[2], stat[3], dmm, dmv)
            rep.check(tag + 'y', maxerr(y, ref['y']), FWD)
    torch.cuda.synchronize()
    rep.done()


# ---- 4. grouped forward and backward against float64 ---------------------------------------------------------------------------
def raw_bwd_grouped(K, dy, y, x, mean, rstd, gamma, rows_g, C, groups, act, dgamma=None, dbeta=None):
    """t2i_bn_bwd_grouped with the masked gradient visible -> (dx, dgamma, dbeta, gmask)"""
    dx = torch.empty_like(x)
    gmask = torch.empty_like(x) if y is not None else None
    acc = dgamma is not None
    if not acc:
        dgamma, dbeta = torch.empty(C, device=DEVICE), torch.empty(C, device=DEVICE)
    need = int(K.lib.t2i_bn_grouped_workspace_bytes(rows_g, C, groups))
    ws = scratch(need)
    ok(K, K.lib.t2i_bn_bwd_grouped(ptr(dy), ptr(y), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), rows_g, C, groups, act, ALPHA, ptr(gmask), ptr(dx),
                                    None, ptr(dgamma), ptr(dbeta), 1 if acc else 0, ptr(ws), need, 1 if x.dtype is torch.bfloat16 else 0, stream()),
       't2i_bn_bwd_grouped')
    return dx, dgamma, dbeta, gmask


@contextlib.contextmanager
def bn_fuse(K, fuse):
    """tuning bn_fuse = 1 (the default: second stage in the consumer's prologue up to 64 chunks) or 0, restored whatever happens"""
    K.tuning_set('bn_fuse', fuse)
    try:
        yield
    finally:
        K.tuning_set('bn_fuse', 1)


def grouped_case(groups, rows_g, C, seed):
    x = CB.grouped_input(groups, rows_g, C, seed)
    dy = np.random.RandomState(seed + 1).standard_normal(x.shape).astype(np.float32)
    return (x, dy) + CB.affine(C, seed)


@pytest.mark.parametrize('act', CB.ACTS)
@pytest.mark.parametrize('groups,rows_g,C,ncg,fused', CB.GROUPED_CASES)
def test_grouped_forward_and_backward(K, groups, rows_g, C, ncg, fused, act):
    """t2i_bn_train_fwd_grouped / t2i_bn_bwd_grouped with bn_fuse 1 and 0, both held to float64 and never to each other.  The backward's
    reference takes what the kernel takes: dy, the activation's output, x, and the stored per-group mean and rstd.
    measured: y <= 6.6e-7, rstd <= 5.9e-7, scale / shift <= 4.9e-7, moving <= 3.4e-7, dx <= 2.0e-6, dgamma <= 2.4e-7, dbeta <= 4.1e-7"""
    x, dy, gamma, beta, mm, mv = grouped_case(groups, rows_g, C, 11 * groups + rows_g + C)
    ref = CB.bn_forward(f64(x), gamma, beta, groups, act, moving_mean=mm, moving_var=mv)
    dx_, ddy, dgam, dbet = dev(x), dev(dy), dev(gamma), dev(beta)
    rep = CB.Report('grouped %d x %d x %d (%d chunks, %s) %s' % (groups, rows_g, C, ncg, 'fused' if fused else 'unfused', act))
    base_g, base_b = np.linspace(-2.0, 2.0, C).astype(np.float32), np.linspace(3.0, -1.0, C).astype(np.float32)

    def run(fuse):
        tag = 'f%d ' % fuse
        dmm, dmv = dev(mm), dev(mv)
        y, mean, rstd = K.bn_train_fwd_grouped(dx_, dgam, dbet, EPS, DECAY, groups, kind(K, act), ALPHA, dmm, dmv)
        stat = mean._base                                  # the wrapper's [4, groups, C] block: mean, rstd, scale, shift
        assert tuple(stat.shape) == (4, groups, C) and stat[1].data_ptr() == rstd.data_ptr()
        check_forward(rep, tag, ref, mean, rstd, stat[2], stat[3], dmm, dmv)
        rep.check(tag + 'y', maxerr(y, ref['y']), FWD)
        yy = y if act != 'none' else None
        rb = CB.bn_backward(f64(dy), f64(y) if yy is not None else None, f64(x), f64(mean), f64(rstd), gamma, groups, act)
        dxk, dg, db = K.bn_bwd_grouped(ddy, yy, dx_, mean, rstd, dgam, groups, kind(K, act), ALPHA)
        rep.check(tag + 'dx', maxerr(dxk, rb['dx']), GRAD)
        rep.check(tag + 'dgamma', maxerr(dg, rb['dgamma']), GRAD)
        rep.check(tag + 'dbeta', maxerr(db, rb['dbeta']), GRAD)
        acc_g, acc_b = dev(base_g), dev(base_b)
        dxa, og, ob, gmask = raw_bwd_grouped(K, ddy, yy, dx_, mean, rstd, dgam, rows_g, C, groups, kind(K, act), acc_g, acc_b)
        assert torch.equal(dxa, dxk), 'dx must not depend on the accumulate flag'
        rep.check(tag + 'dgamma+', float(np.abs(f64(acc_g) - (f64(base_g) + rb['dgamma'])).max() / np.abs(rb['dgamma']).max()), GRAD)
        rep.check(tag + 'dbeta+', float(np.abs(f64(acc_b) - (f64(base_b) + rb['dbeta'])).max() / np.abs(rb['dbeta']).max()), GRAD)
        if yy is not None:
            assert torch.equal(gmask.cpu(), torch.tensor(rb['gmask']).float()), 'the masked gradient is dy times 1, 0 or alpha'

    for fuse in (1, 0):
        with bn_fuse(K, fuse):
            run(fuse)
    torch.cuda.synchronize()
    rep.done()


@pytest.mark.parametrize('groups,rows_g,C', [(3, 15, 36), (3, 101, 8), (3, 4096, 8), (2, 6144, 8), (200, 2, 4)])
def test_moving_updates_and_moving_groups(K, groups, rows_g, C):
    """moving_updates = 2: every group's statistics enter the moving averages twice in a row; moving_groups = 1: only the first group
    moves them, the later ones leave them untouched.      measured: moving <= 4.2e-7"""
    x, _, gamma, beta, mm, mv = grouped_case(groups, rows_g, C, 5 * groups + rows_g)
    rep = CB.Report('moving %d x %d x %d' % (groups, rows_g, C))

    def run(fuse):
        for updates, mgroups in ((2, 0), (1, 1), (2, 1), (1, groups)):
            ref = CB.bn_forward(f64(x), gamma, beta, groups, moving_mean=mm, moving_var=mv, updates=updates, moving_groups=mgroups)
            dmm, dmv = dev(mm), dev(mv)
            y, mean, rstd = K.bn_train_fwd_grouped(dev(x), dev(gamma), dev(beta), EPS, DECAY, groups, K.ACT_NONE, ALPHA, dmm, dmv,
                                                   moving_updates=updates, moving_groups=mgroups)
            tag = 'f%d u%d g%d ' % (fuse, updates, mgroups)
            rep.check(tag + 'mmean', maxerr(dmm, ref['moving_mean']), MOV)
            rep.check(tag + 'mvar', maxerr(dmv, ref['moving_var']), MOV)
            rep.check(tag + 'mean', maxerr(mean, ref['mean']), FWD)            # every group is still normalised
            rep.check(tag + 'y', maxerr(y, ref['y']), FWD)
        if groups > 1:
            only = CB.bn_forward(f64(x)[:rows_g], gamma, beta, 1, moving_mean=mm, moving_var=mv)
            dmm, dmv = dev(mm), dev(mv)
            K.bn_train_fwd_grouped(dev(x), dev(gamma), dev(beta), EPS, DECAY, groups, K.ACT_NONE, ALPHA, dmm, dmv, moving_groups=1)
            rep.check('f%d first group only' % fuse, max(maxerr(dmm, only['moving_mean']), maxerr(dmv, only['moving_var'])), MOV)

    for fuse in (1, 0):
        with bn_fuse(K, fuse):
            run(fuse)
    torch.cuda.synchronize()
    rep.done()


@pytest.mark.parametrize('act', ['none', 'lrelu'])
@pytest.mark.parametrize('rows,C,chunks', CB.SINGLE_BWD_CASES + CB.SCALAR_BWD_CASES)
def test_single_group_backward(K, rows, C, chunks, act):
    """bn_bwd_fused (C % 4 == 0), and bn_bwd after col_reduce(center = mean) resp. act_bwd_colsum: the coefficient kernel on its own and,
    at C = 6, the scalar bn_bwd_apply_kernel<false>.      measured: dx <= 5.0e-7, dgamma <= 1.6e-7, dbeta <= 2.3e-7"""
    x, dy, gamma, beta, mm, mv = grouped_case(1, rows, C, rows + 13 * C)
    dx_, ddy, dgam = dev(x), dev(dy), dev(gamma)
    mean, rstd, scale, shift = K.bn_train_stats(dx_, dgam, dev(beta), EPS, DECAY)
    y = K.bn_apply(dx_, scale, shift, kind(K, act), ALPHA)
    yy = y if act != 'none' else None
    rb = CB.bn_backward(f64(dy), f64(y) if yy is not None else None, f64(x), f64(mean), f64(rstd), gamma, 1, act)
    rep = CB.Report('backward rows %d C %d (%d chunks) %s' % (rows, C, chunks, act))
    base_g, base_b = np.linspace(-2.0, 2.0, C).astype(np.float32), np.linspace(3.0, -1.0, C).astype(np.float32)
    if C % 4 == 0:
        dxk, dg, db = K.bn_bwd_fused(ddy, yy, dx_, mean, rstd, dgam, kind(K, act), ALPHA)
        rep.check('fused dx', maxerr(dxk, rb['dx']), GRAD)
        rep.check('fused dgamma', maxerr(dg, rb['dgamma']), GRAD)
        rep.check('fused dbeta', maxerr(db, rb['dbeta']), GRAD)
        acc_g, acc_b = dev(base_g), dev(base_b)
        dxa, _, _ = K.bn_bwd_fused(ddy, yy, dx_, mean, rstd, dgam, kind(K, act), ALPHA, dgamma_out=acc_g, dbeta_out=acc_b)
        assert torch.equal(dxa, dxk)
        rep.check('fused dgamma+', float(np.abs(f64(acc_g) - (f64(base_g) + rb['dgamma'])).max() / np.abs(rb['dgamma']).max()), GRAD)
        rep.check('fused dbeta+', float(np.abs(f64(acc_b) - (f64(base_b) + rb['dbeta'])).max() / np.abs(rb['dbeta']).max()), GRAD)
    if yy is not None and C % 4 == 0:
        g, sdy, sdyx = K.act_bwd_colsum(ddy, yy, kind(K, act), ALPHA, x2=dx_, center=mean)
        assert torch.equal(g.cpu(), torch.tensor(rb['gmask']).float())
    else:
        g = ddy if yy is None else dev(rb['gmask'])
        sdy, sdyx = K.col_reduce(g, dx_, True, center=mean)
    rep.check('sum g', maxerr(sdy, rb['dbeta']), GRAD)
    rep.check('sum g (x - mean)', maxerr(sdyx * rstd, rb['dgamma']), GRAD)
    dxk, dg, db = K.bn_bwd(g, dx_, mean, rstd, dgam, sdy, sdyx)
    rep.check('dx', maxerr(dxk, rb['dx']), GRAD)
    rep.check('dgamma', maxerr(dg, rb['dgamma']), GRAD)
    rep.check('dbeta', maxerr(db, rb['dbeta']), GRAD)
    acc_g, acc_b = dev(base_g), dev(base_b)
    dxa, _, _ = K.bn_bwd(g, dx_, mean, rstd, dgam, sdy, sdyx, dgamma_out=acc_g, dbeta_out=acc_b)
    assert torch.equal(dxa, dxk)
    rep.check('dgamma+', float(np.abs(f64(acc_g) - (f64(base_g) + rb['dgamma'])).max() / np.abs(rb['dgamma']).max()), GRAD)
    rep.check('dbeta+', float(np.abs(f64(acc_b) - (f64(base_b) + rb['dbeta'])).max() / np.abs(rb['dbeta']).max()), GRAD)
    torch.cuda.synchronize()
    rep.done()


@pytest.mark.parametrize('act', ['none', 'lrelu'])
@pytest.mark.parametrize('groups,rows_g,C,ncg,fused', CB.BF16_GROUPED)
def test_grouped_bf16_storage(K, groups, rows_g, C, ncg, fused, act):
    """bf16 tensors in and out; the float64 reference takes the bf16-rounded inputs.  y and dx are stored rounded: the fp32 bound on the
    value before it is rounded, plus one bf16 rounding (half an ulp, at most 2^-8 |ref|) per element.  The statistics and the
    reductions keep their fp32 bounds: the kernels sum unrounded values (tests/test_storage_gpu.py).  alpha = 0.25 keeps the masked
    gradient exact in bf16.      measured: y <= 0.97 of its bound (a value just above a power of two meets the
    half ulp), dx <= 0.92, dgamma <= 1.2e-7, dbeta <= 2.8e-7"""
    x, dy, gamma, beta, mm, mv = grouped_case(groups, rows_g, C, 3 * groups + rows_g)
    x, dy = CB.bf16_round(x), CB.bf16_round(dy)
    ref = CB.bn_forward(f64(x), gamma, beta, groups, act, moving_mean=mm, moving_var=mv)
    dx_, ddy, dgam = dev(x, torch.bfloat16), dev(dy, torch.bfloat16), dev(gamma)
    dmm, dmv = dev(mm), dev(mv)
    rep = CB.Report('bf16 %d x %d x %d (%s) %s' % (groups, rows_g, C, 'fused' if fused else 'unfused', act))
    y, mean, rstd = K.bn_train_fwd_grouped(dx_, dgam, dev(beta), EPS, DECAY, groups, kind(K, act), ALPHA, dmm, dmv)
    assert y.dtype is torch.bfloat16
    stat = mean._base
    check_forward(rep, '', ref, mean, rstd, stat[2], stat[3], dmm, dmv)
    bound = FWD * np.abs(ref['y']).max() + BF16 * np.abs(ref['y'])
    rep.check('y / bound', float((np.abs(f64(y) - ref['y']) / bound).max()), 1.0)
    yy = y if act != 'none' else None
    rb = CB.bn_backward(f64(dy), f64(y) if yy is not None else None, f64(x), f64(mean), f64(rstd), gamma, groups, act)
    dxk, dg, db, gmask = raw_bwd_grouped(K, ddy, yy, dx_, mean, rstd, dgam, rows_g, C, groups, kind(K, act))
    assert dxk.dtype is torch.bfloat16
    bound = GRAD * np.abs(rb['dx']).max() + BF16 * np.abs(rb['dx'])
    rep.check('dx / bound', float((np.abs(f64(dxk) - rb['dx']) / bound).max()), 1.0)
    rep.check('dgamma', maxerr(dg, rb['dgamma']), GRAD)
    rep.check('dbeta', maxerr(db, rb['dbeta']), GRAD)
    if yy is not None:
        assert gmask.dtype is torch.bfloat16 and torch.equal(gmask.float().cpu(), torch.tensor(rb['gmask']).float())
    dxw, dgw, dbw = K.bn_bwd_grouped(ddy, yy, dx_, mean, rstd, dgam, groups, kind(K, act), ALPHA)
    assert torch.equal(dxw, dxk) and torch.equal(dgw, dg) and torch.equal(dbw, db)
    torch.cuda.synchronize()
    rep.done()


# ---- 5. |mean| >> std: the two cancellations -------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['grouped', 'unfused grouped', 'stats+apply+bwd_fused'])
@pytest.mark.parametrize('rows,C,offset,chunks', CB.LARGE_MEAN_CASES)
def test_large_mean(K, rows, C, offset, chunks, route):
    """x = offset + unit noise.  Both y = x scale + shift and dx = k_dy dy + k_x x + k_0 subtract two numbers of the size of
    |mean| |scale| resp. |k_x| |mean| to leave one of the size of the result, so their error is set by the roundings of the large
    numbers.  The bounds are derived from the kernels' arithmetic, with the reference's scale, k_x and mean:
      |y - ref|  <= FWD max|ref|  + 2e-6 max_c(|mean_c| |scale_c|)
          the mean is held to 1e-6 of its size (SUM), so mean scale inside shift is off by up to 1e-6 |mean scale|; x scale and
          beta - mean scale round once each, 2 * 2^-24 |mean scale| = 1.2e-7 more, and the rounding of scale itself by 2^-24 acts on
          (x - mean), not on x: together below 2e-6 |mean scale|;
      |dx - ref| <= GRAD max|ref| + 8 * 2^-24 max_c(|k_x,c| (|mean_c| + max|x_c|))
          k_x x rounds once (2^-24 |k_x| max|x|), k_0 = -k_dy mean(g) + (k_dy rstd mean sdyxh / n) holds a product of four factors
          and a division whose roundings each move it by 2^-24 |k_x mean| (5 of them), the sum k_x x + k_0 rounds once more, and
          k_x itself carries 3 roundings that act on x - mean only once k_0 is formed from the same factors.
    measured (MI355X), largest ratio of error to bound: y 0.022, dx 0.053 (both at 2 rows, offset 300) — recorded per case in DESIGN.md section 4.37."""
    rs = np.random.RandomState(rows + C)
    x = (offset + rs.standard_normal((rows, C))).astype(np.float32)
    dy = rs.standard_normal((rows, C)).astype(np.float32)
    gamma, beta, mm, mv = CB.affine(C, rows)
    ref = CB.bn_forward(f64(x), gamma, beta, 1, 'none')
    dx_, ddy, dgam, dbet = dev(x), dev(dy), dev(gamma), dev(beta)
    if route == 'stats+apply+bwd_fused':
        mean, rstd, scale, shift = K.bn_train_stats(dx_, dgam, dbet, EPS, DECAY)
        y = K.bn_apply(dx_, scale, shift)
        dxk, dg, db = K.bn_bwd_fused(ddy, None, dx_, mean, rstd, dgam, K.ACT_NONE, ALPHA)
    else:
        with bn_fuse(K, 0 if route.startswith('unfused') else 1):
            y, mean, rstd = K.bn_train_fwd_grouped(dx_, dgam, dbet, EPS, DECAY, 1)
            dxk, dg, db = K.bn_bwd_grouped(ddy, None, dx_, mean, rstd, dgam, 1, K.ACT_NONE, ALPHA)
    torch.cuda.synchronize()
    rb = CB.bn_backward(f64(dy), None, f64(x), f64(mean), f64(rstd), gamma, 1, 'none')
    y_err = float(np.abs(f64(y) - ref['y']).max())
    y_t1, y_t2 = FWD * float(np.abs(ref['y']).max()), 2e-6 * float((np.abs(ref['mean']) * np.abs(ref['scale'])).max())
    dx_err = float(np.abs(f64(dxk) - rb['dx']).max())
    dx_t1, dx_t2 = GRAD * float(np.abs(rb['dx']).max()), 8 * 2.0 ** -24 * float((np.abs(rb['k_x']) * (np.abs(rb['mean']) + rb['xmax'])).max())
    print('  large mean rows %d C %d offset %g %s: y err %.3e <= %.3e + %.3e (ratio %.3f), dx err %.3e <= %.3e + %.3e (ratio %.3f)' % (
        rows, C, offset, route, y_err, y_t1, y_t2, y_err / (y_t1 + y_t2), dx_err, dx_t1, dx_t2, dx_err / (dx_t1 + dx_t2)))
    rep = CB.Report('large mean rows %d C %d offset %g %s' % (rows, C, offset, route))
    rep.check('mean', maxerr(mean.reshape(-1), ref['mean'][0]), SUM)
    rep.check('rstd', maxerr(rstd.reshape(-1), ref['rstd'][0]), RSTD)
    rep.check('y / bound', y_err / (y_t1 + y_t2), 1.0)
    rep.check('dx / bound', dx_err / (dx_t1 + dx_t2), 1.0)
    rep.check('dgamma', maxerr(dg, rb['dgamma']), GRAD)
    rep.check('dbeta', maxerr(db, rb['dbeta']), GRAD)
    rep.done()
