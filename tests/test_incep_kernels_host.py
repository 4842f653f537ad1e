"""tests/incep_kernel_cases.py without a GPU: every restatement against an independent float64 statement (torch.nn.functional on an
explicitly TF-padded tensor, torch.autograd, np.cov, a hand expansion), the sensitivity of the case tables (a corrupted restatement
changes at least one case), the exactness conditions the GPU tests' equalities rest on, and the refusals of the C entry points,
which come before any launch and any pointer is touched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import incep_kernel_cases as IC  # noqa: E402

OPS = (IC.POOL_MAX, IC.POOL_AVG)


# ---- pool: the restatement ----------------------------------------------------------------------------------------------------
def _torch_pool(x, KH, KW, SH, SW, padding, op):
    """float64, by torch.nn.functional on an explicitly padded tensor: -inf padding for max; sum-pool of x over sum-pool of ones
    for avg"""
    t = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    _, pt, pb = IC.tf_geometry(t.shape[2], KH, SH, padding)
    _, pl, pr = IC.tf_geometry(t.shape[3], KW, SW, padding)
    if op == IC.POOL_MAX:
        out = F.max_pool2d(F.pad(t, (pl, pr, pt, pb), value=float('-inf')), (KH, KW), (SH, SW))
    else:
        area = KH * KW
        num = F.avg_pool2d(F.pad(t, (pl, pr, pt, pb)), (KH, KW), (SH, SW)) * area
        den = F.avg_pool2d(F.pad(torch.ones_like(t), (pl, pr, pt, pb)), (KH, KW), (SH, SW)) * area
        out = num / den.round()
    return out.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('g', IC.POOL_GEOMETRIES, ids=lambda g: 'x'.join(str(v) for v in g))
def test_pool_restatement_matches_torch_on_a_padded_tensor(g):
    B, H, W, KH, KW, SH, SW, padding = g
    for kind in IC.POOL_KINDS:
        x = IC.pool_input((B, H, W, 5), kind, IC.pool_seed(g, 5))
        got = IC.pool(x, KH, KW, SH, SW, padding, IC.POOL_MAX)
        assert np.array_equal(got, _torch_pool(x, KH, KW, SH, SW, padding, IC.POOL_MAX))
        got = IC.pool(x, KH, KW, SH, SW, padding, IC.POOL_AVG)
        np.testing.assert_allclose(got, _torch_pool(x, KH, KW, SH, SW, padding, IC.POOL_AVG), rtol=1e-13, atol=1e-13)


def test_tf_geometry_known_answers():
    # tf.nn.*_pool shapes and pads: SAME out = ceil(n / s), odd pad pixel after; VALID out = floor((n - k) / s) + 1
    assert IC.tf_geometry(8, 3, 1, 'SAME') == (8, 1, 1)
    assert IC.tf_geometry(9, 4, 3, 'SAME') == (3, 0, 1)
    assert IC.tf_geometry(8, 4, 3, 'SAME') == (3, 1, 1)
    assert IC.tf_geometry(5, 2, 1, 'SAME') == (5, 0, 1)
    assert IC.tf_geometry(4, 5, 1, 'SAME') == (4, 2, 2)
    assert IC.tf_geometry(9, 3, 4, 'SAME') == (3, 1, 1)
    assert IC.tf_geometry(9, 3, 2, 'VALID') == (4, 0, 0)
    assert IC.tf_geometry(8, 8, 1, 'VALID') == (1, 0, 0)


def test_pool_class_table_names_the_form_the_launcher_picks():
    for name, C, sl, xoff, form in IC.POOL_CLASSES:
        ld, c0 = sl if sl else (C, 0)
        assert IC.pool_form(C, ld, c0, not xoff) == form, name
    assert {f for *_, f in IC.POOL_CLASSES} == {'scalar', 'vector'}
    for rows, C, ld, c0, xoff, form in IC.SLICE_COPY_CASES:
        assert IC.pool_form(C, ld, c0, not xoff) == form
        assert (rows * C // (4 if form == 'vector' else 1)) % 256 != 0
    # the ragged last block the table promises: 3x8x8 outputs x 12 / 4 channel groups
    assert 3 * 8 * 8 * (12 // 4) == 576 and 576 % 256 != 0


# ---- pool: the sensitivity of the table ---------------------------------------------------------------------------------------
def _faulty_pool(x, KH, KW, SH, SW, padding, op, fault=None):
    """The definition again with one error switched on; with none it must equal IC.pool (asserted below)."""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    if fault == 'k_swapped':
        KH, KW = KW, KH
    if fault == 's_swapped':
        SH, SW = SW, SH
    Ho, pt, pb = IC.tf_geometry(H, KH, SH, padding)
    Wo, pl, pr = IC.tf_geometry(W, KW, SW, padding)
    if fault == 'pad_top_left':
        pt, pl = pb, pr
    if fault == 'origin_off_by_one':
        pt, pl = pt - 1, pl - 1
    out = np.zeros((B, Ho, Wo, C))
    for oy in range(Ho):
        for ox in range(Wo):
            taps = [(oy * SH - pt + i, ox * SW - pl + j) for i in range(KH) for j in range(KW)]
            inside = [x[:, iy, ix] for iy, ix in taps if 0 <= iy < H and 0 <= ix < W]
            if op == IC.POOL_MAX:
                if fault == 'max_pad_zero' and len(inside) < len(taps):
                    inside = inside + [np.zeros((B, C))]
                out[:, oy, ox] = np.max(inside, 0) if inside else -np.inf
            else:
                n = len(taps) if fault == 'avg_full_window' else len(inside)
                out[:, oy, ox] = np.sum(inside, 0) / max(n, 1) if inside else 0.0
    return out


POOL_FAULTS = (('max_pad_zero', (IC.POOL_MAX,)), ('avg_full_window', (IC.POOL_AVG,)), ('k_swapped', OPS), ('s_swapped', OPS),
               ('pad_top_left', OPS), ('origin_off_by_one', OPS))


def _pool_table(fault):
    """{(geometry, kind, op): result} over the table, with C = 3 (the channel classes do not enter the definition)"""
    out = {}
    for g in IC.POOL_GEOMETRIES:
        B, H, W, KH, KW, SH, SW, padding = g
        for kind in IC.POOL_KINDS:
            x = IC.pool_input((B, H, W, 3), kind, IC.pool_seed(g, 3))
            for op in OPS:
                out[g, kind, op] = _faulty_pool(x, KH, KW, SH, SW, padding, op, fault)
    return out


@pytest.fixture(scope='module')
def pool_table():
    return _pool_table(None)


def test_faulty_pool_without_a_fault_is_the_restatement(pool_table):
    for (g, kind, op), want in pool_table.items():
        B, H, W, KH, KW, SH, SW, padding = g
        x = IC.pool_input((B, H, W, 3), kind, IC.pool_seed(g, 3))
        got = IC.pool(x, KH, KW, SH, SW, padding, op)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14, (g, kind, op)


@pytest.mark.parametrize('fault,ops', POOL_FAULTS, ids=[f for f, _ in POOL_FAULTS])
def test_pool_table_sees_each_corruption(pool_table, fault, ops):
    bad = _pool_table(fault)
    for op in ops:
        changed = [(g, kind) for g in IC.POOL_GEOMETRIES for kind in IC.POOL_KINDS
                   if bad[g, kind, op].shape != pool_table[g, kind, op].shape or not np.array_equal(bad[g, kind, op], pool_table[g, kind, op])]
        assert changed, (fault, op)
        assert any(kind == 'negative' for _, kind in changed), (fault, op)
    for op in set(OPS) - set(ops):            # and the op the corruption does not touch is unchanged
        assert all(np.array_equal(bad[g, kind, op], pool_table[g, kind, op]) for g in IC.POOL_GEOMETRIES for kind in IC.POOL_KINDS)


def test_old_pool_input_cannot_see_padding_read_as_zero():
    """What the table is for: on randn + 3 (tests/test_eval_gpu.py) a max pool that reads padding as 0 gives the same answer unless a
    whole window is negative; on the 'negative' kind every padded window differs."""
    g = IC.POOL_GEOMETRIES[-1]
    B, H, W, KH, KW, SH, SW, padding = g
    x = np.abs(np.random.default_rng(43).standard_normal((B, H, W, 3))).astype(np.float32) + 3
    assert np.array_equal(_faulty_pool(x, KH, KW, SH, SW, padding, IC.POOL_MAX, 'max_pad_zero'), IC.pool(x, KH, KW, SH, SW, padding, IC.POOL_MAX))
    x = IC.pool_input((B, H, W, 3), 'negative', 1)
    assert (x < 0).all()
    assert not np.array_equal(_faulty_pool(x, KH, KW, SH, SW, padding, IC.POOL_MAX, 'max_pad_zero'), IC.pool(x, KH, KW, SH, SW, padding, IC.POOL_MAX))


def test_pool_inputs_meet_their_exactness_conditions():
    for g in IC.POOL_GEOMETRIES:
        B, H, W, KH, KW, SH, SW, padding = g
        for _, C, _, _, _ in IC.POOL_CLASSES:
            x = IC.pool_input((B, H, W, C), 'negative', IC.pool_seed(g, C))
            assert x.dtype == np.float32 and (x < 0).all()
            x = IC.pool_input((B, H, W, C), 'integer', IC.pool_seed(g, C))
            assert x.dtype == np.float32 and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 4 and x.min() < 0 < x.max()
            total, count = IC.pool_sum_count(x, KH, KW, SH, SW, padding)
            assert count.min() >= 1 and count.max() <= KH * KW
            # every partial sum of a window, in any order, is an integer of magnitude <= 4 KH KW < 2^24: exact in float32
            assert 4 * KH * KW < 2 ** 24 and np.array_equal(total.astype(np.float32).astype(np.float64), total)
            if padding == 'SAME' and (KH > 1 or KW > 1):
                assert count.min() < KH * KW            # some output has padded taps
    B, H, W, KH, KW, SH, SW, padding = IC.POOL_GEOMETRIES[2]
    assert IC.pool_sum_count(np.zeros((B, H, W, 1)), KH, KW, SH, SW, padding)[1].max() < KH * KW      # there, every output has


# ---- gram -------------------------------------------------------------------------------------------------------------------------
def test_gram_restatement_matches_np_cov_and_np_mean():
    rs = np.random.RandomState(3)
    n, d = 57, 9
    X = (rs.standard_normal((n, d)) * 3 + 100).astype(np.float32)
    s = X[0].copy()
    G, sm = IC.gram(X, s, np.zeros((d, d)), np.zeros(d))
    # (X - s) is exact in float32 here?  Not in general: the identity below is about the float32 differences, so form them first
    diff = (X - s[None, :]).astype(np.float64)
    np.testing.assert_allclose(sm / n, diff.mean(0), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose((G - np.outer(sm, sm) / n) / (n - 1), np.cov(diff, rowvar=False), rtol=1e-11, atol=1e-11)
    # and against the activations themselves: the float32 differences cost at most eps_f32 |X - s| per element
    np.testing.assert_allclose(s + sm / n, X.astype(np.float64).mean(0), rtol=1e-6)
    np.testing.assert_allclose((G - np.outer(sm, sm) / n) / (n - 1), np.cov(X.astype(np.float64), rowvar=False), rtol=0, atol=1e-4)
    # accumulation: two calls are one call on the stacked rows, and the starting values are added once
    G0, s0 = rs.randint(-9, 9, (d, d)).astype(np.float64), rs.randint(-9, 9, d).astype(np.float64)
    Ga, sa = IC.gram(X[:20], s, G0, s0)
    Gb, sb = IC.gram(X[20:], s, Ga, sa)
    np.testing.assert_allclose(Gb, G0 + G, rtol=1e-13)
    np.testing.assert_allclose(sb, s0 + sm, rtol=1e-13)


def _gram_table(fn):
    out = {}
    for d in IC.GRAM_DIMS:
        for seq in IC.GRAM_SEQUENCES:
            Xs, s, G, sm = IC.gram_inputs(d, seq)
            for X in Xs:
                G, sm = fn(X, s, G, sm)
            out[d, seq] = (G, sm)
    return out


def test_gram_table_sees_each_corruption():
    good = _gram_table(IC.gram)

    def no_shift(X, s, G0, sum0):
        return IC.gram(X, np.zeros_like(s), G0, sum0)

    def overwrite(X, s, G0, sum0):
        return IC.gram(X, s, np.zeros_like(G0), np.zeros_like(sum0))

    def drop_last_odd_row(X, s, G0, sum0):
        return IC.gram(X[:len(X) - len(X) % 2], s, G0, sum0)[0], IC.gram(X, s, G0, sum0)[1]

    for bad in (no_shift, overwrite, drop_last_odd_row):
        t = _gram_table(bad)
        for d in IC.GRAM_DIMS:                # every width on its own sees it
            assert any(not np.array_equal(t[d, seq][0], good[d, seq][0]) for seq in IC.GRAM_SEQUENCES), (bad.__name__, d)
    for bad in (no_shift, overwrite):
        t = _gram_table(bad)
        for d in IC.GRAM_DIMS:
            assert any(not np.array_equal(t[d, seq][1], good[d, seq][1]) for seq in IC.GRAM_SEQUENCES), (bad.__name__, d)


def test_gram_inputs_meet_their_exactness_conditions():
    assert IC.GRAM_FLUSH == 64
    assert any(sum(seq) % 2 for seq in IC.GRAM_SEQUENCES) and any(n > IC.GRAM_FLUSH and n % IC.GRAM_FLUSH == 1 for seq in IC.GRAM_SEQUENCES for n in seq)
    for d in IC.GRAM_DIMS:
        for seq in IC.GRAM_SEQUENCES:
            Xs, s, G0, sum0 = IC.gram_inputs(d, seq)
            assert (s != 0).all() and (G0 != 0).all() and (sum0 != 0).all()
            assert np.array_equal(G0, np.round(G0)) and np.array_equal(sum0, np.round(sum0))
            G_abs, s_abs = np.abs(G0), np.abs(sum0)
            for X in Xs:
                assert X.dtype == np.float32 and s.dtype == np.float32 and np.array_equal(X, np.round(X)) and np.array_equal(s, np.round(s))
                diff = X.astype(np.float64) - s.astype(np.float64)
                assert np.array_equal((X - s[None, :]).astype(np.float64), diff)          # the float32 difference is exact
                a = np.abs(diff)
                for k0 in range(0, len(X), IC.GRAM_FLUSH):                                  # each 64-row run, summed in float32
                    assert (a[k0:k0 + IC.GRAM_FLUSH].T @ a[k0:k0 + IC.GRAM_FLUSH]).max() < 2 ** 24
                G_abs, s_abs = G_abs + a.T @ a, s_abs + a.sum(0)
            assert G_abs.max() < 2 ** 53 and s_abs.max() < 2 ** 53                        # and the float64 totals


# ---- dropout ----------------------------------------------------------------------------------------------------------------------
def test_dropout_mask_keep_rate_is_binomial():
    """1e5 draws at keep = 0.8: the count of ones is Binomial(1e5, p) with p = 0.8 up to the 2^-24 grid of u; five standard
    deviations, 5 sqrt(1e5 * 0.8 * 0.2) = 632 draws, is a bound a correct generator misses about once in 1.7 million seeds."""
    n = 100000
    for seed, step in IC.DROPOUT_STREAMS:
        m = IC.dropout_mask(seed, step, 1, n, 0.8)
        assert m.dtype == np.float32 and m.shape == (1, n) and set(np.unique(m)) == {0.0, 1.0}
        assert abs(m.sum() - 0.8 * n) <= 5 * np.sqrt(n * 0.8 * 0.2), (seed, step, m.sum())
    assert (IC.dropout_mask(5, 10, 3, 172, 1.0) == 1).all()
    # the four streams differ from each other (the high words enter), and a mask is a function of (seed, step) alone
    ms = [IC.dropout_mask(seed, step, 1, n, 0.8) for seed, step in IC.DROPOUT_STREAMS]
    for i in range(4):
        for j in range(i):
            assert abs((ms[i] == ms[j]).mean() - 0.68) < 0.01         # independent draws agree with probability .8^2 + .2^2
    assert np.array_equal(ms[0], IC.dropout_mask(5, 10, 1, n, 0.8))
    # the layout: element e takes word e % 4 of quad e // 4, whatever B and D are
    assert np.array_equal(IC.dropout_mask(5, 10, 4, 100, 0.8).ravel(), ms[0].ravel()[:400])


def test_dropout_mask_threshold_is_the_float32_sum():
    """mask = floor(fl32(keep + u)): with keep = 0.8f = 13421773 * 2^-24 and u = k * 2^-24 the sum reaches 1 exactly from
    k = 3355443 on, so the first word's top 24 bits decide"""
    k = np.array([3355442, 3355443], np.float32) * np.float32(2.0 ** -24)
    assert list(np.floor(np.float32(0.8) + k)) == [0.0, 1.0]
    assert list(np.floor(np.float32(0.5) + np.array([0.5 - 2.0 ** -24, 0.5], np.float32))) == [0.0, 1.0]


def test_dropout_tables_reach_what_they_name():
    quads = [B * D // 4 for B, _, D, _ in IC.DROPOUT_SHAPES]
    assert quads[:3] == [1, 129, 1285] and 1285 % 256 != 0 and -(-1285 // 256) == 6
    assert all(D % 4 == 0 for _, _, D, _ in IC.DROPOUT_SHAPES) and any(k == 1.0 for *_, k in IC.DROPOUT_SHAPES)
    assert any(seed >> 32 for seed, _ in IC.DROPOUT_STREAMS) and any(step >> 32 for _, step in IC.DROPOUT_STREAMS)
    lo = {(seed & 0xffffffff, step & 0xffffffff) for seed, step in IC.DROPOUT_STREAMS[:3]}
    assert len(lo) == 1                       # the first three differ in their high words only


# ---- the softmax head -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', IC.HEAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', IC.HEAD_KINDS)
def test_head_restatement_matches_autograd(shape, kind):
    y, W, b, labels = IC.head_inputs(*shape, kind)
    ref = IC.head(y, W, b, labels)
    ty, tW, tb = (torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in (y, W, b))
    logits = ty @ tW + tb
    logits.retain_grad()
    loss = F.cross_entropy(logits, torch.from_numpy(labels.astype(np.int64)))
    loss.backward()
    loss = float(loss.detach())
    assert np.isfinite(ref['loss']) and abs(ref['loss'] - loss) <= 1e-12 * max(abs(loss), 1.0)
    np.testing.assert_allclose(ref['logits'], logits.detach().numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(ref['prob'], torch.softmax(logits.detach(), 1).numpy(), rtol=1e-11, atol=1e-300)
    # prob - onehot where a label's probability is nearly 1 is a float64 difference good to 2^-53 absolutely, not relatively:
    # 1e-15 of the largest input magnitude allows for it in dz and in what is summed from dz
    floor = 1e-15 * max(np.abs(y).max(), np.abs(W).max(), 1.0)
    for k, t in (('dz', logits), ('dW', tW), ('db', tb), ('dy', ty)):
        assert np.abs(ref[k] - t.grad.numpy()).max() <= 1e-12 * np.abs(t.grad.numpy()).max() + floor, k
    assert ref['acc'] == float((logits.detach().argmax(1) == torch.from_numpy(labels.astype(np.int64))).double().mean())


def test_head_inputs_hold_what_the_table_promises():
    underflows = 0
    for shape in IC.HEAD_SHAPES:
        B, D, C = shape
        assert (D + C) * 4 <= IC.HEAD_LDS_LIMIT and B * C * 4 <= IC.HEAD_LDS_LIMIT and C <= 1024
        for kind in IC.HEAD_KINDS:
            y, W, b, labels = IC.head_inputs(B, D, C, kind)
            assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() < C          # never out of range
            assert labels[0] == 0 and (B < 2 or labels[1] == C - 1)
            ref = IC.head(y, W, b, labels)
            if B >= 2 and C >= 2:                                                               # the tie, exact in any arithmetic
                t = (C - 1) // 2
                lg = ref['logits'][B - 1]
                assert np.array_equal(lg, b.astype(np.float64)) and lg[t] == lg[C - 1] == lg.max() and (np.delete(lg, [t, C - 1]) < lg.max()).all()
                assert labels[B - 1] == (t if B >= 3 else C - 1) and int(np.argmax(lg)) == t
            # accuracy is asserted exactly: the other rows' two largest logits are far enough apart for float32 to order them
            top = np.sort(ref['logits'][:max(B - 1, 1)], 1)
            if C >= 2:
                assert (top[:, -1] - top[:, -2]).min() >= 1e-4 * max(np.abs(top).max(), 1.0), (shape, kind)
            if kind == 'wide':
                assert np.abs(ref['logits']).max() >= 45.0 or B * C < 100
                underflows += int((ref['prob'][np.arange(B), labels] < 2.0 ** -149).any())
    assert underflows >= 2                    # a label probability below float32's smallest subnormal
    assert {(2, 16380, 4), (16, 8, 1024)} <= set(IC.HEAD_SHAPES)
    assert (16380 + 4) * 4 == IC.HEAD_LDS_LIMIT and 16 * 1024 * 4 == IC.HEAD_LDS_LIMIT
    assert set(IC.HEAD_ACCUMULATE_SHAPES) <= set(IC.HEAD_SHAPES)


def test_per_column_error_sees_what_the_max_norm_hides():
    ref = np.array([[100.0, 1e-3], [50.0, 2e-3]])
    got = ref.copy()
    got[1, 1] *= 1.5                          # a rare class's column, wrong by half
    assert IC.relerr(got, ref) <= 1e-5 and IC.relerr_cols(got, ref) == pytest.approx(0.5)
    assert IC.relerr_rows(got.T, ref.T) == pytest.approx(0.5)
    assert IC.relerr_cols(np.zeros((2, 2)), np.zeros((2, 2))) == 0.0
    assert IC.relerr_cols(np.array([[0.0, 1e-40]]), np.zeros((1, 2))) > 1.0
    assert IC.relerr_cols(np.array([[0.0, 1e-40]]), np.zeros((1, 2)), floor=1e-30) == pytest.approx(1e-10)
    assert IC.mismatches(np.array([1.0, 2.0, -0.0]), np.array([1.0, 2.5, 0.0])) == 1


# ---- scatter, slice copy ----------------------------------------------------------------------------------------------------------
def test_scatter_and_slice_copy_restatements():
    rs = np.random.RandomState(1)
    for B, HW, D, widths, c0s in IC.SCATTER_CASES:
        assert len(widths) == len(c0s) <= IC.MAX_SCATTER_BRANCHES and D % 4 == 0
        assert all(w % 4 == 0 and c % 4 == 0 and c + w <= D for w, c in zip(widths, c0s))
        spans = sorted((c, c + w) for w, c in zip(widths, c0s))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                          # branches do not overlap
        g = rs.standard_normal((B, D)).astype(np.float32)
        m = (rs.random_sample((B, D)) < 0.8).astype(np.float32)
        for keep in IC.SCATTER_KEEPS:
            outs32 = IC.scatter(g, m, keep, HW, c0s, widths)
            outs64 = IC.scatter(g.astype(np.float64), m.astype(np.float64), keep, HW, c0s, widths)
            for o32, o64, w, c0 in zip(outs32, outs64, widths, c0s):
                assert o32.dtype == np.float32 and o32.shape == o64.shape == (B, HW, w)
                for p in range(HW):                                                         # spelled out per pixel
                    np.testing.assert_allclose(o64[:, p], g[:, c0:c0 + w].astype(np.float64) * m[:, c0:c0 + w] / keep / HW, rtol=1e-15)
                assert np.abs(o32 - o64).max() <= 3 * IC.EPS32 * np.abs(o64).max()          # three float32 roundings
    assert any(list(c0s) != sorted(c0s) and sum(widths) < D for _, _, D, widths, c0s in IC.SCATTER_CASES)
    assert any(len(widths) == IC.MAX_SCATTER_BRANCHES and {4, 512} <= set(widths) for *_, widths, _ in IC.SCATTER_CASES)
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    assert int(re.search(r'#define T2I_MAX_SCATTER_BRANCHES (\d+)', header).group(1)) == IC.MAX_SCATTER_BRANCHES
    assert re.search(r'T2I_POOL_MAX = (\d+), T2I_POOL_AVG = (\d+)', header).groups() == (str(IC.POOL_MAX), str(IC.POOL_AVG))
    x, y = np.arange(6.0).reshape(2, 3), np.full((2, 7), -1.0)
    assert np.array_equal(IC.slice_copy(x, y, 2), [[-1, -1, 0, 1, 2, -1, -1], [-1, -1, 3, 4, 5, -1, -1]]) and (y == -1).all()


# ---- RMSProp ----------------------------------------------------------------------------------------------------------------------
def test_rmsprop_restatement_matches_a_hand_expansion():
    """three steps of one element, momentum != 0, every intermediate written out"""
    lr, rho, mu, eps = 0.5, 0.75, 0.5, 0.25
    g1, g2, g3 = 2.0, -1.0, 0.0
    ms1 = 1.0 + (4.0 - 1.0) * 0.25            # 1.75
    mom1 = 0.5 * 0.0 + 0.5 * 2.0 / np.sqrt(1.75 + 0.25)
    w1 = 3.0 - mom1
    ms2 = 1.75 + (1.0 - 1.75) * 0.25          # 1.5625
    mom2 = 0.5 * mom1 + 0.5 * -1.0 / np.sqrt(1.5625 + 0.25)
    w2 = w1 - mom2
    ms3 = 1.5625 + (0.0 - 1.5625) * 0.25      # 1.171875
    mom3 = 0.5 * mom2 + 0.0
    w3 = w2 - mom3
    w, ms, mom = np.array([3.0]), np.array([1.0]), np.array([0.0])
    for g, want in ((g1, (w1, ms1, mom1)), (g2, (w2, ms2, mom2)), (g3, (w3, ms3, mom3))):
        w, ms, mom = IC.rmsprop(w, np.array([g]), ms, mom, lr, rho, mu, eps)
        np.testing.assert_allclose([w[0], ms[0], mom[0]], want, rtol=1e-15)
    assert mom1 == pytest.approx(0.5 * 2.0 / np.sqrt(2.0)) and ms3 == 1.171875 and mom3 != 0.0


def _rmsprop_table(fn):
    out = {}
    for n, (rho, mu, eps), zero_ms in IC.RMSPROP_CASES:
        if n > 2000:
            continue                          # the definition is elementwise: the large size adds nothing on the host
        w, gs = IC.rmsprop_inputs(n)
        w, ms, mom = w.astype(np.float64), np.zeros(n) if zero_ms else np.ones(n), np.zeros(n)
        for g in gs:
            w, ms, mom = fn(w, g.astype(np.float64), ms, mom, IC.RMSPROP_LR, rho, mu, eps)
        out[n, rho, mu, eps, zero_ms] = (w, ms, mom)
    return out


def test_rmsprop_table_sees_each_corruption():
    good = _rmsprop_table(IC.rmsprop)

    def no_momentum(w, g, ms, mom, lr, rho, mu, eps):
        return IC.rmsprop(w, g, ms, mom, lr, rho, 0.0, eps)

    def eps_outside(w, g, ms, mom, lr, rho, mu, eps):
        ms = ms + (g * g - ms) * (1.0 - rho)
        mom = mu * mom + lr * g / (np.sqrt(ms) + eps)
        return w - mom, ms, mom

    for bad in (no_momentum, eps_outside):
        t = _rmsprop_table(bad)
        # beyond the bound the GPU test asserts, not merely different
        seen = [k for k in good if (np.abs(t[k][0] - good[k][0]) > 1e-6 * np.abs(good[k][0]) + 1e-12).any()]
        assert seen, bad.__name__
        if bad is no_momentum:
            assert all(k[2] != 0.0 for k in seen)
    # what the merged test could not see: at momentum = 0 dropping the momentum term changes nothing
    t = _rmsprop_table(no_momentum)
    assert all(np.array_equal(t[k][0], good[k][0]) for k in good if k[2] == 0.0)


def test_rmsprop_inputs_hold_what_the_table_promises():
    assert max(IC.RMSPROP_SIZES) > IC.RMSPROP_GRID_CAP and IC.RMSPROP_GRID_CAP == 2048 * 256
    assert any(z for *_, z in IC.RMSPROP_CASES) and {p for _, p, _ in IC.RMSPROP_CASES} == set(IC.RMSPROP_PARAMS)
    w, gs = IC.rmsprop_inputs(1003)
    assert len(gs) == IC.RMSPROP_STEPS == 3
    mags = np.abs(np.concatenate(gs))
    assert (mags == 0).any() and mags[mags > 0].min() >= 0.99e-4 and mags.max() <= 10.0 and mags[mags > 0].min() < 1e-3 and mags.max() > 1.0
    signs = np.sign(np.stack(gs))
    assert (signs.max(0) * signs.min(0) >= 0).all() and (signs > 0).any() and (signs < 0).any()      # one sign per element


# ---- the C entry points refuse before they launch ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    return _lib.lib


P, ODD = ctypes.c_void_p(4096), ctypes.c_void_p(4100)


def test_pool2d_rejects_bad_arguments_before_launching(lib):
    """Every call below is invalid, so nothing is launched and no pointer is touched (the pointers are dummies)."""
    def call(x=P, B=1, H=8, W=8, C=8, KH=3, KW=3, SH=1, SW=1, same=1, op=IC.POOL_AVG, y=P, ld=8, c0=0):
        return lib.t2i_pool2d(x, B, H, W, C, KH, KW, SH, SW, same, op, y, ld, c0, None)
    for bad in (dict(SH=5), dict(SW=5), dict(SH=0), dict(ld=12, c0=5), dict(ld=7), dict(c0=-4, ld=16), dict(op=2), dict(x=None), dict(y=None),
                dict(B=0), dict(C=0), dict(KH=0)):
        assert call(**bad) == -1, bad
        assert b't2i_pool2d: bad argument' in lib.t2i_last_error()
    for bad in (dict(same=0, KH=9), dict(same=0, KW=9), dict(same=0, H=2, W=2)):
        assert call(**bad) == -1, bad
        assert b'empty output' in lib.t2i_last_error()


def test_pool_dropout_rejects_bad_arguments_before_launching(lib):
    def call(x=P, B=2, HW=4, D=8, keep=0.8, pre=P, mask=P, y=P):
        return lib.t2i_pool_dropout(x, B, HW, D, keep, 5, 10, pre, mask, y, None)
    for bad in (dict(D=6), dict(D=0), dict(keep=0.0), dict(keep=1.5), dict(keep=-0.5), dict(keep=float('nan')), dict(x=ODD), dict(pre=ODD),
                dict(mask=ODD), dict(y=ODD), dict(x=None), dict(B=0), dict(HW=0)):
        assert call(**bad) == -1, bad
        assert b't2i_pool_dropout: bad argument' in lib.t2i_last_error()


def test_pooled_grad_scatter_rejects_bad_arguments_before_launching(lib):
    def call(widths=(8, 4), c0s=(0, 8), D=16, keep=0.8, g=P, mask=P, outs=None, n=None):
        k = len(widths)
        ptrs = (ctypes.c_void_p * max(k, 1))(*(outs if outs is not None else [4096] * k))
        return lib.t2i_pooled_grad_scatter(g, mask, 2, 3, D, keep, k if n is None else n, ptrs, (ctypes.c_int32 * max(k, 1))(*c0s),
                                           (ctypes.c_int32 * max(k, 1))(*widths), None)
    many = IC.MAX_SCATTER_BRANCHES + 1
    for bad in (dict(widths=(6, 4)), dict(widths=(8, 0)), dict(c0s=(0, 6)), dict(c0s=(0, -4)), dict(c0s=(0, 16)), dict(c0s=(12, 0)), dict(D=14),
                dict(widths=(4,) * many, c0s=tuple(range(0, 4 * many, 4)), D=4 * many), dict(n=0), dict(keep=0.0), dict(g=ODD), dict(mask=ODD),
                dict(outs=[4096, 4100]), dict(outs=[4096, 0]), dict(g=None)):
        assert call(**bad) == -1, bad
        assert b't2i_pooled_grad_scatter: bad argument' in lib.t2i_last_error()


def test_softmax_ce_head_rejects_bad_arguments_before_launching(lib):
    ws = ctypes.c_void_p(8192)

    def call(B=4, D=64, C=8, wsn=None, wsp=ws, y=P):
        need = lib.t2i_softmax_ce_head_workspace_bytes(B, C)
        return lib.t2i_softmax_ce_head(y, P, P, P, B, D, C, P, P, P, P, P, P, 0, P, wsp, need if wsn is None else wsn, None)
    # the backward kernel stages B * C floats of LDS, the forward kernel D + C: neither may pass 65536 bytes, and no launcher
    # raises that limit
    for bad in (dict(B=17, C=1024), dict(B=16385, C=1), dict(C=1025, B=1), dict(D=16384, C=4), dict(D=16381, C=4), dict(D=15361, C=1024, B=1),
                dict(D=16384, C=1, B=1), dict(D=20000), dict(B=0), dict(D=0), dict(C=0), dict(y=None)):
        assert call(**bad) == -1, bad
        assert b't2i_softmax_ce_head: bad argument' in lib.t2i_last_error()
    assert call(wsn=4 * 8 * 4) == -2 and call(wsp=None) == -2
    assert b'workspace' in lib.t2i_last_error()
    assert 16384 * 4 == IC.HEAD_LDS_LIMIT
