"""The column reductions and the batch-norm family without a GPU: the planner of tests/col_bn_cases.py against the library's workspace
queries on every shape tests/test_col_bn_gpu.py uses (so that "this shape reaches 65 chunks, unfused" cannot drift), the float64
restatements against float64 autograd of the oracle's batch norm (so that the GPU file does not hold a kernel to a copy of itself),
and the refusals of the entry points, which happen before any launch."""
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

RTOL = 1e-12
INVALID, WORKSPACE = -1, -2          # include/t2i_hip.h T2I_ERR_INVALID, T2I_ERR_WORKSPACE (a failed launch is T2I_ERR_LAUNCH = -3)


@pytest.fixture(scope='module')
def L():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    return _lib.lib


def close(got, ref, atol=0.0):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(ref, np.float64), rtol=RTOL, atol=atol)


# ---- the planner against the library -----------------------------------------------------------------------------------------
def lib_chunks(L, rows, C):
    b = int(L.t2i_col_reduce_workspace_bytes(rows, C))
    assert b % (C * 8) == 0
    return b // (C * 8)


def lib_group_chunks(L, rows_g, C, groups):
    b = int(L.t2i_bn_grouped_workspace_bytes(rows_g, C, groups)) // 4 - groups * 3 * C
    assert b % (groups * C * 2) == 0
    return b // (groups * C * 2)


def test_every_shape_of_the_gpu_file_reaches_the_chunk_count_it_states(L):
    for rows, C, chunks in (CB.REDUCE_CASES + CB.MISALIGNED_CASES + CB.BF16_REDUCE_CASES + CB.STATS_CASES + CB.SINGLE_BWD_CASES +
                            CB.SCALAR_BWD_CASES + [(r, c, n) for r, c, _, n in CB.LARGE_MEAN_CASES]):
        assert CB.plan(rows, C)[1] == chunks == lib_chunks(L, rows, C), (rows, C, chunks)
        assert int(L.t2i_col_reduce_workspace_bytes(rows, C)) == CB.ws_bytes(rows, C)
        assert int(L.t2i_bn_bwd_fused_workspace_bytes(rows, C)) == CB.ws_bytes(rows, C) + 12 * C
    for groups, rows_g, C, ncg, fused in CB.GROUPED_CASES + CB.BF16_GROUPED:
        assert CB.group_plan(rows_g, C, groups)[1] == ncg == lib_group_chunks(L, rows_g, C, groups), (groups, rows_g, C)
        assert int(L.t2i_bn_grouped_workspace_bytes(rows_g, C, groups)) == CB.grouped_ws_bytes(rows_g, C, groups)
        assert CB.fused(ncg) == fused, (groups, rows_g, C, ncg)
    for rows, C, off, ncg in CB.LARGE_MEAN_CASES:
        assert CB.group_plan(rows, C, 1)[1] == ncg == lib_group_chunks(L, rows, C, 1)
    for rows, tile_rows, tiles in CB.TILE_CASES:
        assert (rows + tile_rows - 1) // tile_rows == tiles
        assert CB.fused(tiles) == (tiles <= 64)
    for rows_g, tile_rows in CB.TILE_GROUPED:
        assert rows_g % tile_rows == 0 and any(r == rows_g and t == tile_rows for r, t, _ in CB.TILE_CASES)
    # what the case list says about the shapes, in the planner's own terms
    assert CB.chunk_bounds(65, 2, 33) == [(0, 32), (33, 64)]
    assert CB.chunk_bounds(4097, 65, 64)[-1] == (4096, 4096)                          # the one-row last chunk
    assert CB.plan(12289, 4) == (1, 190, 65) and CB.chunk_bounds(12289, 190, 65)[-1] == (12285, 12288)
    assert CB.plan(3072, 1024) == (16, 48, 64) and CB.plan(130, 49216) == (769, 1, 130)
    assert CB.group_plan(101, 8, 3) == (1, 2, 51) and CB.chunk_bounds(101, 2, 51, 3)[1::2] == [(51, 100), (152, 201), (253, 302)]
    assert CB.group_plan(8200, 132, 2) == (3, 96, 86) and CB.plan(8200, 132)[1] == 129
    assert 2 * 8200 * 132 > 2048 * 256 * 4                                             # the float4 grid of an elementwise kernel wraps
    assert CB.group_plan(2, 4, 200) == (1, 1, 2) and CB.group_plan(20, 1028, 3)[0] == 17


def test_plan_sweeps_around_each_clamp(L):
    rows_sweep = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 12287, 12288, 12289, 12290, 24576, 24577, 100000, 3 * 12288 + 5]
    C_sweep = [1, 3, 4, 5, 63, 64, 65, 68, 128, 132, 256, 260, 1024, 1028, 49088, 49152, 49153, 49216]     # ctiles 767 .. 770 around wgs
    for rows in rows_sweep:
        for C in C_sweep:
            ct, nc, rpc = CB.plan(rows, C)
            assert nc == lib_chunks(L, rows, C), (rows, C)
            assert 1 <= nc <= 192 and (nc - 1) * rpc < rows <= nc * rpc and ct == (C + 63) // 64
            assert nc <= (rows + 63) // 64 and nc <= max(768 // ct, 1)
            assert len(CB.chunk_bounds(rows, nc, rpc)) == nc
    for groups in (1, 2, 3, 4, 5, 64, 96, 97, 191, 192, 193, 200, 1000):
        for rows_g in (1, 2, 15, 16, 17, 64, 65, 100, 101, 4096, 4097, 6144, 8200, 12288, 12289, 40000):
            for C in (4, 8, 36, 132, 1028):
                ct, ncg, rpc = CB.group_plan(rows_g, C, groups)
                assert ncg == lib_group_chunks(L, rows_g, C, groups), (groups, rows_g, C)
                assert 1 <= ncg <= max(192 // groups, 1) and (ncg - 1) * rpc < rows_g <= ncg * rpc
                rpb, nb_g = CB.fuse_rows(rows_g, ct, groups)
                assert (nb_g - 1) * rpb < rows_g <= nb_g * rpb and nb_g <= (rows_g + 15) // 16 and nb_g <= max(1024 // (ct * groups), 1)
    assert CB.fuse_rows(7, 1, 1) == (7, 1) and CB.fuse_rows(15, 1, 3) == (15, 1) and CB.fuse_rows(4096, 1, 3) == (16, 256)
    assert CB.fuse_rows(2, 1, 200) == (2, 1) and CB.fuse_rows(20, 17, 3) == (10, 2)      # rows_g < 16; 1024 / 51 = 20 wanted, 2 allowed
    for bad in ((0, 4), (4, 0), (-1, 4)):
        assert int(L.t2i_col_reduce_workspace_bytes(*bad)) == 0 and int(L.t2i_bn_bwd_fused_workspace_bytes(*bad)) == 0
    assert int(L.t2i_bn_grouped_workspace_bytes(4, 4, 0)) == 0 and int(L.t2i_bn_grouped_workspace_bytes(0, 4, 1)) == 0


def test_plan_follows_the_tuning_values(L):
    """wgs and cap are tuning values of the library (colred_wgs, colred_cap): the restatement takes them as arguments"""
    try:
        assert L.t2i_tuning_set(b'colred_wgs', 96.0) == 0 and L.t2i_tuning_set(b'colred_cap', 8.0) == 0
        for rows in (1, 64, 65, 511, 512, 513, 4097):
            for C in (4, 68, 1024, 6144, 6208):
                assert CB.plan(rows, C, wgs=96, cap=8)[1] == lib_chunks(L, rows, C), (rows, C)
                for groups in (1, 3, 8, 9):
                    assert CB.group_plan(rows, C, groups, wgs=96, cap=8)[1] == lib_group_chunks(L, rows, C, groups), (rows, C, groups)
    finally:
        assert L.t2i_tuning_set(b'colred_wgs', 768.0) == 0 and L.t2i_tuning_set(b'colred_cap', 192.0) == 0
    assert lib_chunks(L, 12289, 4) == 190


# ---- the restatements against float64 autograd of the oracle's batch norm ------------------------------------------------------
@pytest.mark.parametrize('act', CB.ACTS)
@pytest.mark.parametrize('groups,rows_g,C', [(1, 1, 4), (1, 7, 8), (2, 9, 5), (3, 101, 8)])
def test_forward_and_backward_restatements_equal_autograd_of_the_oracle(groups, rows_g, C, act):
    """oracle/torch_step.py _bn (training mode, rank 2) + leaky_relu / relu per group; dgamma / dbeta are the gradients of the
    shared gamma / beta over all groups; the moving averages by its apply_bn_moving, one group after the other, twice each."""
    from oracle import torch_step as T
    x = CB.grouped_input(groups, rows_g, C, 3)
    gamma, beta, mm, mv = CB.affine(C, 3)
    dy = np.random.RandomState(9).standard_normal(x.shape)
    P = {'bn/gamma': torch.tensor(gamma, dtype=torch.float64, requires_grad=True),
         'bn/beta': torch.tensor(beta, dtype=torch.float64, requires_grad=True),
         'bn/moving_mean': torch.tensor(mm, dtype=torch.float64), 'bn/moving_variance': torch.tensor(mv, dtype=torch.float64)}
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ys, means, rstds = [], [], []
    for g in range(groups):
        stats = {}
        z = T._bn(P, 'bn', xt[g * rows_g:(g + 1) * rows_g], True, stats, eps=CB.EPS)
        ys.append(z if act == 'none' else torch.nn.functional.leaky_relu(z, CB.ALPHA if act == 'lrelu' else 0.0))
        means.append(stats['bn'][0].numpy()); rstds.append(1.0 / np.sqrt(stats['bn'][1].numpy() + CB.EPS))
        for _ in range(2):
            T.apply_bn_moving(P, stats, decay=CB.DECAY)
    y = torch.cat(ys, 0)
    gx, gg, gb = torch.autograd.grad((y * torch.tensor(dy)).sum(), [xt, P['bn/gamma'], P['bn/beta']])
    fwd = CB.bn_forward(CB.f64(x), gamma, beta, groups, act, moving_mean=mm, moving_var=mv, updates=2)
    close(fwd['y'], y.detach().numpy(), atol=1e-14)
    close(fwd['mean'], np.stack(means), atol=1e-15); close(fwd['rstd'], np.stack(rstds))
    close(fwd['scale'], fwd['rstd'] * CB.f64(gamma)); close(fwd['shift'] + fwd['mean'] * fwd['scale'], np.tile(CB.f64(beta), (groups, 1)), atol=1e-14)
    close(fwd['moving_mean'], P['bn/moving_mean'].numpy(), atol=1e-15); close(fwd['moving_var'], P['bn/moving_variance'].numpy())
    bwd = CB.bn_backward(dy, fwd['y'] if act != 'none' else None, CB.f64(x), fwd['mean'], fwd['rstd'], gamma, groups, act)
    scale = float(np.abs(gx.numpy()).max())
    close(bwd['dx'], gx.numpy(), atol=1e-13 * max(scale, 1.0))         # rows_g = 1: dx is zero up to the rounding of eps-sized terms
    close(bwd['dgamma'], gg.numpy(), atol=1e-12); close(bwd['dbeta'], gb.numpy(), atol=1e-13)
    close(bwd['gmask'], dy * CB.act_grad(fwd['y'], act))
    # the three-coefficient form the kernels use is the same polynomial: k_x is the coefficient of x
    xg, gm = CB.f64(x).reshape(groups, rows_g, C), bwd['gmask'].reshape(groups, rows_g, C)
    k_dy = CB.f64(gamma) * fwd['rstd']
    k_0 = -k_dy * gm.mean(1) - bwd['k_x'] * fwd['mean']
    close(k_dy[:, None] * gm + bwd['k_x'][:, None] * xg + k_0[:, None], bwd['dx'].reshape(groups, rows_g, C), atol=1e-12 * max(scale, 1.0))
    close(bwd['xmax'], np.abs(xg).max(1)); close(bwd['mean'], fwd['mean'])
    # only the first group moves the moving averages
    one = CB.bn_forward(CB.f64(x), gamma, beta, groups, act, moving_mean=mm, moving_var=mv, moving_groups=1)
    first = CB.bn_forward(CB.f64(x)[:rows_g], gamma, beta, 1, act, moving_mean=mm, moving_var=mv)
    close(one['moving_mean'], first['moving_mean']); close(one['moving_var'], first['moving_var'])


def test_statistics_and_reductions_on_hand_made_values():
    x = np.array([[1.0, 10.0], [3.0, 10.0], [8.0, 10.0]])
    s, m2 = CB.bn_stats(x)
    close(s, [12.0, 30.0]); close(m2, [26.0, 0.0])
    f = CB.bn_finalize(s, m2, 3, [2.0, 1.0], [0.5, -1.0], [1.0, 1.0], [2.0, 2.0])
    close(f['mean'], [[4.0, 10.0]]); close(f['var'], [[26.0 / 3.0, 0.0]])
    close(f['moving_mean'], [0.9 + 0.4, 0.9 + 1.0]); close(f['moving_var'], [1.8 + 0.1 * 13.0, 1.8])        # unbiased: 26 / 2
    one = CB.bn_finalize([5.0], [0.0], 1, [1.0], [0.0], [0.0], [1.0])
    close(one['moving_var'], [0.9]); close(one['rstd'], [[1.0 / np.sqrt(CB.EPS)]])                            # n = 1: the factor n / max(n - 1, 1) = 1
    a = np.array([[1, -2], [3, 4], [-5, 6]])
    b = np.array([[2, 2], [0, 1], [1, -1]])
    assert CB.col_sum(a).tolist() == [-1, 8] and CB.col_sum_sq(a).tolist() == [35, 56]
    assert CB.col_sum_prod(a, b).tolist() == [-3, -6] and CB.col_sum_prod(a, b, np.array([1, -1])).tolist() == [-2, 2]
    assert CB.col_sum(a).dtype == np.int64 and CB.col_sum(a.astype(np.float32)).dtype == np.float64
    ps, pm = CB.tile_partials(x, 2)
    close(ps, [[4.0, 20.0], [8.0, 10.0]]); close(pm, [[2.0, 0.0], [0.0, 0.0]])
    assert ps.dtype == np.float32 and CB.tile_partials(np.tile(x, (2, 1)), 2, groups=2)[0].shape == (4, 2)
    close(CB.act_grad(np.array([-1.0, 0.0, 2.0]), 'lrelu'), [0.25, 0.25, 1.0]); close(CB.act_grad(np.array([-1.0, 0.0, 2.0]), 'relu'), [0.0, 0.0, 1.0])


def test_marked_integers_mark_every_chunk_boundary():
    for rows, C, chunks in [(65, 4, 2), (4097, 4, 65), (12289, 4, 190), (4097, 68, 65)]:
        a = CB.marked_integers(rows, C, 1)
        _, nc, rpc = CB.plan(rows, C)
        bounds = CB.chunk_bounds(rows, nc, rpc)
        marked = sorted(set(r for fl in bounds for r in fl))
        assert nc == chunks and len(marked) == 2 * chunks - (1 if rows == 4097 else 0)      # a one-row chunk has one boundary row
        assert all(abs(int(a[r, 0])) >= 1000 for r in marked) and len(set(int(a[r, 0]) for r in marked)) == len(marked)
        rest = np.delete(a, marked, 0)
        assert int(np.abs(rest).max()) <= 3
        CB.assert_exact_in_f32(a)
    small = CB.marked_integers(4097, 8, 2, base=128, span=60)
    assert int(np.abs(small).max()) <= 256 and np.array_equal(CB.bf16_round(small), small.astype(np.float32))
    with pytest.raises(AssertionError):
        CB.assert_exact_in_f32(np.full((20000, 2), 1000))


# ---- refusals: every one before any launch, with the entry point named in the message ---------------------------------------
def refused(L, name, rc, want=INVALID):
    """On a machine without a GPU a launch fails as well (T2I_ERR_LAUNCH): the code and the message tell a refusal from that."""
    msg = L.t2i_last_error().decode('utf-8', 'replace')
    assert rc == want, (name, rc, msg)
    assert msg.startswith(name + ':'), (name, msg)
    assert ('workspace' in msg) == (want == WORKSPACE), msg


_BUF = (ctypes.c_float * 64)()
_AL = (ctypes.addressof(_BUF) + 15) & ~15


@pytest.fixture(scope='module')
def p():
    """a dummy non-null, 16-byte aligned pointer: no refusal reads through it"""
    return ctypes.c_void_p(_AL)


@pytest.fixture(scope='module')
def q():
    """the same, one float further: 4-byte aligned only"""
    return ctypes.c_void_p(_AL + 4)


def each_null(args, idx):
    for i in idx:
        a = list(args)
        a[i] = None
        yield a


def with_(args, **at):
    a = list(args)
    for k, v in at.items():
        a[int(k[1:])] = v
    return a


def test_col_reduce_refusals(L, p, q):
    name, need = 't2i_col_reduce', CB.ws_bytes(100, 8)
    args = [p, None, None, 100, 8, p, None, 0, p, need, 0, None]
    for a in each_null(args, (0, 5)):
        refused(L, name, L.t2i_col_reduce(*a))
    refused(L, name, L.t2i_col_reduce(*with_(args, _3=0)))
    refused(L, name, L.t2i_col_reduce(*with_(args, _4=0)))
    refused(L, name, L.t2i_col_reduce(*with_(args, _2=p)))                    # center without b
    refused(L, name, L.t2i_col_reduce(*with_(args, _9=need - 1)), WORKSPACE)
    refused(L, name, L.t2i_col_reduce(*with_(args, _8=None)), WORKSPACE)
    refused(L, name, L.t2i_col_reduce(*with_(args, _10=7)))                   # no such dtype
    refused(L, name, L.t2i_col_reduce(*with_(args, _0=q, _10=1)))             # bf16 from a misaligned base
    refused(L, name, L.t2i_col_reduce(*with_(args, _4=6, _10=1)))             # bf16 with C % 4 != 0


def test_bn_stats_refusals(L, p):
    name, need = 't2i_bn_stats', CB.ws_bytes(100, 8)
    args = [p, 100, 8, p, p, p, need, None]
    for a in each_null(args, (0, 3, 4)):
        refused(L, name, L.t2i_bn_stats(*a))
    refused(L, name, L.t2i_bn_stats(*with_(args, _1=0)))
    refused(L, name, L.t2i_bn_stats(*with_(args, _2=-4)))
    refused(L, name, L.t2i_bn_stats(*with_(args, _6=need - 1)), WORKSPACE)
    refused(L, name, L.t2i_bn_stats(*with_(args, _5=None)), WORKSPACE)


def test_bn_train_fwd_stats_refusals(L, p, q):
    name, need = 't2i_bn_train_fwd_stats', CB.ws_bytes(100, 8)
    #       x  psum pm2  ch tr rows C  gamma beta eps  decay mean rstd scale shift mm mv ws ws_bytes dtype stream
    args = [p, None, None, 0, 0, 100, 8, p, p, 1e-5, 0.9, p, p, p, p, p, p, p, need, 0, None]
    for a in each_null(args, (7, 8, 11, 12, 13, 14)):
        refused(L, name, L.t2i_bn_train_fwd_stats(*a))
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _0=None)))                                # neither x nor tile partials
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _1=p, _2=p, _3=2, _4=64)))                # both
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _0=None, _1=p, _3=2, _4=64)))             # sums without M2
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _0=None, _1=p, _2=p, _3=0, _4=64)))
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _0=None, _1=p, _2=p, _3=2, _4=0)))
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _0=None, _1=p, _2=p, _3=3, _4=64)))       # (chunks - 1) * tile_rows >= rows
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _0=None, _1=p, _2=p, _3=1, _4=64)))       # chunks * tile_rows < rows
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _16=None)))                               # one moving average without the other
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _5=0)))
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _18=need - 1)), WORKSPACE)
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _17=None)), WORKSPACE)
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _0=q, _19=1)))                            # bf16 from a misaligned base
    refused(L, name, L.t2i_bn_train_fwd_stats(*with_(args, _19=5)))


def test_bn_stats_tiles_refusals(L, p):
    name = 't2i_bn_stats_tiles'
    args = [p, p, 2, 64, 100, 8, p, p, None]
    for a in each_null(args, (0, 1, 6, 7)):
        refused(L, name, L.t2i_bn_stats_tiles(*a))
    for i in (2, 3, 4, 5):
        refused(L, name, L.t2i_bn_stats_tiles(*with_(args, **{'_%d' % i: 0})))
    refused(L, name, L.t2i_bn_stats_tiles(*with_(args, _2=1)))                # the tiles do not cover the rows
    refused(L, name, L.t2i_bn_stats_tiles(*with_(args, _2=3)))                # (chunks - 1) * tile_rows >= rows: a tile of no rows
    refused(L, name, L.t2i_bn_stats_tiles(*with_(args, _2=3, _4=128)))        # ... exactly at the boundary


def test_col_reduce_partials_refusals(L, p):
    name = 't2i_col_reduce_partials'
    args = [p, p, 3, 8, p, p, 0, None]
    for a in each_null(args, (0, 4)):
        refused(L, name, L.t2i_col_reduce_partials(*a))
    refused(L, name, L.t2i_col_reduce_partials(*with_(args, _1=None)))        # out1 without part1
    refused(L, name, L.t2i_col_reduce_partials(*with_(args, _5=None)))        # part1 without out1
    refused(L, name, L.t2i_col_reduce_partials(*with_(args, _2=0)))
    refused(L, name, L.t2i_col_reduce_partials(*with_(args, _3=0)))


def test_bn_finalize_refusals(L, p):
    name = 't2i_bn_finalize'
    args = [p, p, 100, 8, p, p, 1e-5, 0.9, p, p, p, p, p, p, None]
    for a in each_null(args, (0, 1, 4, 5, 8, 9, 10, 11)):
        refused(L, name, L.t2i_bn_finalize(*a))
    refused(L, name, L.t2i_bn_finalize(*with_(args, _2=0)))
    refused(L, name, L.t2i_bn_finalize(*with_(args, _3=0)))
    refused(L, name, L.t2i_bn_finalize(*with_(args, _12=None)))               # one moving average without the other
    refused(L, name, L.t2i_bn_finalize(*with_(args, _13=None)))


def test_bn_apply_refusals(L, p, q):
    name = 't2i_bn_apply'
    args = [p, p, p, 100, 8, 0, 0.2, p, None, 0, None]
    for a in each_null(args, (0, 1, 2, 7)):
        refused(L, name, L.t2i_bn_apply(*a))
    refused(L, name, L.t2i_bn_apply(*with_(args, _3=0)))
    refused(L, name, L.t2i_bn_apply(*with_(args, _4=0)))
    refused(L, name, L.t2i_bn_apply(*with_(args, _8=q)))                      # a misaligned bf16 twin
    refused(L, name, L.t2i_bn_apply(*with_(args, _4=6, _8=p)))                # a twin with C % 4 != 0
    refused(L, name, L.t2i_bn_apply(*with_(args, _0=q, _8=p)))                # a twin of a misaligned x
    refused(L, name, L.t2i_bn_apply(*with_(args, _9=1, _8=p)))                # bf16 storage has no twin
    refused(L, name, L.t2i_bn_apply(*with_(args, _9=1, _1=q)))                # bf16 with a misaligned scale
    refused(L, name, L.t2i_bn_apply(*with_(args, _9=3)))


def test_bn_bwd_refusals(L, p, q):
    name = 't2i_bn_bwd'
    args = [p, p, p, p, p, p, p, 100, 8, p, p, p, 0, p, 96, None]
    for a in each_null(args, (0, 1, 2, 3, 4, 5, 6, 9, 10, 11)):
        refused(L, name, L.t2i_bn_bwd(*a))
    refused(L, name, L.t2i_bn_bwd(*with_(args, _7=0)))
    refused(L, name, L.t2i_bn_bwd(*with_(args, _8=0)))
    refused(L, name, L.t2i_bn_bwd(*with_(args, _14=95)), WORKSPACE)           # three coefficients per column
    refused(L, name, L.t2i_bn_bwd(*with_(args, _13=None)), WORKSPACE)
    refused(L, name, L.t2i_bn_bwd(*with_(args, _13=q)), WORKSPACE)            # the coefficients are read as float4


def test_bn_bwd_fused_refusals(L, p, q):
    name, need = 't2i_bn_bwd_fused', CB.ws_bytes(100, 8) + 96
    #       dy y  x  mean rstd gamma rows C act alpha gmask dx dx_h dgamma dbeta acc ws ws_bytes dtype stream
    args = [p, p, p, p, p, p, 100, 8, 2, 0.2, p, p, None, p, p, 0, p, need, 0, None]
    for a in each_null(args, (0, 2, 3, 4, 5, 11, 13, 14)):
        refused(L, name, L.t2i_bn_bwd_fused(*a))
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _6=0)))
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _7=0)))
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _7=6)))                  # C % 4 != 0
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _10=None)))              # y without gmask
    for i in (0, 1, 2, 3, 10, 11):
        refused(L, name, L.t2i_bn_bwd_fused(*with_(args, **{'_%d' % i: q})))  # misaligned dy, y, x, mean, gmask, dx
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _17=need - 1)), WORKSPACE)
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _16=None)), WORKSPACE)
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _16=q)), WORKSPACE)
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _12=q)))                 # a misaligned dx_h
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _12=p, _18=1)))          # bf16 storage has no twin
    refused(L, name, L.t2i_bn_bwd_fused(*with_(args, _18=2)))


def test_act_bwd_colsum_refusals(L, p, q):
    name, need = 't2i_act_bwd_colsum', CB.ws_bytes(100, 8)
    #       dy y  x2    center rows C act alpha dx dx_h colsum colsum_x2 acc ws ws_bytes dtype stream
    args = [p, p, None, None, 100, 8, 2, 0.2, p, None, p, None, 0, p, need, 0, None]
    for a in each_null(args, (0, 1, 8, 10)):
        refused(L, name, L.t2i_act_bwd_colsum(*a))
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _3=p)))                # center without x2
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _2=p, _11=p, _3=q)))   # a misaligned center
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _2=p)))                # x2 without colsum_x2
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _11=p)))               # colsum_x2 without x2
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _2=q, _11=p)))         # a misaligned x2
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _4=0)))
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _5=6)))                # C % 4 != 0
    for i in (0, 1, 8):
        refused(L, name, L.t2i_act_bwd_colsum(*with_(args, **{'_%d' % i: q})))
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _14=need - 1)), WORKSPACE)
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _13=q)), WORKSPACE)
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _9=q)))                # a misaligned dx_h
    refused(L, name, L.t2i_act_bwd_colsum(*with_(args, _9=p, _15=1)))         # bf16 storage has no twin


def test_grouped_tile_and_moving_refusals(L, p, q):
    """the grouped entries have their refusals in tests/test_host.py; the tile and moving-average arguments this suite drives are restated here"""
    name, need = 't2i_bn_train_fwd_grouped', CB.grouped_ws_bytes(128, 8, 2)
    #       x rows_g C groups gamma beta eps decay mean rstd scale shift mm mv act alpha y y_h tsum tm2 tchunks trows upd mgroups ws ws_bytes dtype stream
    args = [p, 128, 8, 2, p, p, 1e-5, 0.9, p, p, p, p, p, p, 0, 0.2, p, None, p, p, 2, 64, 1, 0, p, need, 0, None]
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _20=3)))          # a tile that starts behind the group
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _20=1)))          # tiles that do not cover the group
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _21=48, _20=3)))  # groups = 2: a tile would straddle the groups
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _19=None)))
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _18=q)))
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _22=0)))
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _22=9)))
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _23=3)))
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _23=-1)))
    refused(L, name, L.t2i_bn_train_fwd_grouped(*with_(args, _25=need - 1)), WORKSPACE)
