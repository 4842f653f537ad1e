"""The resampling kernel on the GPU (csrc/t2i_resample.hip) against its float64 restatement
(tests/upfirdn_cases.py): the forward and the adjoint elementwise over the case table, the second backward against the forward bit for
bit, independence of the batch, repeatability, a captured call, the wrapped grid, the scalar form on a misaligned base, and the two
ties with the reference's resampling.

Bound, derived and not measured: |y - ref| <= (n^2 + 2) 2^-24 (sum |g|)^2 max |x| — at most n^2 products and one intermediate rounding."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import upfirdn_cases as UC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    return ops


@pytest.fixture(scope='module')
def K(ops):
    from t2i_amd import kernels
    assert kernels.UPFIRDN_TILE == UC.TILE
    return kernels


def _groups():
    """The case table cut by (u, d) and by its two parts (the 3x5x7x3 cross of taps and pads; the extents x channels cross)."""
    out = {}
    for i, c in enumerate(UC.CASES):
        out.setdefault('u%dd%d-%s' % (c[2], c[3], UC.PART[i]), []).append(i)
    return out


GROUPS = _groups()


def test_the_table_covers_every_dimension():
    cs = UC.CASES
    assert {(c[2], c[3]) for c in cs} == set(UC.UD) and {c[1] for c in cs} == set(UC.TAPS)
    assert {c[0][3] for c in cs} == set(UC.CHANNELS) and {c[0][0] for c in cs} == {1, 3}
    assert {c[0][1:3] for c in cs} >= set(UC.EXTENTS)
    T = UC.TILE
    for axis in (1, 2):
        assert {c[0][axis] for c in cs} >= {T - 1, T, T + 1, 2 * T + 1}
    for u, d in UC.UD:                                              # every kind of pad met under every (u, d)
        kinds = {(c[4], c[5]) for c in cs if (c[2], c[3]) == (u, d)}
        assert {(0, 0), (-1, 0), (3, -1)} <= kinds and any(p0 == len(UC.TAPS[c[1]]) + 2 for c in cs for p0 in (c[4],) if (c[2], c[3]) == (u, d))


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_forward_and_adjoint_against_float64(K, group):
    worst = (0.0, '')
    for i in GROUPS[group]:
        shape, name, u, d, p0, p1, flip = UC.CASES[i]
        f = UC.TAPS[name]
        x, yref, g, aref, adj = UC.reference(i)
        y = K.upfirdn2d(x.cuda(), f, u, d, p0, p1, flip)
        a = K.upfirdn2d(g.cuda(), f, *adj)
        assert tuple(y.shape) == yref.shape and tuple(a.shape) == tuple(shape) == aref.shape, UC.case_id(UC.CASES[i])
        for got, ref, src in ((y, yref, x), (a, aref, g)):
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
            b = UC.bound(f, src.numpy())
            worst = max(worst, (err / b, UC.case_id(UC.CASES[i])))
            assert err <= b, (UC.case_id(UC.CASES[i]), err, b)
    print('upfirdn2d %s: %d cases, largest error / bound %.3f (%s)' % (group, len(GROUPS[group]), worst[0], worst[1]))


PICKS = [((3, 5, 7, 3), 'asym5', 2, 1, 3, -1, True), ((3, 9, 17, 20), 'bin4', 1, 2, 1, 1, False), ((3, 8, 9, 4), 'oct8', 2, 2, 4, 3, True),
         ((3, 17, 7, 68), 'tri3', 1, 1, 1, 1, False), ((3, 2, 3, 1), 'box2', 1, 2, 0, 0, False)]
PICK_IDS = dict(ids=[UC.case_id(c) for c in PICKS])


@pytest.mark.parametrize('case', PICKS, **PICK_IDS)
def test_second_backward_is_the_forward_bit_for_bit(ops, case):
    shape, name, u, d, p0, p1, flip = case
    f = UC.TAPS[name]
    x = UC.inputs(shape).cuda().requires_grad_(True)
    y = ops.upfirdn2d(x, f, up=u, down=d, pad=(p0, p1), flip=flip)
    v = UC.inputs(tuple(y.shape), seed=2).cuda().requires_grad_(True)
    gx, = torch.autograd.grad(y, x, v, create_graph=True)                  # A^T v, by the kernel with the adjoint's parameters
    assert gx.shape == x.shape and gx.requires_grad
    w = UC.inputs(shape, seed=3).cuda()
    ggv, = torch.autograd.grad(gx, v, w)                                   # A w: the backward of the backward
    assert torch.equal(ggv, ops.upfirdn2d(w, f, up=u, down=d, pad=(p0, p1), flip=flip))
    ref = UC.ref_upfirdn2d(v.detach().cpu(), f, *UC.adjoint_of(case))
    assert np.abs(gx.detach().cpu().numpy() - ref).max() <= UC.bound(f, v.detach().cpu().numpy())


@pytest.mark.parametrize('case', PICKS, **PICK_IDS)
def test_a_batch_row_is_the_sample_alone_and_calls_repeat(K, case):
    shape, name, u, d, p0, p1, flip = case
    f = UC.TAPS[name]
    x = UC.inputs(shape).cuda()
    y = K.upfirdn2d(x, f, u, d, p0, p1, flip)
    assert torch.equal(y, K.upfirdn2d(x, f, u, d, p0, p1, flip))
    for b in range(shape[0]):
        assert torch.equal(y[b:b + 1], K.upfirdn2d(x[b:b + 1].contiguous(), f, u, d, p0, p1, flip)), b


def test_a_captured_call_replayed_equals_eager(K):
    shape, name, u, d, p0, p1, flip = PICKS[1]
    f = UC.TAPS[name]
    static = UC.inputs(shape).cuda()
    K.upfirdn2d(static, f, u, d, p0, p1, flip)                             # the kernel is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = K.upfirdn2d(static, f, u, d, p0, p1, flip)
    for seed in (5, 6):
        x = UC.inputs(shape, seed=seed).cuda()
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, K.upfirdn2d(x, f, u, d, p0, p1, flip))


def test_a_batch_beyond_the_grid_limit_is_wrapped(K):
    """B = 70000 of 1 x 1 x 1: more tiles than the launch has workgroups (65535), reached by the stride."""
    x = UC.inputs((70000, 1, 1, 1)).cuda()
    f = UC.TAPS['tri3']
    y = K.upfirdn2d(x, f, 2, 1, 2, 0, False)                               # upsample_2d's pads for three taps
    ref = UC.ref_upfirdn2d(x.cpu(), f, 2, 1, 2, 0)
    assert tuple(y.shape) == ref.shape == (70000, 2, 2, 1)
    assert np.abs(y.cpu().numpy() - ref).max() <= UC.bound(f, x.cpu().numpy())
    assert float(y[65535:].abs().min()) > 0.0                              # the rows past the first sweep were written


def test_a_base_misaligned_by_one_float_takes_the_scalar_form(K):
    shape, f = (3, 9, 8, 4), UC.TAPS['bin4']
    x = UC.inputs(shape)
    n = x.numel()
    buf = torch.zeros(n + 5, device='cuda')
    xm = buf[1:1 + n].view(shape)
    xm.copy_(x)
    assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
    for u, d in UC.UD:
        p0, p1 = UC.helper_pads(4, u, d)
        y = K.upfirdn2d(xm, f, u, d, p0, p1, False)
        ref = UC.ref_upfirdn2d(x, f, u, d, p0, p1)
        assert np.abs(y.cpu().numpy() - ref).max() <= UC.bound(f, x.numpy())
        assert torch.equal(y, K.upfirdn2d(x.cuda(), f, u, d, p0, p1, False))      # the 16-byte form adds the same products in the same order
        out = torch.zeros(y.numel() + 5, device='cuda')
        ym = out[1:1 + y.numel()].view(y.shape)
        assert K.upfirdn2d(x.cuda(), f, u, d, p0, p1, False, out=ym) is ym and torch.equal(ym, y)
        assert float(out[0]) == 0.0 and float(out[1 + y.numel():].abs().max()) == 0.0


@pytest.mark.parametrize('shape', [(2, 4, 4, 3), (3, 8, 8, 16), (2, 9, 7, 4), (1, 16, 16, 68)], ids=lambda s: 'x'.join(map(str, s)))
def test_box_taps_tie_to_upscale_and_pool(ops, shape):
    x = UC.inputs(shape).cuda()
    assert torch.equal(ops.upsample_2d(x, (1, 1)), ops.upscale(x, 2))
    if shape[1] % 2 == 0 and shape[2] % 2 == 0:
        y, p = ops.downsample_2d(x, (1, 1)), ops.pool(x, 2)
        assert y.shape == p.shape
        assert float((y - p).abs().max()) <= 4 * 2.0 ** -24 * float(x.abs().max())


def test_helpers_against_float64_at_the_model_shapes(ops):
    """upsample_2d / downsample_2d with the default taps: the publication's pads, DC gain 1, exactly 2H and H / 2."""
    x = UC.inputs((2, 8, 8, 12)).cuda()
    k = np.asarray((1, 3, 3, 1), dtype=np.float64)
    up, down = ops.upsample_2d(x), ops.downsample_2d(x)
    assert tuple(up.shape) == (2, 16, 16, 12) and tuple(down.shape) == (2, 4, 4, 12)
    for got, ref, f in ((up, UC.ref_upfirdn2d(x.cpu(), 2 * k / 8, 2, 1, 2, 1), 2 * k / 8), (down, UC.ref_upfirdn2d(x.cpu(), k / 8, 1, 2, 1, 1), k / 8)):
        assert np.abs(got.cpu().numpy() - ref).max() <= UC.bound(f, x.cpu().numpy())
    g = ops.upsample_2d(x, gain=4.0)
    assert float((g - 4.0 * up).abs().max()) <= 4 * UC.bound(2 * k / 8, x.cpu().numpy())
