"""The minibatch standard deviation to second order.  Every quantity is compared, as max-norm relative `relerr`,
against a float64 torch restatement written here and differentiated by torch.autograd; bounds are those of
tests/test_norm_second_order_gpu.py: 1e-5 the forward, 1e-4 input gradients of first and second order.

Conditioning: the double backward carries 1 / sigma^3, so a comparison in fp32 means something only while no column's sigma is tiny;
every case asserts on the float64 run that the smallest sigma is >= 1e-2 (inputs randn * 1.3 + 0.1 from seed 21 leave >= 1.2e-2).
With G = 2 sigma is |x1 - x2| / 2 up to eps: its second derivative vanishes and the two terms of dL/dx cancel, so dL/dx is held to
1e-4 of max(|ref|max, |k (v - vbar) / sigma|max) — the scale of its first term — in every case."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_norm_second_order_gpu import _store, relerr  # noqa: E402

pytestmark = pytest.mark.gpu

SIGMA_FLOOR = 1e-2


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    return ops


def _sigma64(x, G, eps=1e-8):
    """x [B,H,W,C] -> (d [M,G,H,W,C], sigma [M,H,W,C]) over groups of G contiguous rows"""
    B, H, W, C = x.shape
    xg = x.reshape(B // G, G, H, W, C)
    d = xg - xg.mean(1, keepdim=True)
    return d, torch.sqrt((d ** 2).mean(1) + eps)


def _stat64(x, G, Fs, eps=1e-8):
    """-> (stat [B,Fs], sigma)"""
    B, H, W, C = x.shape
    _, sigma = _sigma64(x, G, eps)
    stat = sigma.reshape(B // G, H, W, Fs, C // Fs).mean((1, 2, 4))
    return stat.repeat_interleave(G, 0), sigma


def _inputs(shape, Fs, seed=21):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 1.3 + 0.1
    gs = torch.randn(shape[0], Fs, generator=g)
    v = torch.randn(shape, generator=g)
    return x, gs, v


def _block_units():
    """kMbBlockUnits of csrc/t2i_ops.hip — units (float4 or float) of a (group, chunk) per workgroup — from the library itself: the
    workspace query counts one float per workgroup of the scalar form, and a (group, chunk) of exactly n floats needs one workgroup
    while n <= kMbBlockUnits; the smallest n that needs two is kMbBlockUnits + 1"""
    from t2i_amd import _lib
    ws = _lib.lib.t2i_minibatch_stddev_workspace_bytes
    n = 1
    while int(ws(1, 1, n, 1, 1, 1)) == 4:
        n *= 2
        assert n <= 1 << 20
    lo, hi = n // 2, n                  # one workgroup at lo, two or more at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if int(ws(1, 1, mid, 1, 1, 1)) == 4 else (lo, mid)
    return lo


def _workgroups(shape, Fs):
    """workgroups per (group, chunk) in the form the kernel takes for this shape (16-byte where (C/F) % 4 == 0: the tensors are aligned)"""
    _, H, W, C = shape
    cf = C // Fs
    return -(-H * W * (cf // 4 if cf % 4 == 0 else cf) // _block_units())


CASES = [((6, 4, 4, 16), 3, 4),          # 16-byte form
         ((8, 3, 5, 6), 4, 2),           # scalar form, C / F = 3
         ((8, 1, 1, 3), 4, 1),           # a one-column-block group
         ((12, 4, 4, 32), 4, 4),         # three groups
         ((32, 4, 4, 512), 4, 4),        # the critic's shape: several workgroups per (group, chunk)
         ((16, 32, 32, 64), 16, 1),      # G at its cap, many partials reach the join
         ((4, 2, 2, 8), 2, 1)]           # G = 2


@pytest.mark.parametrize('shape,G,Fs', CASES)
def test_second_order_parity(ops, shape, G, Fs):
    nblk = _workgroups(shape, Fs)
    if shape in ((32, 4, 4, 512), (16, 32, 32, 64)):
        assert nblk > 1, nblk                               # the join adds more than one partial
    if shape == (16, 32, 32, 64):
        assert nblk >= 16, nblk                             # many partials: the join's strided loop and its butterfly both add
    if shape == (8, 1, 1, 3):
        assert nblk == 1
    x, gs, v = _inputs(shape, Fs)
    xr, gsr = x.double().requires_grad_(True), gs.double().requires_grad_(True)
    statr, sigma = _stat64(xr, G, Fs)
    assert float(sigma.detach().min()) >= SIGMA_FLOOR, float(sigma.detach().min())
    dxr, = torch.autograd.grad(statr, xr, gsr, create_graph=True)
    r_dgs, r_ddx = torch.autograd.grad((dxr * v.double()).sum(), [gsr, xr])
    # the scale of dL/dx's first term, k (v - vbar) / sigma, in float64
    B, H, W, C = shape
    Nf = H * W * C // Fs
    k = gs.double().reshape(B // G, G, Fs).sum(1) / (Nf * G)                                        # [M, Fs]
    k = k.repeat_interleave(C // Fs, 1).reshape(B // G, 1, 1, 1, C)
    vg = v.double().reshape(B // G, G, H, W, C)
    first = k * (vg - vg.mean(1, keepdim=True)) / sigma.detach().unsqueeze(1)
    scale = max(float(r_ddx.abs().max()), float(first.abs().max()))

    xc, gsc = x.cuda().requires_grad_(True), gs.cuda().requires_grad_(True)
    stat = ops.minibatch_stddev_stat(xc, G, Fs)
    assert tuple(stat.shape) == (B, Fs)
    dx, = torch.autograd.grad(stat, xc, gsc, create_graph=True)
    dgs, ddx = torch.autograd.grad((dx * v.cuda()).sum(), [gsc, xc])
    e = dict(stat=relerr(stat, statr), dx=relerr(dx, dxr), dgs=relerr(dgs, r_dgs),
             ddx=float((ddx.double().cpu() - r_ddx).abs().max()) / scale)
    print('minibatch_stddev %s G=%d F=%d: min sigma %.3g  %s  (ddx: |ref|max %.3g, first term %.3g)' % (
        shape, G, Fs, float(sigma.detach().min()), '  '.join('%s %.2e' % kv for kv in e.items()), float(r_ddx.abs().max()), float(first.abs().max())))
    assert e['stat'] <= 1e-5 and e['dx'] <= 1e-4 and e['dgs'] <= 1e-4 and e['ddx'] <= 1e-4, e
    m = stat.reshape(B // G, G, Fs)
    assert torch.equal(m, m[:, :1].expand_as(m))                       # the same bits in every row of a group
    m = dgs.reshape(B // G, G, Fs)
    assert torch.equal(m, m[:, :1].expand_as(m))


@pytest.mark.parametrize('shape,Fs', [((5, 4, 4, 16), 4), ((3, 3, 5, 6), 2)])
def test_group_of_one(ops, shape, Fs):
    """G = 1: d = 0 exactly, so the statistic is sqrt(eps) and both input gradients are exact zeros"""
    x, gs, v = _inputs(shape, Fs)
    xc, gsc = x.cuda().requires_grad_(True), gs.cuda().requires_grad_(True)
    stat = ops.minibatch_stddev_stat(xc, 1, Fs)
    dx, = torch.autograd.grad(stat, xc, gsc, create_graph=True)
    dgs, ddx = torch.autograd.grad((dx * v.cuda()).sum(), [gsc, xc])
    assert float((stat.detach().double() - 1e-4).abs().max()) <= 1e-6 * 1e-4
    assert bool((dx == 0).all()) and bool((ddx == 0).all()) and bool((dgs == 0).all())


def test_parts_are_independent(ops):
    """The critic's 3B pass: the statistic and its gradient for cat[a, b, c] are bit for bit those of a, b and c; calls repeat bit for bit"""
    g = torch.Generator().manual_seed(21)
    parts = [(torch.randn(8, 4, 4, 32, generator=g) * 1.3 + 0.1).cuda() for _ in range(3)]
    gss = [torch.randn(8, 4, generator=g).cuda() for _ in range(3)]
    vs = [torch.randn(8, 4, 4, 32, generator=g).cuda() for _ in range(3)]

    def run(x, gs, v):
        x, gs = x.clone().requires_grad_(True), gs.clone().requires_grad_(True)
        stat = ops.minibatch_stddev_stat(x, 4, 4)
        dx, = torch.autograd.grad(stat, x, gs, create_graph=True)
        dgs, ddx = torch.autograd.grad((dx * v).sum(), [gs, x])
        return stat.detach(), dx.detach(), dgs, ddx
    whole = run(torch.cat(parts), torch.cat(gss), torch.cat(vs))
    again = run(torch.cat(parts), torch.cat(gss), torch.cat(vs))
    single = [run(*t) for t in zip(parts, gss, vs)]
    for i, name in enumerate(('stat', 'dx', 'dgs', 'ddx')):
        assert torch.equal(whole[i], torch.cat([s[i] for s in single])), name
        assert torch.equal(whole[i], again[i]), name
    assert bool(whole[0].abs().max() > 0) and bool(whole[1].abs().max() > 0) and bool(whole[3].abs().max() > 0)


def test_minibatch_stddev_appends_the_tiled_statistic(ops):
    """ops.minibatch_stddev -> [B,H,W,C+F]; then a conv on top, differentiated twice the way the gradient penalty does, against float64"""
    from t2i_amd import scope as S
    shape, G, Fs = (6, 4, 4, 8), 3, 2
    x, _, _ = _inputs(shape, Fs)
    xc = x.cuda().requires_grad_(True)
    y = ops.minibatch_stddev(xc, G, Fs)
    stat = ops.minibatch_stddev_stat(xc, G, Fs)
    assert tuple(y.shape) == (6, 4, 4, 10)
    assert torch.equal(y[..., :8], xc.detach()) and torch.equal(y[..., 8:], stat.detach()[:, None, None, :].expand(6, 4, 4, 2))
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(3, 3, 10, 4, generator=gen) * (2.0 / 90) ** 0.5
    st = S.VariableStore(device='cuda', seed=3)
    with _store(st):
        with st.variable_scope('d_net'):
            h = ops.conv2d(y, 4, ks=(3, 3), s=(1, 1), act=None)
        names = [[n for n in st.vars if n.endswith(k)][0] for k in ('weights', 'biases')]
        assert len(st.vars) == 2 and tuple(st.vars[names[0]].shape) == (3, 3, 10, 4), list(st.vars)
        st.load({names[0]: w.numpy(), names[1]: np.zeros(4, np.float32)})
        with st.variable_scope('d_net', reuse=True):
            h = ops.conv2d(ops.minibatch_stddev(xc, G, Fs), 4, ks=(3, 3), s=(1, 1), act=None)
        out = (h ** 2).sum((1, 2, 3))
        gx, = torch.autograd.grad(out.sum(), xc, create_graph=True)
        loss = (gx ** 2).sum()
        loss.backward(inputs=[xc, st.vars[names[0]]])
        dw = st.vars[names[0]].grad
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    statr, sigma = _stat64(xr, G, Fs)
    assert float(sigma.detach().min()) >= SIGMA_FLOOR
    yr = torch.cat([xr, statr[:, None, None, :].expand(6, 4, 4, 2)], 3)
    hr = F.conv2d(yr.permute(0, 3, 1, 2), wr.permute(3, 2, 0, 1), None, padding=1)
    gxr, = torch.autograd.grad((hr ** 2).sum(), xr, create_graph=True)
    lossr = (gxr ** 2).sum()
    r_dx, r_dw = torch.autograd.grad(lossr, [xr, wr])
    e = dict(gx=relerr(gx, gxr), loss=abs(float(loss.detach()) - float(lossr.detach())) / float(lossr.detach()), ddx=relerr(xc.grad, r_dx), dw=relerr(dw, r_dw))
    print('minibatch_stddev + conv: %s' % '  '.join('%s %.2e' % kv for kv in e.items()))
    assert max(e.values()) <= 1e-4, e


def test_refusals_on_device_tensors(ops):
    """bf16, a stacked pass and a group that does not divide the batch: raised before any launch, naming the operator"""
    from t2i_amd import kernels as K
    from t2i_amd import stacked as ST
    x = torch.zeros(6, 2, 2, 8, device='cuda')
    launches = []
    real = (K.minibatch_stddev_fwd, K.concat_tile_fwd)
    K.minibatch_stddev_fwd = lambda *a, **k: launches.append('fwd') or real[0](*a, **k)
    K.concat_tile_fwd = lambda *a, **k: launches.append('concat') or real[1](*a, **k)
    try:
        for fn in (ops.minibatch_stddev, ops.minibatch_stddev_stat):
            with pytest.raises(ValueError, match='minibatch_stddev'):
                fn(x.bfloat16())
            with pytest.raises(ValueError, match='minibatch_stddev'):
                fn(x, group_size=4)
            with pytest.raises(NotImplementedError, match='minibatch_stddev'):
                fn(ST.Stacked(x[:3], x[3:]))
        assert launches == []
        ops.minibatch_stddev(x, group_size=3)
        assert launches == ['fwd', 'concat']
    finally:
        K.minibatch_stddev_fwd, K.concat_tile_fwd = real
