"""layer_norm and pixel_norm to second order: what a critic under the gradient penalty needs from them.  Every
quantity is compared, as max-norm relative `relerr`, against a float64 torch restatement written here and differentiated by
torch.autograd.  Bounds are those of tests/test_ops_surface_gpu.py: 1e-5 a normalisation's forward, 1e-4 input gradients (first and
second order), 1e-5 parameter gradients.

Kink condition: lrelu / relu are piecewise linear, so a comparison means something only while the fp32 run takes the float64 run's
branches.  Every case with an activation asserts on the float64 reference that no pre-activation is closer to zero than 1e-4 (inputs
randn * 1.3 + 0.1 from seed 21 leave more than 1e-3); cases with more than a few thousand elements run without an activation."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KINK = 1e-4


def relerr(got, ref, floor=1e-30):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), floor))


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    return ops


@contextlib.contextmanager
def _store(st):
    from t2i_amd import scope as S
    prev = S._DEFAULT[0]
    S.set_default_store(st)
    try:
        yield st
    finally:
        S.set_default_store(prev)


def _act64(t, act):
    if act is None:
        return t
    return {'lrelu': lambda v: F.leaky_relu(v, 0.2), 'relu': torch.relu, 'tanh': torch.tanh}[act](t)


def _fused(ops, act):
    return {None: None, 'lrelu': ops.lrelu_act(0.2), 'relu': ops.relu, 'tanh': ops.tanh}[act]


def _kind(act):
    from t2i_amd import kernels as K
    return {None: (K.ACT_NONE, 0.0), 'lrelu': (K.ACT_LRELU, 0.2), 'relu': (K.ACT_RELU, 0.0), 'tanh': (K.ACT_TANH, 0.0)}[act]


def _ln64(x, gamma, beta, act):
    """-> (y, pre-activation): per sample over everything but axis 0, biased variance, eps 1e-12, per-channel affine on the last axis"""
    dims = tuple(range(1, x.dim()))
    mu = x.mean(dims, keepdim=True)
    var = ((x - mu) ** 2).mean(dims, keepdim=True)
    z = (x - mu) / torch.sqrt(var + 1e-12) * gamma + beta
    return _act64(z, act), z


def _pn64(x, act):
    u = _act64(x, act)
    return u / torch.sqrt((u ** 2).mean(-1, keepdim=True) + 1e-8), x


def _second_order(y, x, extra, dy, v):
    """(dx, [dL/ddy, dL/dx] + dL/d(extra)) with L = <dx, v>, dx = d<y, dy>/dx kept differentiable"""
    dx, = torch.autograd.grad(y, x, dy, create_graph=True)
    return dx, torch.autograd.grad((dx * v).sum(), [dy, x] + list(extra))


# The reduction of the layer-norm double backward gives one workgroup 4096 floats of a sample (kLnChunkFloats in csrc/t2i_ops.hip):
# a sample of 64 * 64 * 16 = 65536 floats is split over 16 workgroups and finished by the fixed-order second stage.
LN_CHUNK_FLOATS = 4096
LN_CASES = [((2, 3, 5, 3), None), ((2, 4, 4, 16), 'lrelu'), ((3, 2, 2, 64), 'relu'), ((4, 50), None), ((3, 64, 64, 16), None)]


@pytest.mark.parametrize('shape,act', LN_CASES)
def test_layer_norm_second_order(ops, shape, act):
    from t2i_amd import autograd as A
    if shape == (3, 64, 64, 16):
        assert int(np.prod(shape[1:])) > LN_CHUNK_FLOATS and -(-int(np.prod(shape[1:])) // LN_CHUNK_FLOATS) == 16      # the multi-workgroup path
    else:
        assert int(np.prod(shape[1:])) <= LN_CHUNK_FLOATS                                                             # one workgroup per sample
    g = torch.Generator().manual_seed(21)
    x = torch.randn(shape, generator=g) * 1.3 + 0.1
    C = shape[-1]
    gam, bet = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    dy, v = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xr, gr, br = x.double().requires_grad_(True), gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    dyr = dy.double().requires_grad_(True)
    yr, pre = _ln64(xr, gr, br, act)
    if act is not None:
        assert float(pre.abs().min()) >= KINK, float(pre.abs().min())
    dxr, (r_dgy, r_ddx, r_dgam) = _second_order(yr, xr, [gr], dyr, v.double())
    kind, alpha = _kind(act)
    xc, gc, bc = x.cuda().requires_grad_(True), gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True)
    dyc = dy.cuda().requires_grad_(True)
    y = A.LayerNormFn.apply(xc, gc, bc, 1e-12, kind, alpha)
    dx, (dgy, ddx, dgam) = _second_order(y, xc, [gc], dyc, v.cuda())
    e = dict(y=relerr(y, yr), dx=relerr(dx, dxr), dgy=relerr(dgy, r_dgy), ddx=relerr(ddx, r_ddx), dgamma=relerr(dgam, r_dgam))
    print('layer_norm %s %s: %s' % (shape, act, '  '.join('%s %.2e' % kv for kv in e.items())))
    assert e['y'] <= 1e-5 and e['dx'] <= 1e-4 and e['dgy'] <= 1e-4 and e['ddx'] <= 1e-4 and e['dgamma'] <= 1e-5, e


# (the double-backward kernel sizes its register arrays by the row: 1, 2, 4 or 8 units per lane, or none for a row read twice; the last
# three cases reach the sizes the first six leave out: 4 and 8 in the 16-byte form, 4 in the scalar form)
PN_CASES = [((2, 3, 5, 3), None), ((2, 4, 4, 16), 'lrelu'), ((3, 2, 2, 64), 'relu'), ((1, 2, 3, 512), None), ((5, 1, 1, 260), 'lrelu'),
            ((1, 1, 3, 2304), None), ((1, 1, 2, 1024), None), ((1, 1, 2, 2048), None), ((2, 1, 1, 130), None)]


@pytest.mark.parametrize('shape,act', PN_CASES)
def test_pixel_norm_second_order(ops, shape, act):
    g = torch.Generator().manual_seed(21)
    x = torch.randn(shape, generator=g) * 1.3 + 0.1
    if act == 'relu':
        x[1, 0, 1, :] = -x[1, 0, 1, :].abs() - 0.01              # a pixel with u = 0 everywhere
    dy, v = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xr, dyr = x.double().requires_grad_(True), dy.double().requires_grad_(True)
    yr, pre = _pn64(xr, act)
    if act is not None:
        assert float(pre.abs().min()) >= KINK, float(pre.abs().min())
    dxr, (r_dgy, r_ddx) = _second_order(yr, xr, [], dyr, v.double())
    xc, dyc = x.cuda().requires_grad_(True), dy.cuda().requires_grad_(True)
    y = ops.pixel_norm(xc, act=_fused(ops, act))
    dx, (dgy, ddx) = _second_order(y, xc, [], dyc, v.cuda())
    e = dict(y=relerr(y, yr), dx=relerr(dx, dxr), dgy=relerr(dgy, r_dgy), ddx=relerr(ddx, r_ddx))
    print('pixel_norm %s %s: %s' % (shape, act, '  '.join('%s %.2e' % kv for kv in e.items())))
    assert e['y'] <= 1e-5 and e['dx'] <= 1e-4 and e['dgy'] <= 1e-4 and e['ddx'] <= 1e-4, e
    if act == 'relu':
        for t in (dx, dgy, ddx):
            assert bool(torch.isfinite(t).all()) and bool((t[1, 0, 1] == 0).all())


def test_first_order_bits_do_not_depend_on_create_graph(ops):
    """The backward Functions run today's kernel sequence: dx of a plain backward() == dx taken with create_graph=True, bit for bit"""
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(3, 4, 4, 16, generator=g) * 1.3 + 0.1).cuda()
    dy = torch.randn(3, 4, 4, 16, generator=g).cuda()
    from t2i_amd import scope as S
    st = S.VariableStore(device='cuda')
    for name in ('layer_norm', 'pixel_norm'):
        with _store(st):
            def run(t, reuse):
                if name == 'pixel_norm':
                    return ops.pixel_norm(t, act=ops.lrelu_act(0.2))
                with st.variable_scope('n', reuse=reuse):
                    return ops.layer_norm(t, act=ops.lrelu_act(0.2), scope='LayerNorm')
            a = x.clone().requires_grad_(True)
            run(a, False).backward(dy)
            b = x.clone().requires_grad_(True)
            db, = torch.autograd.grad(run(b, True), b, dy, create_graph=True)
        assert db.requires_grad and torch.equal(a.grad, db.detach()), name


def test_input_grads_only_skips_the_parameter_gradients(ops):
    from t2i_amd import autograd as A
    from t2i_amd import kernels as K
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 4, 8, generator=g).cuda().requires_grad_(True)
    gam, bet = torch.ones(8).cuda().requires_grad_(True), torch.zeros(8).cuda().requires_grad_(True)
    y = A.LayerNormFn.apply(x, gam, bet, 1e-12, K.ACT_LRELU, 0.2)
    full = torch.autograd.grad(y.sum(), [x, gam], retain_graph=True)
    with A.input_grads_only():
        gx, gg = torch.autograd.grad(y.sum(), [x, gam], allow_unused=True)
    assert gg is None and full[1] is not None and torch.equal(gx, full[0])


def test_tanh_first_order_works_and_second_order_is_refused(ops):
    from t2i_amd import autograd as A
    from t2i_amd import kernels as K
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 3, 8, generator=g)
    dy, v = torch.randn(2, 3, 3, 8, generator=g), torch.randn(2, 3, 3, 8, generator=g)
    gam, bet = 1 + 0.3 * torch.randn(8, generator=g), 0.2 * torch.randn(8, generator=g)
    xr = x.double().requires_grad_(True)
    refs = {'layer_norm': _ln64(xr, gam.double(), bet.double(), 'tanh')[0], 'pixel_norm': _pn64(xr, 'tanh')[0]}
    for name in ('layer_norm', 'pixel_norm'):
        xc = x.cuda().requires_grad_(True)
        if name == 'layer_norm':
            y = A.LayerNormFn.apply(xc, gam.cuda().requires_grad_(True), bet.cuda().requires_grad_(True), 1e-12, K.ACT_TANH, 0.0)
        else:
            y = ops.pixel_norm(xc, act=ops.tanh)
        dx, = torch.autograd.grad(y, xc, dy.cuda(), create_graph=True)
        dxr, = torch.autograd.grad(refs[name], xr, dy.double())
        assert relerr(y, refs[name]) <= 1e-5 and relerr(dx, dxr) <= 1e-4, name
        with pytest.raises(NotImplementedError, match=name):
            torch.autograd.grad((dx * v.cuda()).sum(), xc)


# ---- a small normalised critic under the gradient penalty ----------------------------------------------------------------------------
def _conv64(x_nhwc, w_hwio, b):
    return F.conv2d(x_nhwc.permute(0, 3, 1, 2), w_hwio.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)


def _critic64(P, x):
    """-> (logits [B], the two normalisations' pre-activations)"""
    h = _conv64(x, P['d_net/Conv/weights'], P['d_net/Conv/biases'])
    h, pre_ln = _ln64(h, P['d_net/LayerNorm/gamma'], P['d_net/LayerNorm/beta'], 'lrelu')
    h = F.avg_pool2d(h.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    h = _conv64(h, P['d_net/Conv_1/weights'], P['d_net/Conv_1/biases'])
    h, pre_pn = _pn64(h, 'lrelu')
    return (h.reshape(h.shape[0], -1) @ P['d_net/dense/kernel'] + P['d_net/dense/bias']).reshape(-1), (pre_ln, pre_pn)


def _penalty64(grad):
    slopes = torch.sqrt((grad ** 2).reshape(grad.shape[0], -1).sum(1))
    return torch.mean(torch.clamp(slopes - 1.0, min=0.0) ** 2)


def test_small_critic_under_the_penalty(ops):
    """conv -> layer_norm(lrelu) -> pool -> conv -> pixel_norm(lrelu) -> fc, loss = mean(D) + 10 * penalty with the penalty formed as
    PGGAN.get_gradient_penalty forms it: every parameter gradient against the same critic in float64 torch"""
    from t2i_amd import autograd as A
    from t2i_amd import kernels as K
    from t2i_amd import scope as S
    from t2i_amd.models.pggan.pggan import PGGAN
    st = S.VariableStore(device='cuda', seed=3)

    def critic(x, reuse):
        with st.variable_scope('d_net', reuse=reuse):
            h = ops.conv2d(x, 8, ks=(3, 3), s=(1, 1), act=None)
            h = ops.layer_norm(h, act=ops.lrelu_act())
            h = ops.pool(h, 2)
            h = ops.conv2d(h, 8, ks=(3, 3), s=(1, 1), act=None)
            h = ops.pixel_norm(h, act=ops.lrelu_act())
            return ops.fc(h.reshape(h.shape[0], -1), 1).reshape(-1)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(4, 8, 8, 3, generator=g) * 1.3 + 0.1
    with _store(st):
        with K.dry_run(), torch.no_grad():
            critic(torch.empty(4, 8, 8, 3, device='cuda'), False)
        values = {}
        for n, p in st.vars.items():           # He-scaled filters, a dense layer wide enough for slopes above 1, non-trivial biases and affine
            t = torch.randn(p.shape, generator=g)
            if n.endswith('weights'):
                t = t * (2.0 / (9 * p.shape[2])) ** 0.5
            elif n.endswith('kernel'):
                t = t * 0.5
            elif n.endswith('gamma'):
                t = 1 + 0.3 * t
            else:
                t = 0.2 * t
            values[n] = t
        st.load(values)
        xc = x.cuda().requires_grad_(True)
        D = critic(xc, True)
        with A.input_grads_only():                                         # PGGAN.get_gradient_penalty
            grad_y, = torch.autograd.grad(D.sum(), [xc], create_graph=True)
        pen = PGGAN._penalty(grad_y)
        loss = D.mean() + 10.0 * pen
        loss.backward(inputs=list(st.vars.values()))
    P = {n: t.double().requires_grad_(True) for n, t in values.items()}
    xr = x.double().requires_grad_(True)
    Dr, pres = _critic64(P, xr)
    for pre in pres:
        assert float(pre.abs().min()) >= KINK, float(pre.abs().min())
    gr, = torch.autograd.grad(Dr.sum(), xr, create_graph=True)
    penr = _penalty64(gr)
    assert float(penr) > 0.05                                          # the hinge is active: the second-order path carries the gradient
    lossr = Dr.mean() + 10.0 * penr
    grads = dict(zip(P, torch.autograd.grad(lossr, list(P.values()))))
    assert relerr(D, Dr) <= 1e-5 and abs(float(pen) - float(penr)) <= 1e-4 * max(float(penr), 1.0)
    errs = {n: relerr(st.vars[n].grad, grads[n]) for n in P}
    print('small critic: penalty %.4f  %s' % (float(penr), '  '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) <= 1e-5, errs
