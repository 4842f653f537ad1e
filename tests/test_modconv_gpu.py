"""The weight-demodulated convolution's kernels (csrc/t2i_modconv.hip) on the GPU against the float64
restatements of tests/modconv_cases.py: every entry point over its case table at max(floor, 8 e32), the wrapped grid, a misaligned base,
batch independence and determinism bit for bit, the composed ops.modulated_conv2d against the float64 definition (per-sample filters, a
grouped convolution), and a captured forward + backward against eager."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import modconv_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    assert kernels.MODCONV_CHUNK_ROWS == MC.CHUNK
    return kernels


DEV = lambda a: None if a is None else torch.tensor(a, device='cuda')
NP = lambda t: t.detach().double().cpu().numpy()
ACT = lambda K, act: {None: K.ACT_NONE, 'relu': K.ACT_RELU, 'lrelu': K.ACT_LRELU}[act]


def check(got, ref, tol, what):
    worst = {}
    for k, t in got.items():
        if ref[k] is None:
            assert t is None, k
            continue
        worst[k] = MC.relerr(NP(t), ref[k])
    print('%s: %s' % (what, ', '.join('%s %.2e/%.2e' % (k, e, tol[k]) for k, e in worst.items())))
    for k, e in worst.items():
        assert e <= tol[k], (what, k, e, tol[k])


# ---- the demodulation coefficients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(MC.COEF_CASES)), ids=lambda i: 'T%d-%dx%d-B%d' % MC.COEF_CASES[i])
def test_demod_coef_and_its_backward(K, i):
    T, ci, co, B = MC.COEF_CASES[i]
    (W, s, gd), ref, tol = MC.coef_reference(i)
    kh = 3 if T == 9 else 1
    Wd, sd, gdd = DEV(W.reshape(kh, kh, ci, co)), DEV(s), DEV(gd)
    d, q = K.demod_coef(Wd, sd, MC.EPS)
    ds, dW = K.demod_coef_bwd(gdd, d, Wd, sd, q)
    check(dict(q=q, d=d, ds=ds, dW=dW.reshape(T, ci, co)), ref, tol, 'demod_coef %s' % (MC.COEF_CASES[i],))
    # s as a slice of a wider tensor (a row stride above Cin) gives the same bits
    wide = torch.zeros(B, ci + 5, device='cuda')
    wide[:, 2:2 + ci] = sd
    d2, q2 = K.demod_coef(Wd, wide[:, 2:2 + ci], MC.EPS)
    ds2, dW2 = K.demod_coef_bwd(gdd, d2, Wd, wide[:, 2:2 + ci], q2)
    assert torch.equal(d, d2) and torch.equal(q, q2) and torch.equal(ds, ds2) and torch.equal(dW, dW2)
    # only one of the two gradients, and dW added into a buffer
    assert K.demod_coef_bwd(gdd, d, Wd, sd, q, want_w=False)[1] is None and K.demod_coef_bwd(gdd, d, Wd, sd, q, want_s=False)[0] is None
    slot = torch.full((Wd.numel(),), 0.5, device='cuda')
    K.demod_coef_bwd(gdd, d, Wd, sd, q, want_s=False, out=slot, accumulate=True)
    assert torch.equal(slot, 0.5 + dW.reshape(-1))
    K.demod_coef_bwd(gdd, d, Wd, sd, q, want_s=False, out=slot, accumulate=False)
    assert torch.equal(slot, dW.reshape(-1))


def test_an_all_zero_style_row_gives_a_finite_coefficient_and_the_bias(K):
    from t2i_amd import autograd as A
    W, s, _ = MC.coef_inputs((9, 20, 12, 3), zero_row=True)
    Wd, sd = DEV(W.reshape(3, 3, 20, 12)), DEV(s)
    d, _ = K.demod_coef(Wd, sd, MC.EPS)
    assert bool(torch.isfinite(d).all()) and float((d[2] - 1e4).abs().max()) <= 1e4 * 1e-6           # rsqrt(eps)
    x = torch.randn(3, 5, 7, 20, device='cuda')
    bias = torch.randn(12, device='cuda')
    geom = K.conv_desc(3, 5, 7, 20, 12, 3, 3, 1, 1, 'SAME')
    c = A.Conv2dFn.apply(K.modulate(x, sd), Wd, None, geom, K.ACT_NONE, 0.0)
    out = K.demod_act(c, d, bias)
    assert torch.equal(out[2], bias.expand(5, 7, 12))      # the layer's output under a zero style is the bias, exactly


# ---- the scale pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(MC.SCALE_CASES)), ids=lambda i: '%dx%dx%dx%d' % MC.SCALE_CASES[i])
def test_modulate_its_adjoint_and_the_scale_gradient(K, i):
    (x, s, g), ref, tol = MC.scale_reference(i)
    xd, sd, gd = DEV(x), DEV(s), DEV(g)
    got = dict(xs=K.modulate(xd, sd), dx=K.modulate(gd, sd), ds=K.modulate_bwd_scale(gd, xd))
    check(got, ref, tol, 'modulate %s' % (MC.SCALE_CASES[i],))
    # a base that is not 16-byte aligned takes the scalar body: the same values bit for bit (a product has one rounding; the sums keep
    # their order only between equal bodies, so ds is held to the tolerance)
    B, H, W, C = x.shape
    off = lambda t: torch.cat([torch.zeros(1, device='cuda'), t.reshape(-1)])[1:].view(t.shape)
    xo, go = off(xd), off(gd)
    assert xo.data_ptr() % 16 == 4
    assert torch.equal(K.modulate(xo, sd), got['xs']) and torch.equal(K.modulate(go, sd), got['dx'])
    assert MC.relerr(NP(K.modulate_bwd_scale(go, xo)), ref['ds']) <= tol['ds']


def test_the_wrapped_grid(K):
    """70 000 samples of 1 x 2 x 1: more items than the 65 535 workgroups of a launch."""
    B = 70000
    rng = np.random.default_rng(5)
    x, s, g = (rng.standard_normal(sh).astype(np.float32) for sh in ((B, 1, 2, 1), (B, 1), (B, 1, 2, 1)))
    ref, tol = MC.scale(x, s, g, np.float64), MC.tolerances(MC.scale(x, s, g, np.float64), MC.scale(x, s, g, np.float32))
    xd, sd, gd = DEV(x), DEV(s), DEV(g)
    assert np.array_equal(NP(K.modulate(xd, sd)), (x * s[:, None, None, :]).astype(np.float64))
    assert MC.relerr(NP(K.modulate_bwd_scale(gd, xd)), ref['ds']) <= tol['ds']
    d = rng.uniform(0.5, 2.0, (B, 1)).astype(np.float32)
    bias, st, nz = np.float32([0.3]), np.float32([0.4]), rng.standard_normal((B, 1, 2)).astype(np.float32)
    r = MC.epilogue(x, d, bias, nz, st, g, None, np.float64)
    tol = MC.tolerances(r, MC.epilogue(x, d, bias, nz, st, g, None, np.float32))
    out = K.demod_act(xd, DEV(d), DEV(bias), DEV(nz), DEV(st))
    dc, dd, dbias, dstrength = K.demod_act_bwd(gd, xd, DEV(d), DEV(bias), DEV(nz), DEV(st))
    check(dict(out=out, dc=dc, dd=dd, dbias=dbias, dstrength=dstrength), r, tol, 'wrapped grid')


# ---- the epilogue -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(MC.EPI_CASES)), ids=lambda i: MC.epi_id(MC.EPI_CASES[i]))
def test_demod_act_and_its_backward(K, i):
    case = MC.EPI_CASES[i]
    (c, d, bias, noise, strength, g), ref, tol = MC.epi_reference(i)
    act = ACT(K, case[4])
    args = [DEV(a) for a in (c, d, bias, noise, strength)]
    out = K.demod_act(*args, act=act, alpha=MC.ALPHA)
    dc, dd, dbias, dstrength = K.demod_act_bwd(DEV(g), *args, act=act, alpha=MC.ALPHA)
    check(dict(out=out, dc=dc, dd=dd, dbias=dbias, dstrength=dstrength), ref, tol, 'demod_act ' + MC.epi_id(case))
    # unwanted sums are not formed, and dc does not depend on which are
    only = K.demod_act_bwd(DEV(g), *args, act=act, alpha=MC.ALPHA, want_d=False, want_bias=False, want_strength=False)
    assert only[1:] == (None, None, None) and torch.equal(only[0], dc)
    if noise is None:
        # a constant-zero strength is the call without noise, bit for bit
        nz = torch.randn(c.shape[:3], device='cuda')
        zero = torch.zeros(c.shape[3], device='cuda')
        assert torch.equal(K.demod_act(args[0], args[1], args[2], nz, zero, act=act, alpha=MC.ALPHA), out)
        assert torch.equal(K.demod_act_bwd(DEV(g), args[0], args[1], args[2], nz, zero, act=act, alpha=MC.ALPHA)[0], dc)


# ---- batch independence and determinism -------------------------------------------------------------------------------------------------
def test_a_sample_alone_equals_its_row_of_a_batch_and_runs_repeat(K):
    rng = np.random.default_rng(9)
    f = lambda *sh: torch.tensor(rng.standard_normal(sh).astype(np.float32), device='cuda')
    B, H, W, Cin, Cout = 3, 5, 27, 68, 20                  # 135 rows: three chunks, the last one partial; two channel tiles
    x, g, s, Wt, gd = f(B, H, W, Cin), f(B, H, W, Cin), 1.0 + 0.5 * f(B, Cin), f(3, 3, Cin, Cout) * 0.05, f(B, Cout)
    c, gc, bias, nz, st = f(B, H, W, Cout), f(B, H, W, Cout), f(Cout), f(B, H, W), f(Cout)

    def run(b):
        sl = slice(None) if b is None else slice(b, b + 1)
        d, q = K.demod_coef(Wt, s[sl], MC.EPS)
        ds, _ = K.demod_coef_bwd(gd[sl].contiguous(), d, Wt, s[sl], q, want_w=False)
        res = [d, ds, K.modulate(x[sl].contiguous(), s[sl]), K.modulate_bwd_scale(g[sl].contiguous(), x[sl].contiguous()),
               K.demod_act(c[sl].contiguous(), d, bias, nz[sl].contiguous(), st, act=K.ACT_LRELU, alpha=0.2)]
        dc, dd, _, _ = K.demod_act_bwd(gc[sl].contiguous(), c[sl].contiguous(), d, bias, nz[sl].contiguous(), st, act=K.ACT_LRELU, alpha=0.2)
        return res + [dc, dd]
    whole, again = run(None), run(None)
    for a, b in zip(whole, again):
        assert torch.equal(a, b)                           # two runs are identical
    for b in range(B):
        for a, alone in zip(whole, run(b)):
            assert torch.equal(a[b:b + 1], alone)          # a sample alone is its row of the batch
    full = K.demod_act_bwd(gc, c, whole[0], bias, nz, st, act=K.ACT_LRELU, alpha=0.2)
    for a, b in zip(full, K.demod_act_bwd(gc, c, whole[0], bias, nz, st, act=K.ACT_LRELU, alpha=0.2)):
        assert torch.equal(a, b)                           # ... dbias and dstrength included
    assert torch.equal(K.demod_coef_bwd(gd, whole[0], Wt, s, K.demod_coef(Wt, s)[1])[1], K.demod_coef_bwd(gd, whole[0], Wt, s, K.demod_coef(Wt, s)[1])[1])


# ---- the composed operator --------------------------------------------------------------------------------------------------------------
def _layer(K, inp, act, demodulate=True, noise=True, store=None):
    """ops.modulated_conv2d on the case's variables -> (out, x, w, the store)."""
    from t2i_amd import scope as S
    from t2i_amd.utils import ops
    st = S.set_default_store(store or S.VariableStore(device='cuda', seed=0))
    x, w = DEV(inp['x']).requires_grad_(True), DEV(inp['w']).requires_grad_(True)
    a = {None: None, 'relu': ops.relu, 'lrelu': ops.lrelu_act(MC.ALPHA)}[act]
    with S.variable_scope('t', reuse=store is not None):
        if store is None:
            with K.dry_run(), torch.no_grad():
                ops.modulated_conv2d(x, w, inp['weights'].shape[3], noise=DEV(inp['noise']) if noise else None, name='ModConv')
            st.load({'t/ModConv/weights': inp['weights'], 't/ModConv/biases': inp['biases'], 't/ModConv/style/kernel': inp['kernel'],
                     't/ModConv/style/bias': inp['bias'], **({'t/ModConv/noise_strength': inp['noise_strength']} if noise else {})})
    with S.variable_scope('t', reuse=True):
        out = ops.modulated_conv2d(x, w, inp['weights'].shape[3], noise=DEV(inp['noise']) if noise else None, act=a, demodulate=demodulate,
                                   name='ModConv')
    return out, x, w, st


@pytest.mark.parametrize('case', MC.LAYER_CASES, ids=str)
def test_modulated_conv2d_against_the_float64_definition(K, case):
    inp, ref, grads = MC.layer_reference(case)
    out, x, w, st = _layer(K, inp, None)
    fwd = MC.relerr(NP(out), ref)
    names = ('weights', 'biases', 'noise_strength', 'style/kernel', 'style/bias')
    leaves = [st.vars['t/ModConv/' + n] for n in names]
    got = torch.autograd.grad((out * DEV(inp['g'])).sum(), [x, w] + leaves)
    errs = {k: MC.relerr(NP(t), grads[k]) for k, t in zip(('x', 'w', 'weights', 'biases', 'noise_strength', 'kernel', 'bias'), got)}
    _, ref_relu, _ = MC.layer_reference(case, 'relu', with_grads=False)
    relu = MC.relerr(NP(_layer(K, inp, 'relu', store=st)[0]), ref_relu)
    print('modulated_conv2d %s: out %.2e, relu %.2e, %s' % (case, fwd, relu, ', '.join('d%s %.2e' % kv for kv in errs.items())))
    assert fwd <= 1e-4 and relu <= 1e-4
    for k, e in errs.items():
        assert e <= 1e-4, (k, e)                           # (weights: the total of the convolution's and the coefficients' paths)
    with pytest.raises(NotImplementedError, match='second differentiation'):
        out2, x2, _, _ = _layer(K, inp, None, store=st)
        gx, = torch.autograd.grad(out2.sum(), [x2], create_graph=True)
        gx.sum().backward()


def test_without_demodulation_and_with_unit_scales_it_is_conv2d(K):
    from t2i_amd import scope as S
    from t2i_amd.utils import ops
    inp = dict(MC.layer_inputs((3, 5, 7, 20, 12)))
    inp['kernel'], inp['bias'] = np.zeros_like(inp['kernel']), np.zeros_like(inp['bias'])          # s == 1
    out, x, _, st = _layer(K, inp, None, demodulate=False, noise=False)
    plain = S.set_default_store(S.VariableStore(device='cuda', seed=0))
    with S.variable_scope('t'):
        with K.dry_run(), torch.no_grad():
            ops.conv2d(x, 12, ks=(3, 3), s=(1, 1), name='Conv')
        plain.load({'t/Conv/weights': inp['weights'], 't/Conv/biases': inp['biases']})
    with S.variable_scope('t', reuse=True), torch.no_grad():
        want = ops.conv2d(x, 12, ks=(3, 3), s=(1, 1), name='Conv')
    assert MC.relerr(NP(out), NP(want)) <= 1e-6


def test_a_captured_forward_and_backward_replays_like_eager(K):
    """One graph, replayed with re-drawn noise and a new w in the static buffers, equals the eager run on the same values."""
    case = (2, 8, 8, 64, 68)
    inp = MC.layer_inputs(case)
    _, _, _, st = _layer(K, inp, 'relu')
    names = ('weights', 'biases', 'noise_strength', 'style/kernel', 'style/bias')
    leaves = [st.vars['t/ModConv/' + n] for n in names]
    from t2i_amd import scope as S
    from t2i_amd.utils import ops
    xs, ws, nzs, gs = DEV(inp['x']).requires_grad_(True), DEV(inp['w']).requires_grad_(True), DEV(inp['noise']), DEV(inp['g'])

    def step():
        with S.variable_scope('t', reuse=True):
            out = ops.modulated_conv2d(xs, ws, 68, noise=nzs, act=ops.relu, name='ModConv')
        return [out] + list(torch.autograd.grad((out * gs).sum(), [xs, ws] + leaves))
    step()                                                 # the kernels are loaded and the workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    rng = np.random.default_rng(3)
    for _ in range(2):
        with torch.no_grad():
            nzs.copy_(DEV(rng.standard_normal(nzs.shape).astype(np.float32)))
            ws.copy_(DEV(rng.standard_normal(ws.shape).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in static]
        for a, b in zip(replayed, step()):
            assert torch.equal(a, b)
