"""The weight-demodulated convolution's second-order kernels (csrc/t2i_modconv.hip) on the GPU against the float64
restatements of tests/modconv2_cases.py: every entry point over the first-order case tables at max(floor, 8 e32), the wrapped grid, a
misaligned base, each cotangent alone, batch independence and determinism bit for bit, ops.modulated_conv2d(second_order=True) against
second_order=False (bit for bit at first order) and against the float64 definition's path-length gradient, and a captured forward + first
+ second backward against eager."""
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
import modconv2_cases as M2  # noqa: E402

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
SAME = lambda a, b: (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def off(t):
    """The same values at a base that is 4 bytes past a 16-byte boundary: the scalar form."""
    o = torch.cat([torch.zeros(1, device='cuda'), t.reshape(-1)])[1:].view(t.shape)
    assert o.data_ptr() % 16 == 4
    return o


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


# ---- the epilogue -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(M2.EPI_CASES)), ids=lambda i: MC.epi_id(M2.EPI_CASES[i]))
def test_demod_act_bwd2(K, i):
    case = M2.EPI_CASES[i]
    (c, d, bias, noise, strength, g), (vc, vd), ref, tol = M2.epi_reference(i)
    act = ACT(K, case[4])
    args = [DEV(a) for a in (g, c, d, bias, noise, strength)]
    vcd, vdd = DEV(vc), DEV(vd)
    gg, gc, gd = K.demod_act_bwd2(*args, vcd, vdd, act=act, alpha=MC.ALPHA)
    check(dict(gg=gg, gc=gc, gd=gd), ref, tol, 'demod_act_bwd2 ' + MC.epi_id(case))
    # vc alone: gc is not formed, gd keeps its bits; vd alone: gd is not formed, gc keeps its bits; gg is the restatement's for that cotangent
    alone = lambda a, b, dt: M2.epilogue2(c, d, bias, noise, strength, g, a, b, case[4], dt)
    a_gg, a_gc, a_gd = K.demod_act_bwd2(*args, vcd, None, act=act, alpha=MC.ALPHA)
    r = alone(vc, None, np.float64)
    assert a_gc is None and SAME(a_gd, gd) and MC.relerr(NP(a_gg), r['gg']) <= M2.tolerances(r, alone(vc, None, np.float32))['gg']
    if vd is not None:
        b_gg, b_gc, b_gd = K.demod_act_bwd2(*args, None, vdd, act=act, alpha=MC.ALPHA)
        r = alone(None, vd, np.float64)
        assert b_gd is None and torch.equal(b_gc, gc) and MC.relerr(NP(b_gg), r['gg']) <= M2.tolerances(r, alone(None, vd, np.float32))['gg']
    # an unwanted output is None and the others keep their bits
    only = K.demod_act_bwd2(*args, vcd, vdd, act=act, alpha=MC.ALPHA, want_c=False, want_d=False)
    assert only[1] is None and only[2] is None and torch.equal(only[0], gg)
    nog = K.demod_act_bwd2(*args, vcd, vdd, act=act, alpha=MC.ALPHA, want_g=False)
    assert nog[0] is None and SAME(nog[1], gc) and SAME(nog[2], gd)
    # the scalar form on a misaligned base: the planes bit for bit (products and one fmaf per element), the sum to its tolerance
    o = K.demod_act_bwd2(off(args[0]), off(args[1]), *args[2:], off(vcd), vdd, act=act, alpha=MC.ALPHA)
    assert torch.equal(o[0], gg) and SAME(o[1], gc)
    if gd is not None:
        assert MC.relerr(NP(o[2]), ref['gd']) <= tol['gd']


# ---- the scale pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(M2.SCALE_CASES)), ids=lambda i: '%dx%dx%dx%d' % M2.SCALE_CASES[i])
def test_modulate2_and_the_two_reused_launches(K, i):
    (x, s, g), (vx, vs), ref, tol = M2.scale_reference(i)
    xd, sd, gd, vxd, vsd = (DEV(a) for a in (x, s, g, vx, vs))
    gg = K.modulate2(sd, vxd, xd, vsd)
    check(dict(gg=gg, gx=K.modulate(gd, vsd), gs=K.modulate_bwd_scale(vxd, gd)), ref, tol, 'modulate2 %s' % (M2.SCALE_CASES[i],))
    # each cotangent alone is the product it stands for, bit for bit
    assert torch.equal(K.modulate2(sd, vxd, None, None), K.modulate(vxd, sd)) and torch.equal(K.modulate2(None, None, xd, vsd), K.modulate(xd, vsd))
    # s as a slice of a wider tensor, and the scalar form on a misaligned base
    wide = torch.zeros(x.shape[0], x.shape[3] + 5, device='cuda')
    wide[:, 2:2 + x.shape[3]] = sd
    assert torch.equal(K.modulate2(wide[:, 2:2 + x.shape[3]], vxd, xd, vsd), gg)
    assert torch.equal(K.modulate2(sd, off(vxd), off(xd), vsd), gg)


def test_the_wrapped_grid(K):
    """70 000 samples of 1 x 2 x 1: more items than the 65 535 workgroups of a launch."""
    B = 70000
    rng = np.random.default_rng(5)
    x, g, vx = (rng.standard_normal((B, 1, 2, 1)).astype(np.float32) for _ in range(3))
    s, vs = (rng.standard_normal((B, 1)).astype(np.float32) for _ in range(2))
    r = M2.scale2(x, s, g, vx, vs, np.float64)
    tol = M2.tolerances(r, M2.scale2(x, s, g, vx, vs, np.float32))
    check(dict(gg=K.modulate2(DEV(s), DEV(vx), DEV(x), DEV(vs))), dict(gg=r['gg']), tol, 'wrapped modulate2')
    d = rng.uniform(0.5, 2.0, (B, 1)).astype(np.float32)
    bias, st, nz = np.float32([0.3]), np.float32([0.4]), rng.standard_normal((B, 1, 2)).astype(np.float32)
    r = M2.epilogue2(x, d, bias, nz, st, g, vx, vs, 'lrelu', np.float64)
    tol = M2.tolerances(r, M2.epilogue2(x, d, bias, nz, st, g, vx, vs, 'lrelu', np.float32))
    gg, gc, gd = K.demod_act_bwd2(DEV(g), DEV(x), DEV(d), DEV(bias), DEV(nz), DEV(st), DEV(vx), DEV(vs), act=K.ACT_LRELU, alpha=MC.ALPHA)
    check(dict(gg=gg, gc=gc, gd=gd), r, tol, 'wrapped demod_act_bwd2')


# ---- the coefficients -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(M2.COEF_CASES)), ids=lambda i: 'T%d-%dx%d-B%d' % M2.COEF_CASES[i])
def test_demod_coef_bwd2(K, i):
    T, ci, co, B = M2.COEF_CASES[i]
    (W, s, gd), vs, ref, tol = M2.coef_reference(i)
    kh = 3 if T == 9 else 1
    Wd, sd, gdd, vsd = DEV(W.reshape(kh, kh, ci, co)), DEV(s), DEV(gd), DEV(vs)
    d, q = K.demod_coef(Wd, sd, MC.EPS)
    ggd, gd_d, gW = K.demod_coef_bwd2(vsd, gdd, d, Wd, sd, q)
    gs = K.demod_coef_bwd(gdd, d, Wd, vsd, q, True, False)[0]                             # the term to s: the first-order launch, vs for s
    check(dict(ggd=ggd, gdd=gd_d, gs=gs, gW=gW.reshape(T, ci, co)), ref, tol, 'demod_coef_bwd2 %s' % (M2.COEF_CASES[i],))
    wide = torch.zeros(B, ci + 5, device='cuda')
    wide[:, 2:2 + ci] = sd
    for a, b in zip(K.demod_coef_bwd2(vsd, gdd, d, Wd, wide[:, 2:2 + ci], q), (ggd, gd_d, gW)):
        assert torch.equal(a, b)
    one = K.demod_coef_bwd2(vsd, gdd, d, Wd, sd, q, want_d=False, want_w=False)
    assert one[1] is None and one[2] is None and torch.equal(one[0], ggd)
    one = K.demod_coef_bwd2(vsd, gdd, d, Wd, sd, q, want_gd=False, want_w=False)
    assert one[0] is None and torch.equal(one[1], gd_d)
    slot = torch.full((Wd.numel(),), 0.5, device='cuda')
    assert K.demod_coef_bwd2(vsd, gdd, d, Wd, sd, q, False, False, True, out=slot, accumulate=True)[:2] == (None, None)
    assert torch.equal(slot, 0.5 + gW.reshape(-1))
    K.demod_coef_bwd2(vsd, gdd, d, Wd, sd, q, False, False, True, out=slot, accumulate=False)
    assert torch.equal(slot, gW.reshape(-1))


# ---- batch independence and determinism -------------------------------------------------------------------------------------------------
def test_a_sample_alone_equals_its_row_of_a_batch_and_runs_repeat(K):
    rng = np.random.default_rng(9)
    f = lambda *sh: torch.tensor(rng.standard_normal(sh).astype(np.float32), device='cuda')
    B, H, W, Cin, Cout = 3, 5, 27, 68, 20                  # 135 rows: three chunks, the last one partial; two channel tiles
    x, vx, s, vs, Wt, gd = f(B, H, W, Cin), f(B, H, W, Cin), 1.0 + 0.5 * f(B, Cin), f(B, Cin), f(3, 3, Cin, Cout) * 0.05, f(B, Cout)
    c, g, vc, vd, bias, nz, st = f(B, H, W, Cout), f(B, H, W, Cout), f(B, H, W, Cout), f(B, Cout), f(Cout), f(B, H, W), f(Cout)

    def run(b):
        sl = slice(None) if b is None else slice(b, b + 1)
        k = lambda t: t[sl].contiguous()
        d, q = K.demod_coef(Wt, s[sl], MC.EPS)
        res = list(K.demod_coef_bwd2(k(vs), k(gd), d, Wt, s[sl], q, want_w=False)[:2]) + [K.modulate2(s[sl], k(vx), k(x), k(vs))]
        return res + list(K.demod_act_bwd2(k(g), k(c), d, bias, k(nz), st, k(vc), k(vd), act=K.ACT_LRELU, alpha=0.2))
    whole, again = run(None), run(None)
    for a, b in zip(whole, again):
        assert torch.equal(a, b)                           # two runs are identical
    for b in range(B):
        for a, alone in zip(whole, run(b)):
            assert torch.equal(a[b:b + 1], alone)          # a sample alone is its row of the batch
    d, q = K.demod_coef(Wt, s, MC.EPS)
    assert torch.equal(K.demod_coef_bwd2(vs, gd, d, Wt, s, q)[2], K.demod_coef_bwd2(vs, gd, d, Wt, s, q)[2])


# ---- the composed operator --------------------------------------------------------------------------------------------------------------
NAMES = ('weights', 'biases', 'noise_strength', 'style/kernel', 'style/bias')


def _store(K, inp):
    from t2i_amd import scope as S
    from t2i_amd.utils import ops
    st = S.set_default_store(S.VariableStore(device='cuda', seed=0))
    with S.variable_scope('t'), K.dry_run(), torch.no_grad():
        ops.modulated_conv2d(DEV(inp['x']), DEV(inp['w']), inp['weights'].shape[3], noise=DEV(inp['noise']), name='ModConv', second_order=True)
    st.load({'t/ModConv/weights': inp['weights'], 't/ModConv/biases': inp['biases'], 't/ModConv/style/kernel': inp['kernel'],
             't/ModConv/style/bias': inp['bias'], 't/ModConv/noise_strength': inp['noise_strength']})
    return st


def _layer(inp, x, w, act, second):
    from t2i_amd import scope as S
    from t2i_amd.utils import ops
    a = {None: None, 'relu': ops.relu, 'lrelu': ops.lrelu_act(MC.ALPHA)}[act]
    with S.variable_scope('t', reuse=True):
        return ops.modulated_conv2d(x, w, inp['weights'].shape[3], noise=DEV(inp['noise']), act=a, name='ModConv', second_order=second)


def _path_length(A, inp, x, w, leaves, act, g):
    out = _layer(inp, x, w, act, True)
    with A.input_grads_only():
        J, = torch.autograd.grad((out * g).sum(), [w], create_graph=True)
    return J, torch.autograd.grad((J * J).sum(), [x, w] + leaves, allow_unused=True)


@pytest.mark.parametrize('case', MC.LAYER_CASES, ids=str)
def test_second_order_is_first_order_bit_for_bit_and_the_path_length_gradient_is_the_definitions(K, case):
    from t2i_amd import autograd as A
    inp, Jref, ref = M2.layer_path_length(case)
    st = _store(K, inp)
    leaves = [st.vars['t/ModConv/' + n] for n in NAMES]
    x, w, g = DEV(inp['x']).requires_grad_(True), DEV(inp['w']).requires_grad_(True), DEV(inp['g'])
    for act in MC.ACTS:                                    # the forward and every first-order gradient: the same bits
        first = []
        for second in (False, True):
            out = _layer(inp, x, w, act, second)
            first.append([out] + list(torch.autograd.grad((out * g).sum(), [x, w] + leaves)))
        for a, b in zip(*first):
            assert torch.equal(a, b), act
    J, got = _path_length(A, inp, x, w, leaves, None, g)
    errs = {'J': MC.relerr(NP(J), Jref)}
    for k, t in zip(M2.LAYER_NAMES, got):
        if np.abs(ref[k]).max() == 0.0:                    # biases and noise_strength: sum(J^2) does not depend on them
            assert t is None or float(t.abs().max()) == 0.0, k
        else:
            errs[k] = MC.relerr(NP(t), ref[k])             # (weights: the total of the convolution's and the coefficients' paths)
    print('path length %s: %s' % (case, ', '.join('%s %.2e' % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e <= 1e-4, (k, e)
    # relu and lrelu run the same path (act' from the recomputed pre-activation); two runs agree bit for bit
    for act in ('relu', 'lrelu'):
        a, b = _path_length(A, inp, x, w, leaves, act, g), _path_length(A, inp, x, w, leaves, act, g)
        assert torch.equal(a[0], b[0]) and all(SAME(p, q) for p, q in zip(a[1], b[1]))
    with pytest.raises(NotImplementedError, match='third differentiation'):
        out = _layer(inp, x, w, None, True)
        J, = torch.autograd.grad((out * g).sum(), [w], create_graph=True)
        gx, = torch.autograd.grad((J * J).sum(), [x], create_graph=True)
        gx.sum().backward()
    with pytest.raises(NotImplementedError, match='gradient of a parameter gradient'):
        out = _layer(inp, x, w, 'relu', True)
        gb, = torch.autograd.grad((out * g).sum(), [leaves[1]], create_graph=True)
        (gb * gb).sum().backward()


def test_the_weight_terms_go_through_the_arena_sink(K):
    """In the final backward the filter's three contributions (convolution, coefficients, second-order coefficient term) land in its
    registered slot, first-touch store then adds, and autograd gets None for it: the slot equals the gradient formed without a sink."""
    from t2i_amd import autograd as A
    case = (3, 5, 7, 20, 12)
    inp = MC.layer_inputs(case)
    st = _store(K, inp)
    leaves = [st.vars['t/ModConv/' + n] for n in NAMES]
    x, w, g = DEV(inp['x']).requires_grad_(True), DEV(inp['w']).requires_grad_(True), DEV(inp['g'])
    _, plain = _path_length(A, inp, x, w, leaves, 'relu', g)
    W = leaves[0]
    slot = torch.full((W.numel(),), 7.0, device='cuda')    # stale contents: the first contribution is a plain store
    touched = [False]

    def first_touch():
        was, touched[0] = touched[0], True
        return not was
    A.register_sink(W, slot, first_touch)
    try:
        out = _layer(inp, x, w, 'relu', True)
        with A.input_grads_only():
            J, = torch.autograd.grad((out * g).sum(), [w], create_graph=True)
        (J * J).sum().backward(inputs=[x, w] + leaves)
        A.side_join()
        torch.cuda.synchronize()
    finally:
        A.SINKS.pop(W.data_ptr(), None)
    assert W.grad is None and touched[0]
    ref = NP(plain[2]).reshape(-1)
    assert MC.relerr(NP(slot), ref) <= 1e-5                # (the same terms in another order of addition)
    for t, p in zip([x, w] + leaves[1:], [plain[0], plain[1]] + list(plain[3:])):
        assert SAME(t.grad, p)
        t.grad = None


def test_a_captured_forward_and_both_backwards_replay_like_eager(K):
    """One graph, replayed with re-drawn noise and a new w in the static buffers, equals the eager run on the same values."""
    from t2i_amd import autograd as A
    from t2i_amd import scope as S
    from t2i_amd.utils import ops
    case = (2, 8, 8, 64, 68)
    inp = MC.layer_inputs(case)
    st = _store(K, inp)
    leaves = [st.vars['t/ModConv/' + n] for n in NAMES]
    xs, ws, nzs, gs = DEV(inp['x']).requires_grad_(True), DEV(inp['w']).requires_grad_(True), DEV(inp['noise']), DEV(inp['g'])

    def step():
        with S.variable_scope('t', reuse=True):
            out = ops.modulated_conv2d(xs, ws, 68, noise=nzs, act=ops.relu, name='ModConv', second_order=True)
        with A.input_grads_only():
            J, = torch.autograd.grad((out * gs).sum(), [ws], create_graph=True)
        got = torch.autograd.grad((J * J).sum(), [xs, ws] + leaves, allow_unused=True)
        return [out.detach(), J.detach()] + [t for t in got if t is not None]
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
        eager = step()
        assert len(replayed) == len(eager) == 7
        for a, b in zip(replayed, eager):
            assert torch.equal(a, b)
