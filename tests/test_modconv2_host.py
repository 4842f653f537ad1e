"""Host-side checks of the weight-demodulated convolution's second order, no GPU: the float64 restatements of
tests/modconv2_cases.py against torch's double backward, the composed layer's path-length gradient by the factorised form against the
definition, every refusal of the three new C entries (all before any launch), the keyword on a dry run, and the two refusals of the
new autograd functions."""
import ctypes
import os
import re
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


@pytest.fixture(scope='module')
def t2i():
    lib = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd
    return t2i_amd


T64 = lambda a, grad=True: None if a is None else torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def close(got, ref, what, tol=1e-12):
    got = np.zeros_like(ref) if got is None else got.detach().numpy()
    assert np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()), what


# ---- the restatements against autograd's double backward, float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize('i,which', [(i, w) for i, c in enumerate(MC.EPI_CASES) if c[:4] in ((3, 7, 9, 68), (1, 3, 43, 3))
                                     for w in (('both', 'vc', 'vd') if c[6] else ('vc',))],
                         ids=lambda v: v if isinstance(v, str) else MC.epi_id(MC.EPI_CASES[v]))
def test_the_epilogue_restatement_agrees_with_the_double_backward(i, which):
    case = MC.EPI_CASES[i]
    c, d, bias, noise, strength, g = MC.epi_inputs(case)
    vc, vd = M2.epi_cotangents(case)                                                         # (vd is None without d)
    if which == 'vc':
        vd = None
    if which == 'vd':
        vc = None
    r =M2.epilogue2(c, d, bias, noise, strength, g, vc, vd, case[4], np.float64)
    ct, dt, bt, stt, gt = T64(c), T64(d), T64(bias), T64(strength), T64(g)
    p = ct if dt is None else ct * dt[:, None, None, :]
    if bt is not None:
        p = p + bt
    if noise is not None:
        p = p + stt * T64(noise, False)[..., None]
    first = torch.autograd.grad(MC._t_act(p, case[4]), [ct] + ([dt] if dt is not None else []), gt, create_graph=True)
    total = 0.0
    if vc is not None:
        total = total + (first[0] * T64(vc, False)).sum()
    if vd is not None:
        total = total + (first[1] * T64(vd, False)).sum()
    leaves = [gt, ct] + ([dt] if dt is not None else []) + [t for t in (bt, stt) if t is not None]
    got = torch.autograd.grad(total, leaves, allow_unused=True)
    close(got[0], r['gg'], 'gg')
    close(got[1], r['gc'] if r['gc'] is not None else np.zeros_like(c, np.float64), 'gc')
    if dt is not None:
        close(got[2], r['gd'] if r['gd'] is not None else np.zeros_like(d, np.float64), 'gd')
    for extra in got[3 if dt is not None else 2:]:                                          # bias and strength get nothing
        assert extra is None or float(extra.abs().max()) == 0.0


def test_the_scale_restatement_agrees_with_the_double_backward():
    case = (3, 5, 7, 4)
    x, s, g = MC.scale_inputs(case)
    vx, vs = M2.scale_cotangents(case)
    for vx_, vs_ in ((vx, vs), (vx, None), (None, vs)):
        r = M2.scale2(x, s, g, vx_, vs_, np.float64)
        xt, st, gt = T64(x), T64(s), T64(g)
        dx, ds = torch.autograd.grad(xt * st[:, None, None, :], [xt, st], gt, create_graph=True)
        total = (0.0 if vx_ is None else (dx * T64(vx_, False)).sum()) + (0.0 if vs_ is None else (ds * T64(vs_, False)).sum())
        got = torch.autograd.grad(total, [gt, xt, st], allow_unused=True)
        for t, k in zip(got, ('gg', 'gx', 'gs')):
            close(t, r[k] if r[k] is not None else np.zeros(t.shape if t is not None else 1), k)


@pytest.mark.parametrize('case', [(1, 3, 4, 3), (9, 20, 12, 2), (9, 4, 3, 1)], ids=str)
def test_the_coefficient_restatement_agrees_with_the_double_backward(case):
    """ds depends on d, which is handed its cotangent: the totals to s and W are the direct terms plus the first-order backward of d."""
    W, s, gd = MC.coef_inputs(case)
    vs = M2.coef_cotangent(case)
    r = M2.coef2(W, s, gd, vs, np.float64)
    again = MC.coef(W, s, r['gdd'], np.float64)                                              # the first-order backward, once more
    Wt, st, gdt = T64(W), T64(s), T64(gd)
    d = torch.rsqrt(((Wt[None] * st[:, None, :, None]) ** 2).sum((1, 2)) + MC.EPS)
    ds, = torch.autograd.grad(d, [st], gdt, create_graph=True)
    ggd, gs, gW = torch.autograd.grad((ds * T64(vs, False)).sum(), [gdt, st, Wt])
    close(ggd, r['ggd'], 'ggd')
    close(gs, r['gs'] + again['ds'], 'gs')
    close(gW, r['gW'] + again['dW'], 'gW')
    # ... and with d a leaf (what the kernel's formulas state term by term)
    q = (Wt * Wt).sum(0)
    dl = T64(MC.coef(W, s, gd, np.float64)['d'])
    ds = 2.0 * st * ((-0.5 * dl ** 3 * gdt) @ q.T)
    ggd, gdd, gs, gW = torch.autograd.grad((ds * T64(vs, False)).sum(), [gdt, dl, st, Wt])
    for t, k in ((ggd, 'ggd'), (gdd, 'gdd'), (gs, 'gs'), (gW, 'gW')):
        close(t, r[k], k)


@pytest.mark.parametrize('case', MC.LAYER_CASES, ids=str)
@pytest.mark.parametrize('act', MC.ACTS, ids=lambda a: a or 'none')
def test_the_factorised_path_length_gradient_is_the_definitions(case, act):
    _, J, ref = M2.layer_path_length(case, MC.layer_definition, act)
    _, J2, got = M2.layer_path_length(case, MC.layer_factorised, act)
    assert np.abs(J - J2).max() <= 1e-10 * max(1.0, np.abs(J).max())
    for k in M2.LAYER_NAMES:
        assert np.abs(got[k] - ref[k]).max() <= 1e-10 * max(1.0, np.abs(ref[k]).max()), k
    assert np.abs(ref['weights']).max() > 0 and np.abs(ref['x']).max() > 0 and np.abs(ref['kernel']).max() > 0


# ---- the C entries -------------------------------------------------------------------------------------------------------------------------
NAMES = (('t2i_demod_act_bwd2_workspace_bytes', 3), ('t2i_demod_act_bwd2', 19), ('t2i_modulate2', 10), ('t2i_demod_coef_bwd2', 16))


def test_abi_declares_binds_and_exports_the_entries(t2i):
    from t2i_amd import _lib
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    for name, nargs in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and len(_lib.SIGNATURES[name][1]) == nargs and name + '(' in header, name
    assert '#define T2I_ABI_VERSION 13' in header                                       # added within v13
    L = _lib.lib
    assert L.t2i_demod_act_bwd2_workspace_bytes(8, 65536, 64) >= 8 * 1024 * 64 * 4
    assert L.t2i_demod_act_bwd2_workspace_bytes(0, 4, 4) == 0 and L.t2i_demod_act_bwd2_workspace_bytes(3, 1 << 31, 1) == 0


def test_every_entry_refuses_bad_arguments_before_any_launch(t2i):
    """No GPU is touched: every refusal returns before the first launch, so the fake pointers are never read."""
    from t2i_amd import _lib
    L = _lib.lib
    P = ctypes.c_void_p
    a = [P(0x100000 * (i + 1)) for i in range(16)]        # distinct, 16-byte aligned, a MiB apart, never dereferenced
    ws, wsn = P(0x10000000), 1 << 20
    INVALID, WORKSPACE = -1, -2

    def act2(g=a[6], c=a[0], d=a[1], bias=a[2], nz=a[3], st=a[4], vc=a[7], vd=a[8], B=2, R=16, C=8, act=2, alpha=0.0, gg=a[9], gc=a[10], gd=a[11],
             w=ws, wn=wsn):
        return L.t2i_demod_act_bwd2(g, c, d, bias, nz, st, vc, vd, B, R, C, act, alpha, gg, gc, gd, w, wn, None)

    def mod2(s=a[1], stride=8, vx=a[2], x=a[0], vs=a[3], B=2, R=16, C=8, gg=a[4]):
        return L.t2i_modulate2(s, stride, vx, x, vs, B, R, C, gg, None)

    def coef2(vs=a[7], gd=a[4], d=a[3], s=a[1], stride=8, W=a[0], q=a[2], T=9, Cin=8, Cout=4, B=2, ggd=a[5], gdd=a[6], dW=a[8], acc=0):
        return L.t2i_demod_coef_bwd2(vs, gd, d, s, stride, W, q, T, Cin, Cout, B, ggd, gdd, dW, acc, None)

    def refused(f, want=INVALID, **kw):
        assert f(**kw) == want, (f.__name__, kw)
        assert L.t2i_last_error()

    for f in (act2, mod2):
        for kw in (dict(B=0), dict(R=0), dict(C=0), dict(R=1 << 31), dict(B=1 << 16, R=1 << 10, C=64)):
            refused(f, **kw)
    for kw in (dict(c=None), dict(vc=None, vd=None), dict(gg=None, gc=None, gd=None), dict(act=3), dict(act=7), dict(act=1, alpha=-0.1),
               dict(act=1, alpha=float('nan')), dict(nz=None), dict(st=None), dict(d=None), dict(d=None, vd=None), dict(vd=None), dict(vc=None),
               dict(g=None), dict(gg=a[0]), dict(gg=a[6]), dict(gg=a[7]), dict(gc=a[8]), dict(gc=a[9]), dict(gd=a[1]), dict(gd=a[10]), dict(gd=a[3])):
        refused(act2, **kw)                                # ... vd or gd without d, gc without vd, gd without vc, gc / gd without g, overlaps
    assert act2(d=None, vd=None, gc=None, gd=None, B=0) == INVALID                       # (the accepted combination, refused only for its shape)
    for kw in (dict(w=None), dict(w=P(0x10000004)), dict(wn=16)):
        refused(act2, WORKSPACE, **kw)
    for kw in (dict(gg=None), dict(vx=None, vs=None), dict(s=None), dict(x=None), dict(stride=7), dict(gg=a[2]), dict(gg=a[0]), dict(gg=a[1]),
               dict(gg=a[3]), dict(B=1 << 10, stride=1 << 21, R=1, C=8)):
        refused(mod2, **kw)
    for kw in (dict(vs=None), dict(gd=None), dict(d=None), dict(s=None), dict(q=None), dict(W=None), dict(ggd=None, gdd=None, dW=None), dict(T=0),
               dict(Cin=0), dict(Cout=0), dict(B=0), dict(stride=7), dict(Cin=1 << 16, Cout=1 << 15, stride=1 << 16),
               dict(T=1 << 12, Cin=1 << 10, Cout=1 << 10, stride=1 << 10), dict(B=1 << 20, Cout=1 << 11), dict(B=1 << 20, stride=1 << 11),
               dict(dW=a[0]), dict(ggd=a[4]), dict(gdd=a[3]), dict(gdd=a[5]), dict(dW=a[7]), dict(ggd=a[2])):
        refused(coef2, **kw)
    for call, words in ((lambda: act2(vc=None, vd=None), 't2i_demod_act_bwd2: .*no cotangent'), (lambda: act2(d=None), 't2i_demod_act_bwd2: .*vd without d'),
                        (lambda: act2(vd=None), 't2i_demod_act_bwd2: .*gc without vd'), (lambda: act2(vc=None), 't2i_demod_act_bwd2: .*gd without vc'),
                        (lambda: act2(wn=16), 't2i_demod_act_bwd2: workspace .*16 bytes where'), (lambda: act2(R=1 << 31), 't2i_demod_act_bwd2: .*2\\^31 elements'),
                        (lambda: mod2(x=None), 't2i_modulate2: .*vx comes with s, vs with x'), (lambda: mod2(gg=a[0]), 't2i_modulate2: .*gg overlaps'),
                        (lambda: coef2(dW=a[0]), 't2i_demod_coef_bwd2: .*overlaps an input'), (lambda: coef2(gdd=a[5]), 't2i_demod_coef_bwd2: .*two outputs overlap'),
                        (lambda: coef2(stride=7), 't2i_demod_coef_bwd2: .*style rows 7 floats apart')):
        assert call() < 0 and re.match(words, L.t2i_last_error().decode()), (words, L.t2i_last_error().decode())


# ---- the keyword and the refusals of the functions ------------------------------------------------------------------------------------------
def test_second_order_on_a_dry_run_creates_the_same_variables(t2i):
    from t2i_amd import kernels as K, scope as S
    from t2i_amd.utils import ops
    x, w, nz = torch.zeros(2, 4, 4, 8), torch.zeros(2, 6), torch.zeros(2, 4, 4)
    made = []
    for second in (False, True):
        st = S.set_default_store(S.VariableStore(device='cpu', seed=0))
        with K.dry_run(), torch.no_grad(), S.variable_scope('t'):
            assert ops.modulated_conv2d(x, w, 12, noise=nz, act=ops.relu, second_order=second).shape == (2, 4, 4, 12)
            assert ops.modulated_conv2d(x, w, 5, ks=(1, 1), act=ops.lrelu_act(0.2), demodulate=False, second_order=second).shape == (2, 4, 4, 5)
        made.append([(n, tuple(v.shape), v.detach().clone()) for n, v in st.vars.items()])
    assert [m[:2] for m in made[0]] == [m[:2] for m in made[1]] and all(torch.equal(a[2], b[2]) for a, b in zip(*made))
    with K.dry_run(), torch.no_grad(), S.variable_scope('u'):
        before = list(S.default_store().vars)
        for bad in (1, 'yes', None):
            with pytest.raises(ValueError, match='modulated_conv2d.*second_order must be'):
                ops.modulated_conv2d(x, w, 12, second_order=bad)
        for kw, err, word in ((dict(act=ops.tanh), ValueError, 'act must be'), (dict(act=torch.relu), ValueError, 'act must be'),
                              (dict(x=x.bfloat16()), ValueError, 'float32')):
            args = dict(x=x, w=w)
            args.update(kw)
            with pytest.raises(err, match='modulated_conv2d.*' + word):
                ops.modulated_conv2d(args.pop('x'), args.pop('w'), 12, second_order=True, **args)
        from t2i_amd import stacked as ST
        with pytest.raises(NotImplementedError, match='modulated_conv2d.*stacked'):
            ops.modulated_conv2d(ST.Stacked(x, x), w, 12, second_order=True)
        assert list(S.default_store().vars) == before


def test_a_third_differentiation_and_a_parameter_gradient_cotangent_raise_by_name(t2i):
    from t2i_amd import autograd as A
    with pytest.raises(NotImplementedError, match='^modulated_conv2d: a third differentiation is not implemented'):
        A._SecondOrder.backward(type('C', (), {'op': 'modulated_conv2d'})())
    v = torch.zeros(3)
    with pytest.raises(NotImplementedError, match='^modulated_conv2d: a cotangent for the gradient of biases is the gradient of a parameter gradient'):
        A.DemodActBwdFn.backward(None, None, None, v, None)
    with pytest.raises(NotImplementedError, match='^modulated_conv2d: a cotangent for the gradient of noise_strength .*input_grads_only'):
        A.DemodActBwdFn.backward(None, None, None, None, v)
    with pytest.raises(NotImplementedError, match='^modulated_conv2d: a cotangent for the gradient of weights .*input_grads_only'):
        A.DemodCoefBwdFn.backward(None, None, v)
    # the first-order functions keep their refusal
    with pytest.raises(NotImplementedError, match='second differentiation'):
        A._FirstOrder.backward(type('C', (), {'op': 'modulated_conv2d'})())
    assert issubclass(A.ModulateFn2, A.ModulateFn) and issubclass(A.DemodCoefFn2, A.DemodCoefFn) and issubclass(A.DemodActFn2, A.DemodActFn)
