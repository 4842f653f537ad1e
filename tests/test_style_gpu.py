"""The style layer's kernels on the GPU (csrc/t2i_style.hip) against the float64 restatement of
tests/style_cases.py: the case table (forward and all four gradients), a mean of 100 sigma, a constant channel, strength 0, independence
of the batch, repeatability, the scalar form, the wrapped grid, a captured forward + backward, and the refused second differentiation.

Tolerance per case and tensor: max(floor, 8 e32) relative to the largest reference entry, e32 = the error of the float32 numpy evaluation
of the restatement on that case (style_cases.tolerances); floors 1e-5 (y, dys, dyb, dstrength) and 1e-4 (dx)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import style_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    from t2i_amd.utils import ops
    assert kernels.ADAIN_CHUNK_ROWS == SC.CHUNK
    return ops


def _act(ops, act):
    return {None: None, 'relu': ops.relu, 'lrelu': ops.lrelu_act(SC.ALPHA)}[act]


def _dev(a, grad=False):
    return None if a is None else torch.tensor(a).cuda().requires_grad_(grad)


def run(ops, inp, act, grads=True, wrap=None):
    """ops.adain on the case's inputs -> dict of device tensors (y, dx, dstrength, dys, dyb).  wrap: applied to the device x first."""
    x = _dev(inp['x'])
    if wrap is not None:
        x = wrap(x)
    x.requires_grad_(grads)
    ys, yb, st = _dev(inp['ys'], grads), _dev(inp['yb'], grads), _dev(inp['strength'], grads)
    y = ops.adain(x, ys, yb, noise=_dev(inp['noise']), strength=st, act=_act(ops, act))
    out = dict(y=y.detach())
    if grads:
        y.backward(_dev(inp['g']))
        out.update(dx=x.grad, dys=ys.grad, dyb=yb.grad, dstrength=None if st is None else st.grad)
    return out


def check(got, ref, tol, label):
    """-> the largest error / tolerance over the tensors; asserts each is within its tolerance"""
    worst = 0.0
    for k, t in tol.items():
        err = SC.relerr(got[k].cpu().numpy(), ref[k])
        assert np.isfinite(err) and err <= t, (label, k, err, t)
        worst = max(worst, err / t)
    return worst


GROUPS = {}
for _i, _c in enumerate(SC.CASES):
    GROUPS.setdefault(SC.group_of(_c), []).append(_i)


def test_the_table_covers_every_dimension():
    cs = SC.CASES
    assert {c[0] for c in cs} == {1, 3} and {c[1:3] for c in cs} >= set(SC.MAPS) and {c[3] for c in cs} == set(SC.CHANNELS) | {512}
    assert {c[1] * c[2] for c in cs} >= {SC.CHUNK - 1, SC.CHUNK, SC.CHUNK + 1, 2 * SC.CHUNK + 1, 1, 16, 15, 1023, 4096}
    assert {(c[4], c[5]) for c in cs} == {(a, n) for a in SC.ACTS for n in (False, True)}
    for hw in SC.MAPS:                                              # every map meets every channel count
        assert {c[3] for c in cs if c[1:3] == hw} >= set(SC.CHANNELS), hw
    assert {(c[4], c[5]) for c in cs if c[1:4] == (64, 64, 64)} == {(a, n) for a in SC.ACTS for n in (False, True)}
    assert {(c[4], c[5]) for c in cs if c[1:4] == (4, 4, 512)} == {(a, n) for a in SC.ACTS for n in (False, True)}


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_forward_and_gradients_against_float64(ops, group):
    worst = (0.0, '')
    for i in GROUPS[group]:
        inp, ref, tol = SC.reference(i)
        act = SC.CASES[i][4]
        r = check(run(ops, inp, act), ref, tol, SC.case_id(SC.CASES[i]))
        worst = max(worst, (r, SC.case_id(SC.CASES[i])))
    print('adain %s: %d cases, largest error / tolerance %.3f (%s)' % (group, len(GROUPS[group]), worst[0], worst[1]))


@pytest.mark.parametrize('act', [None, 'relu'], ids=['none', 'relu'])
def test_a_mean_of_100_sigma(ops, act):
    """2 x 64 x 64 x 8 with x ~ N(100, 1): the same rule.  The one-pass variance E[u^2] - mu^2, evaluated in float32 numpy, is far outside it."""
    shape = (2, 64, 64, 8)
    rng = np.random.default_rng(5)
    inp = SC.inputs(shape, True, act, seed=9)
    inp['x'] = (100.0 + rng.standard_normal(shape)).astype(np.float32)
    ref = SC.evaluate(inp, act, np.float64)
    tol = SC.tolerances(ref, SC.evaluate(inp, act, np.float32))
    r = check(run(ops, inp, act), ref, tol, 'mean100')
    one = SC.evaluate(inp, act, np.float32, one_pass=True)
    bad = SC.relerr(one['y'], ref['y']) / tol['y']
    print('adain mean 100 (%s): largest error / tolerance %.3f; tolerance y %.2e; one-pass float32 variance: %.0f x the tolerance' % (
        act or 'none', r, tol['y'], bad))
    assert not (bad <= 10.0)                                        # (NaN included: the one-pass form is what the rule excludes)


@pytest.mark.parametrize('act', SC.ACTS, ids=lambda a: a or 'none')
@pytest.mark.parametrize('shape', [(2, 8, 8, 8), (3, 5, 13, 3), (1, 3, 43, 68)], ids=lambda s: 'x'.join(map(str, s)))
def test_a_constant_channel_gives_yb_exactly(ops, shape, act):
    inp = SC.inputs(shape, False, act)
    C = shape[3]
    inp['x'][..., C - 1] = np.float32(0.7310585)                    # variance 0
    inp['x'][:, :, :, 0] = np.arange(shape[0], dtype=np.float32)[:, None, None] * np.float32(1.37) + np.float32(3.3)
    got = run(ops, inp, act)
    y = got['y'].cpu().numpy()
    assert np.isfinite(y).all() and np.isfinite(got['dx'].cpu().numpy()).all()
    for c in (0, C - 1):
        assert (y[..., c] == inp['yb'][:, None, None, c]).all(), c


@pytest.mark.parametrize('i', [i for i, c in enumerate(SC.CASES) if c[5]][::7][:5])
def test_strength_zero_is_the_call_without_noise(ops, i):
    inp, _, _ = SC.reference(i)
    act = SC.CASES[i][4]
    zero = dict(inp, strength=np.zeros_like(inp['strength']))
    plain = dict(inp, noise=None, strength=None)
    a, b = run(ops, zero, act), run(ops, plain, act)
    for k in ('y', 'dx', 'dys', 'dyb'):
        assert torch.equal(a[k], b[k]), k


PICKS = [(3, 33, 31, 20, 'relu', True), (3, 5, 13, 3, 'lrelu', True), (3, 3, 43, 68, None, False), (3, 64, 64, 64, 'relu', True), (3, 4, 4, 512, 'lrelu', True)]


@pytest.mark.parametrize('case', PICKS, ids=[SC.case_id(c) for c in PICKS])
def test_a_batch_row_is_the_sample_alone_and_calls_repeat(ops, case):
    B, H, W, C, act, nz = case
    inp = SC.inputs((B, H, W, C), nz, act, seed=3)
    full = run(ops, inp, act)
    again = run(ops, inp, act)
    for k, v in full.items():
        assert v is None or torch.equal(v, again[k]), k
    for b in range(B):
        one = {k: (v if v is None or k == 'strength' else np.ascontiguousarray(v[b:b + 1])) for k, v in inp.items()}
        alone = run(ops, one, act)
        for k in ('y', 'dx', 'dys', 'dyb'):
            assert torch.equal(full[k][b:b + 1], alone[k]), (k, b)


@pytest.mark.parametrize('case', [(3, 9, 8, 4, 'relu', True), (2, 5, 13, 68, 'lrelu', False)], ids=lambda c: SC.case_id(c))
def test_a_base_misaligned_by_one_float_takes_the_scalar_form(ops, case):
    B, H, W, C, act, nz = case
    inp = SC.inputs((B, H, W, C), nz, act, seed=4)
    ref = SC.evaluate(inp, act, np.float64)
    tol = SC.tolerances(ref, SC.evaluate(inp, act, np.float32))

    def shifted(x):
        buf = torch.zeros(x.numel() + 5, device='cuda')
        xm = buf[1:1 + x.numel()].view(x.shape)
        xm.copy_(x)
        assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
        return xm.detach()
    vec = run(ops, inp, act)
    sca = run(ops, inp, act, wrap=shifted)
    check(vec, ref, tol, 'vector'); check(sca, ref, tol, 'scalar')
    for k in tol:                                                   # the two forms against each other: twice the rule at the most
        assert SC.relerr(sca[k].cpu().numpy(), vec[k].cpu().numpy()) <= 2 * tol[k], k


def test_a_batch_beyond_the_grid_limit_is_wrapped(ops):
    """B = 70000 of 1 x 2 x 1: more items than the launch has workgroups (65535), reached by the stride."""
    shape = (70000, 1, 2, 1)
    inp = SC.inputs(shape, True, 'lrelu', seed=6)
    ref = SC.evaluate(inp, 'lrelu', np.float64)
    tol = SC.tolerances(ref, SC.evaluate(inp, 'lrelu', np.float32))
    got = run(ops, inp, 'lrelu')
    check(got, ref, tol, 'wrapped')
    assert float(got['y'][65535:].abs().min()) > 0.0                # the rows past the first sweep were written


def test_a_captured_forward_and_backward_replayed_equals_eager(ops):
    B, H, W, C, act = 2, 33, 31, 20, 'relu'
    inp = SC.inputs((B, H, W, C), True, act, seed=7)
    x, ys, yb, st = _dev(inp['x'], True), _dev(inp['ys'], True), _dev(inp['yb'], True), _dev(inp['strength'], True)
    noise, g = _dev(inp['noise']), _dev(inp['g'])
    leaves = (x, ys, yb, st)

    def step():
        y = ops.adain(x, ys, yb, noise=noise, strength=st, act=_act(ops, act))
        return (y,) + torch.autograd.grad(y, leaves, g)
    step()                                                          # the kernels are loaded and the workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    gen = torch.Generator(device='cuda').manual_seed(11)
    seen = []
    for _ in range(2):
        noise.copy_(torch.randn(noise.shape, generator=gen, device='cuda'))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        eager = step()
        for a, b in zip(replayed, eager):
            assert torch.equal(a, b)
        seen.append(replayed[0])
    assert not torch.equal(seen[0], seen[1])                        # the re-drawn noise reached the replay


def test_a_second_differentiation_is_refused(ops):
    inp = SC.inputs((2, 4, 4, 8), True, 'relu')
    x, ys, yb, st = _dev(inp['x'], True), _dev(inp['ys'], True), _dev(inp['yb'], True), _dev(inp['strength'], True)
    y = ops.adain(x, ys, yb, noise=_dev(inp['noise']), strength=st, act=ops.relu)
    gx, = torch.autograd.grad(y, x, _dev(inp['g']), create_graph=True)
    with pytest.raises(NotImplementedError, match='second differentiation'):
        torch.autograd.grad(gx.sum(), x)


def test_input_grads_only_skips_the_strength_gradient(ops):
    from t2i_amd import autograd as A
    inp = SC.inputs((2, 4, 4, 8), True, 'relu')
    x, ys, yb, st = _dev(inp['x'], True), _dev(inp['ys'], True), _dev(inp['yb'], True), _dev(inp['strength'], True)
    y = ops.adain(x, ys, yb, noise=_dev(inp['noise']), strength=st, act=ops.relu)
    with A.input_grads_only():
        gx, gs, gb, gst = torch.autograd.grad(y, (x, ys, yb, st), _dev(inp['g']), allow_unused=True)
    assert gst is None and gx is not None and gs is not None and gb is not None
