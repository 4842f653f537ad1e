"""Spectral normalisation on the GPU (csrc/t2i_spectral.hip, optim.SpectralNorm, optim.AdamTF(spectral=...)) against the float64
restatement of tests/sn_cases.py on the test arena, every comparison from the same fp32 state (no compounding over steps).  Bounds are
those of tests/test_norm_second_order_gpu.py: 1e-5 forward quantities (u, v, sigma, flat, raw), 1e-4 gradients, max-norm relative per
tensor.  Bit-for-bit: the slots that are not normalised, the padding, repeated calls, iterations = 3 against three calls of 1, a matrix
alone against the same matrix inside the arena, Adam on raw against K.adam_tf / K.adam_tf_slots, and a captured apply() against eager."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import sn_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

FWD, GRAD = 1e-5, 1e-4
VALUES, GRADS = SC.arena_values(), SC.arena_grads()


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def make(names=None, warmup=0, normalised=None, seed=0):
    from t2i_amd import optim
    names = list(names or VALUES)
    vs = OrderedDict((n, torch.tensor(VALUES[n], device='cuda').requires_grad_()) for n in names)
    arena = optim.Arena(vs)
    sn = optim.SpectralNorm(arena, [n for n in names if n in (normalised or SC.NORMALISED)], seed=seed, warmup=warmup)
    return arena, sn


def set_grads(arena, scale=1.0):
    with torch.no_grad():
        arena.grad.zero_()
        for n in arena.names:
            arena.grad_of(n).copy_(torch.tensor(GRADS[n] * np.float32(scale), device='cuda'))


def state(arena, sn):
    torch.cuda.synchronize()
    return OrderedDict((k, t.detach().clone()) for k, t in (('flat', arena.flat), ('raw', sn.raw), ('u', sn.u), ('v', sn.v), ('sigma', sn.sigma)))


def put(arena, sn, st):
    with torch.no_grad():
        for k, t in (('flat', arena.flat), ('raw', sn.raw), ('u', sn.u), ('v', sn.v), ('sigma', sn.sigma)):
            t.copy_(st[k])


def same(a, b, keys=None):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in (keys or a))


def slot(sn, arena, st, n):
    """(raw, flat, u, v, sigma) of variable n out of a state, as float64 numpy"""
    i = sn.index[n]
    o, k = arena.offsets[n]
    _, R, C, uo, vo = (int(x) for x in sn.table.host[i][:5])
    f = lambda t: t.double().cpu().numpy()       # noqa: E731
    return f(st['raw'][o:o + k]).reshape(R, C), f(st['flat'][o:o + k]).reshape(R, C), f(st['u'][uo:uo + C]), f(st['v'][vo:vo + R]), float(st['sigma'][i])


def check_iteration(arena, sn, before, after, iterations, tag):
    worst = dict(u=0.0, v=0.0, sigma=0.0, flat=0.0)
    for n in sn.names:
        raw, _, u0, _, _ = slot(sn, arena, before, n)
        raw1, flat, u, v, sigma = slot(sn, arena, after, n)
        assert np.array_equal(raw, raw1)
        ur, vr, sr = SC.iterate(raw, u0, iterations)
        e = dict(u=SC.relerr(u, ur), v=SC.relerr(v, vr), sigma=abs(sigma - sr) / sr, flat=SC.relerr(flat, SC.normalised(raw, sr)))
        print('%s %s [%d, %d]: u %.2e  v %.2e  sigma %.2e  flat %.2e' % ((tag, n) + raw.shape + (e['u'], e['v'], e['sigma'], e['flat'])))
        for k in e:
            worst[k] = max(worst[k], e[k])
            assert e[k] <= FWD, (n, k, e[k])
    print('%s: maxima u %.2e  v %.2e  sigma %.2e  flat %.2e' % (tag, worst['u'], worst['v'], worst['sigma'], worst['flat']))


def check_rest(arena, sn, st):
    """The slots that are not normalised equal raw bit for bit, and the padding of every slot is 0 in flat and in raw."""
    for n in arena.names:
        o, k = arena.offsets[n]
        end = o + (k + 3) // 4 * 4
        if n not in sn.index:
            assert torch.equal(_bits(st['flat'][o:o + k]), _bits(st['raw'][o:o + k])), n
        assert not st['flat'][o + k:end].any() and not st['raw'][o + k:end].any(), n
    assert any((k % 4) for _, k in arena.offsets.values())                                    # (the arena has a padded slot)


def test_one_iteration_from_the_drawn_u_and_from_a_warmed_state():
    need_gpu()
    arena, sn = make()
    s0 = state(arena, sn)
    assert torch.equal(s0['flat'], s0['raw']) and bool((s0['sigma'] == 1).all()) and not s0['v'].any()      # warmup = 0: nothing moved
    sn.normalize(1)
    s1 = state(arena, sn)
    check_iteration(arena, sn, s0, s1, 1, 'first iteration')
    check_rest(arena, sn, s1)
    sn.normalize(SC.WARMUP - 1)
    s15 = state(arena, sn)
    sn.normalize(1)
    s16 = state(arena, sn)
    check_iteration(arena, sn, s15, s16, 1, 'iteration 16')
    check_rest(arena, sn, s16)
    for n in sn.names:                                           # and the warmed estimate is the top singular value's, as on the host
        raw, _, _, _, sigma = slot(sn, arena, s16, n)
        top = float(np.linalg.svd(raw, compute_uv=False)[0])
        assert 0.95 * top <= sigma <= (1.0 + 1e-5) * top, (n, sigma, top)
    # construction with warmup runs the same launches
    arena2, sn2 = make(warmup=SC.WARMUP)
    assert same(state(arena2, sn2), s15)


def test_the_other_slots_follow_raw_and_iterations_0_only_rewrites_flat():
    need_gpu()
    arena, sn = make(warmup=2)
    with torch.no_grad():
        sn.raw.mul_(1.5)                                          # raw moves (as an optimizer step would); the padding stays 0
        arena.flat.fill_(7.0)
    before = state(arena, sn)
    sn.normalize(0)
    after = state(arena, sn)
    assert same(before, after, ('raw', 'u', 'v', 'sigma'))
    check_rest(arena, sn, after)
    for n in sn.names:
        raw, flat, _, _, sigma = slot(sn, arena, after, n)
        assert SC.relerr(flat, SC.normalised(raw, sigma)) <= FWD, n
    for n in arena.names:
        if n not in sn.index:
            o, k = arena.offsets[n]
            assert torch.equal(after['flat'][o:o + k], torch.tensor(VALUES[n], device='cuda').reshape(-1) * 1.5), n


def test_three_iterations_are_three_calls_and_calls_repeat():
    need_gpu()
    arena, sn = make(warmup=1)
    s0 = state(arena, sn)
    sn.normalize(3)
    a = state(arena, sn)
    check_iteration(arena, sn, s0, a, 3, 'three iterations')
    put(arena, sn, s0)
    for _ in range(3):
        sn.normalize(1)
    b = state(arena, sn)
    put(arena, sn, s0)
    sn.normalize(3)
    c = state(arena, sn)
    assert same(a, b) and same(a, c) and not same(a, s0, ('u',))
    set_grads(arena)
    g0 = arena.grad.clone()
    sn.grad_()
    g1 = arena.grad.clone()
    arena.grad.copy_(g0)
    sn.grad_()
    torch.cuda.synchronize()
    assert torch.equal(_bits(arena.grad), _bits(g1)) and not torch.equal(g1, g0)


def test_the_gradient_transform():
    need_gpu()
    arena, sn = make(warmup=3)
    st = state(arena, sn)
    set_grads(arena)
    g0 = arena.grad.clone()
    sn.grad_()
    torch.cuda.synchronize()
    assert same(state(arena, sn), st)                              # nothing but the gradient arena is written
    worst = seen = 0.0
    for n in arena.names:
        o, k = arena.offsets[n]
        end = o + (k + 3) // 4 * 4
        assert torch.equal(_bits(arena.grad[o + k:end]), _bits(g0[o + k:end]))
        if n not in sn.index:
            assert torch.equal(_bits(arena.grad[o:o + k]), _bits(g0[o:o + k])), n
            continue
        _, W, u, v, sigma = slot(sn, arena, st, n)
        G = g0[o:o + k].double().cpu().numpy().reshape(W.shape)
        ref = SC.grad_raw(G, W, u, v, sigma)
        got = arena.grad[o:o + k].double().cpu().numpy().reshape(W.shape)
        if W.size == 1:                                            # W = +-1, v u = +-1: the gradient of raw / |raw| is 0
            assert abs(ref.item()) <= 1e-12 * abs(G.item()) / sigma and abs(got.item()) <= GRAD * abs(G.item()) / sigma
            continue
        e = SC.relerr(got, ref)
        print('gradient transform %s: %.2e   <G, W> = %.6g' % (n, e, float(np.sum(G * W))))
        worst = max(worst, e)
        seen = max(seen, SC.relerr(ref, G / sigma))
        assert e <= GRAD, (n, e)
    print('gradient transform: maximum %.2e' % worst)
    assert seen > 100 * GRAD                                       # (the rank-1 term is far above the bound: dropping it would fail)


@pytest.mark.parametrize('scales', [False, True], ids=['plain', 'slot_scales'])
def test_apply_steps_raw_with_the_transformed_gradient(scales):
    need_gpu()
    from t2i_amd import kernels as K
    from t2i_amd import optim
    arena, sn = make(warmup=3)
    kw = dict(slot_scales={SC.ALONE: 0.25, 'd_net/fc/kernel': (2.0, 0.5), 'd_net/a/biases': (1.0, 3.0)}) if scales else {}
    opt = optim.AdamTF(arena, 0.0, 0.99, spectral=sn, **kw)
    assert opt.skip_m
    set_grads(arena)
    s0 = state(arena, sn)
    g0 = arena.grad.clone()
    lr = 1e-3
    opt.prepare(lr)
    opt.apply(grad_scale=0.5)
    s1 = state(arena, sn)
    # (1) arena.grad holds the transformed gradient
    expect = arena.grad.clone()
    arena.grad.copy_(g0)
    put(arena, sn, s0)                                             # the transform used the u, v, sigma and W of before the step
    sn.grad_()
    torch.cuda.synchronize()
    assert torch.equal(_bits(arena.grad), _bits(expect)) and not torch.equal(expect, g0)
    put(arena, sn, s1)
    # (2) raw is Adam's step of the old raw with it, bit for bit
    w, v = s0['raw'].clone(), torch.zeros_like(s0['raw'])
    if scales:
        K.adam_tf_slots(w, expect, None, v, opt.slot_end, opt.slot_mult, 0.0, 0.0, 0.99, 1e-8, 0.5, lr_t_dev=opt.lr_t_dev)
    else:
        K.adam_tf(w, expect, None, v, 0.0, 0.0, 0.99, 1e-8, 0.5, lr_t_dev=opt.lr_t_dev)
    torch.cuda.synchronize()
    assert torch.equal(_bits(s1['raw']), _bits(w)) and torch.equal(_bits(opt.v), _bits(v)) and not torch.equal(w, s0['raw'])
    # ... and the float64 restatement of that step, per variable (multipliers (1, 1) where none is named)
    mult = {n: (1.0, 1.0) for n in arena.names}
    if scales:
        mult.update({SC.ALONE: (0.25, 0.25), 'd_net/fc/kernel': (2.0, 0.5), 'd_net/a/biases': (1.0, 3.0)})
    for n in arena.names:
        o, k = arena.offsets[n]
        ref, _, _ = SC.adam_tf(s0['raw'][o:o + k].double().cpu().numpy(), expect[o:o + k].double().cpu().numpy(), np.zeros(k), 1, lr,
                               grad_scale=0.5, grad_mult=mult[n][0], lr_mult=mult[n][1])
        assert SC.relerr(s1['raw'][o:o + k].double().cpu().numpy(), ref) <= FWD, n
    # (3) one power iteration on the new raw from the old u, and flat rewritten from it
    check_iteration(arena, sn, dict(s0, raw=s1['raw']), s1, 1, 'after apply()')
    check_rest(arena, sn, s1)
    # the on-demand first moment is the moment of raw: the transformed gradient times what the launch scaled it by
    o, k = arena.offsets['d_net/d/weights']
    assert torch.equal(opt.m[o:o + k], expect[o:o + k] * 0.5)


def test_a_matrix_gives_the_same_bits_alone_and_inside_the_arena():
    need_gpu()
    arena, sn = make()
    alone, sn1 = make(names=[SC.ALONE])
    n = SC.ALONE
    C = SC.ARENA[n][-1]
    uo = int(sn.table.host[sn.index[n]][3])
    with torch.no_grad():
        sn1.u[:C].copy_(sn.u[uo:uo + C])
    for a, s in ((arena, sn), (alone, sn1)):
        s.normalize(2)
        set_grads(a)
        s.grad_()
    torch.cuda.synchronize()
    big, one = state(arena, sn), state(alone, sn1)
    (o, k), (o1, k1) = arena.offsets[n], alone.offsets[n]
    _, R, _, _, vo = (int(x) for x in sn.table.host[sn.index[n]][:5])
    assert (o1, k1) == (0, k) and o > 0 and uo > 0 and vo > 0
    assert torch.equal(_bits(big['flat'][o:o + k]), _bits(one['flat'][:k])) and torch.equal(_bits(big['u'][uo:uo + C]), _bits(one['u'][:C]))
    assert torch.equal(_bits(big['v'][vo:vo + R]), _bits(one['v'][:R])) and torch.equal(_bits(big['sigma'][sn.index[n]:sn.index[n] + 1]), _bits(one['sigma'][:1]))
    assert torch.equal(_bits(arena.grad[o:o + k]), _bits(alone.grad[:k])) and float(one['sigma'][0]) != 1.0


def test_sync_and_the_state_dict():
    """sync(names): those slots restart from the weights the arena holds, the others keep their state bit for bit; a state_dict loads
    verbatim into a fresh object."""
    need_gpu()
    arena, sn = make(warmup=SC.WARMUP)
    s0 = state(arena, sn)
    names = ['d_net/fc/kernel', 'd_net/d/weights']
    with torch.no_grad():
        for n in names:
            arena.grad_of(n)                                       # (exists)
            o, k = arena.offsets[n]
            arena.flat[o:o + k].copy_(torch.tensor(VALUES[n], device='cuda').reshape(-1) * 2.0)
    sn.sync(names)
    s1 = state(arena, sn)
    for n in sn.names:
        raw, flat, u, v, sigma = slot(sn, arena, s1, n)
        raw0, flat0, u0, v0, sigma0 = slot(sn, arena, s0, n)
        if n in names:
            assert np.array_equal(raw, VALUES[n].astype(np.float64).reshape(raw.shape) * 2.0)
            # twice the matrix, iterated on from the u it had: the estimate cannot fall below twice the old one or rise above twice the top
            top = float(np.linalg.svd(raw0, compute_uv=False)[0])
            assert 2.0 * sigma0 * (1.0 - FWD) <= sigma <= 2.0 * top * (1.0 + FWD) and SC.relerr(flat, SC.normalised(raw, sigma)) <= FWD, n
        else:
            assert np.array_equal(raw, raw0) and np.array_equal(u, u0) and np.array_equal(v, v0) and sigma == sigma0 and np.array_equal(flat, flat0), n
    arena2, sn2 = make(seed=9)
    f2 = arena2.flat.clone()
    sn2.load_state_dict(sn.state_dict())
    assert same(state(arena2, sn2), s1, ('raw', 'u', 'v', 'sigma')) and torch.equal(_bits(arena2.flat), _bits(f2))      # verbatim; flat is not touched
    sn2.normalize(0)
    assert same(state(arena2, sn2), s1)


def test_a_captured_apply_replayed_twice_equals_two_eager_calls():
    need_gpu()
    from t2i_amd import optim
    from t2i_amd.graphs import capture_mode
    ends = []
    for captured in (False, True):
        arena, sn = make(warmup=2)
        opt = optim.AdamTF(arena, 0.0, 0.99, spectral=sn, slot_scales={SC.ALONE: 0.5})
        set_grads(arena)
        opt.step(1e-3)                                 # one eager step first (it also loads the kernels before any capture)
        if captured:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode=capture_mode()):
                opt.apply(grad_scale=0.5)
        for i in range(2):
            set_grads(arena, scale=1.0 + i)
            opt.prepare(1e-3 * (2 + i))
            if captured:
                graph.replay()
            else:
                opt.apply(grad_scale=0.5)
        ends.append((state(arena, sn), opt.v.clone(), arena.grad.clone(), opt.t))
    (s0, v0, g0, t0), (s1, v1, g1, t1) = ends
    assert t0 == t1 == 3 and same(s0, s1) and torch.equal(_bits(v0), _bits(v1)) and torch.equal(_bits(g0), _bits(g1))
    assert bool(torch.isfinite(s0['flat']).all()) and bool((s0['sigma'] > 0).all())


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if 'cuda' in str(getattr(e, 'device_type', '')).lower()]


def test_the_launch_count_does_not_depend_on_the_slots():
    """apply() with spectral= enqueues six kernels more than without (dot, correction, rows, columns, finish, rewrite), in a nine-slot
    arena as in a one-slot arena."""
    need_gpu()
    from t2i_amd import optim
    counts = {}
    for tag, names in (('arena', None), ('alone', [SC.ALONE])):
        arena, sn = make(names=names, warmup=1)
        plain, spec = optim.AdamTF(arena, 0.0, 0.99), optim.AdamTF(arena, 0.0, 0.99, spectral=sn)
        set_grads(arena)
        for o in (plain, spec):                       # (the first call loads code objects)
            o.prepare(1e-3)
            o.apply(refresh=False)
        a, b = _kernels(lambda: plain.apply(refresh=False)), _kernels(lambda: spec.apply(refresh=False))
        print('%s: %d kernel(s) without, %d with: %s' % (tag, len(a), len(b), b))
        counts[tag] = (len(a), len(b))
        assert sum('sn_' in k for k in b) == 6 and not any('sn_' in k for k in a)
    assert counts['arena'] == counts['alone'] and counts['arena'][1] - counts['arena'][0] == 6
