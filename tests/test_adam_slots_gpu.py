"""Per-slot multipliers in the Adam launch on the GPU: t2i_adam_tf_slots against t2i_adam_tf / t2i_adam_tf_ema
bit for bit (an all-ones table; a general table against one launch per slot), its refusals, optim.AdamTF(slot_scales=...) against the
float64 explicit form of the equalized learning rate, its first moment, apply() under graph replay, PGGAN(equalized_lr=True) eager and
replayed, and train_pggan.py --equalized-lr --lr over the first three schedule entries."""
import ctypes
import itertools
import math
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

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
EMA = '/ExponentialMovingAverage'
TINY = dict(fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)      # tests/test_pggan.py's widths
SIZES = (1, 3, 4, 5, 64, 1027, 4101)
MULTS = ((math.sqrt(2.0 / 27), 0.01), (3.0, math.sqrt(2.0 / 27)), (0.01, 3.0), (1.0, 0.5), (math.sqrt(2.0 / 4608), 1.0))   # grad_mult != lr_mult
BOUND = 1e-6                       # the project's bound for an Adam launch (test_adam_golden)
GSCALE, LR_T, DECAY = 0.5, 3e-3, 0.9


def _bits(t):
    return t.detach().reshape(-1).view(torch.int32)


def _pad(k):
    return (k + 3) // 4 * 4


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _layout(sizes):
    """-> (n, slot ends (padded), mask of the elements that belong to a variable)"""
    ends, off = [], 0
    live = []
    for k in sizes:
        live.append(torch.arange(off, off + k))
        off += _pad(k)
        ends.append(off)
    mask = torch.zeros(off, dtype=torch.bool)
    mask[torch.cat(live)] = True
    return off, ends, mask.to(DEV)


def _inputs(n, mask, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda: torch.randn(n, generator=g, device=DEV) * mask       # noqa: E731  (padding elements are zero)
    return dict(w=r(), g=r() * 3.0, m=r() * 0.1, v=r().abs() * 0.01, s=r())


LAYOUTS = {'sizes': (SIZES, 2048), 'sizes, 2 blocks': (SIZES, 2), '600 slots of 4, 1 block': ((4,) * 600, 1)}
# (beta1, m given), lr_t on the device, shadow: None / decay on the host / decay on the device
COMBOS = list(itertools.product(((0.0, False), (0.0, True), (0.5, True)), (False, True), (None, 'host', 'dev')))


def _plain(x, beta1, has_m, lr_t, lr_buf, gscale, shadow, d_buf, lo=0, hi=None):
    """t2i_adam_tf / t2i_adam_tf_ema on [lo, hi) of the buffers in x (in place)."""
    from t2i_amd import kernels as K
    sl = slice(lo, hi)
    m = x['m'][sl] if has_m else None
    if shadow is None:
        K.adam_tf(x['w'][sl], x['g'][sl], m, x['v'][sl], lr_t, beta1, 0.99, 1e-8, gscale, lr_t_dev=lr_buf)
    else:
        K.adam_tf_ema(x['w'][sl], x['g'][sl], m, x['v'][sl], x['s'][sl], lr_t, beta1, 0.99, 1e-8, gscale,
                      7.0 if d_buf is not None else DECAY, lr_t_dev=lr_buf, ema_decay_dev=d_buf)


def _slots(x, ends, mult, beta1, has_m, lr_dev, shadow):
    from t2i_amd import kernels as K
    lr_buf = torch.full((4,), LR_T, device=DEV) if lr_dev else None
    d_buf = torch.full((4,), DECAY, device=DEV) if shadow == 'dev' else None
    # with a device scalar the host value is ignored: pass one that would be wrong / refused
    K.adam_tf_slots(x['w'], x['g'], x['m'] if has_m else None, x['v'], ends, mult, 0.0 if lr_dev else LR_T, beta1, 0.99, 1e-8, GSCALE,
                    ema=None if shadow is None else x['s'], ema_decay=7.0 if shadow == 'dev' else DECAY, lr_t_dev=lr_buf, ema_decay_dev=d_buf)


def _same(a, b, has_m, shadow, what):
    for k in ('w', 'v', 'g') + (('m',) if has_m else ()) + (('s',) if shadow is not None else ()):
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


@pytest.mark.parametrize('layout', list(LAYOUTS), ids=list(LAYOUTS))
def test_all_ones_table_equals_the_plain_launches(layout):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    sizes, blocks = LAYOUTS[layout]
    n, ends, mask = _layout(sizes)
    ends_dev = torch.tensor(ends, dtype=torch.int64, device=DEV)
    ones = torch.ones((len(ends), 2), device=DEV)
    K.tuning_set('adam_blocks', blocks)
    try:
        for case, ((beta1, has_m), lr_dev, shadow) in enumerate(COMBOS):
            x0 = _inputs(n, mask, 1000 + case)
            a, b = {k: t.clone() for k, t in x0.items()}, {k: t.clone() for k, t in x0.items()}
            lr_buf = torch.full((4,), LR_T, device=DEV) if lr_dev else None
            d_buf = torch.full((4,), DECAY, device=DEV) if shadow == 'dev' else None
            _plain(a, beta1, has_m, 0.0 if lr_dev else LR_T, lr_buf, GSCALE, shadow, d_buf)
            _slots(b, ends_dev, ones, beta1, has_m, lr_dev, shadow)
            torch.cuda.synchronize()
            what = (layout, beta1, has_m, lr_dev, shadow)
            assert not torch.equal(a['w'], x0['w']), what
            _same(b, a, has_m, shadow, what)
            if not has_m:
                assert torch.equal(_bits(b['m']), _bits(x0['m'])), what
            if shadow is None:
                assert torch.equal(_bits(b['s']), _bits(x0['s'])), what
    finally:
        K.tuning_set('adam_blocks', 2048)


@pytest.mark.parametrize('layout', list(LAYOUTS), ids=list(LAYOUTS))
def test_general_table_equals_one_plain_launch_per_slot(layout):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    sizes, blocks = LAYOUTS[layout]
    n, ends, mask = _layout(sizes)
    ends_dev = torch.tensor(ends, dtype=torch.int64, device=DEV)
    mults = [MULTS[(s * 3 + s // 5) % len(MULTS)] for s in range(len(ends))]
    mult_dev = torch.tensor(mults, dtype=torch.float32, device=DEV)
    # the two fp32 products per slot, formed on the host
    gs = [float(np.float32(GSCALE) * np.float32(gm)) for gm, _ in mults]
    lrs = [float(np.float32(LR_T) * np.float32(lm)) for _, lm in mults]
    lr_rows = torch.tensor(lrs, dtype=torch.float32, device=DEV).reshape(-1, 1).repeat(1, 4).contiguous()      # one 16-byte row per slot
    assert np.array_equal(lr_rows[:, 0].cpu().numpy(), np.array(lrs, np.float32))
    d_buf0 = torch.full((4,), DECAY, device=DEV)
    try:
        for case, ((beta1, has_m), lr_dev, shadow) in enumerate(COMBOS):
            x0 = _inputs(n, mask, 2000 + case)
            a, b = {k: t.clone() for k, t in x0.items()}, {k: t.clone() for k, t in x0.items()}
            K.tuning_set('adam_blocks', 2048)
            lo = 0
            for s, hi in enumerate(ends):
                _plain(a, beta1, has_m, 0.0 if lr_dev else lrs[s], lr_rows[s] if lr_dev else None, gs[s], shadow,
                       d_buf0 if shadow == 'dev' else None, lo, hi)
                lo = hi
            K.tuning_set('adam_blocks', blocks)
            _slots(b, ends_dev, mult_dev, beta1, has_m, lr_dev, shadow)
            torch.cuda.synchronize()
            what = (layout, beta1, has_m, lr_dev, shadow)
            _same(b, a, has_m, shadow, what)
            assert not torch.equal(b['w'][mask], x0['w'][mask]), what                 # w actually changed
            for k in ('w', 'v') + (('m',) if has_m else ()) + (('s',) if shadow is not None else ()):
                assert bool((b[k][~mask] == 0).all()), (what, k)                      # padding stays zero
            # the table did something: the all-ones launch gives other weights
            c = {k: t.clone() for k, t in x0.items()}
            _slots(c, ends_dev, torch.ones_like(mult_dev), beta1, has_m, lr_dev, shadow)
            assert not torch.equal(c['w'], b['w']), what
    finally:
        K.tuning_set('adam_blocks', 2048)


def test_every_refusal_leaves_every_buffer_untouched():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    from t2i_amd import kernels as K
    n, ns = 64, 4
    pool = torch.randn(8 * n, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)
    pool[3 * n:4 * n].abs_()
    before = pool.clone()
    w, g, m, v, s = (pool[i * n:(i + 1) * n] for i in range(5))
    ends = torch.tensor([0, 16, 32, 48, 64, 0], dtype=torch.int64, device=DEV)[1:5]          # 8-byte aligned; + 4 bytes is not
    mult = torch.tensor([[0.5, 2.0], [1.0, 1.0], [3.0, 0.25], [0.1, 0.1]], device=DEV)
    tables = (ends.clone(), mult.clone())
    dec = torch.full((4,), 0.5, device=DEV)
    P = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)     # noqa: E731
    st = K._stream()
    assert ends.data_ptr() % 8 == 0

    def call(w=w, g=g, m=m, v=v, s=s, n=n, e=ends, mu=mult, ns=ns, beta1=0.5, decay=0.5, decay_dev=None, off={}):
        o = lambda k: off.get(k, 0)     # noqa: E731
        return _lib.lib.t2i_adam_tf_slots(P(w, o('w')), P(g, o('g')), P(m, o('m')), P(v, o('v')), P(s, o('s')), n, P(e, o('e')), P(mu, o('mu')), ns,
                                          1e-3, None, beta1, 0.99, 1e-8, 0.5, decay, P(decay_dev), st)

    refused = OrderedDict([
        ('null w', dict(w=None)), ('null g', dict(g=None)), ('null v', dict(v=None)),
        ('null slot_end', dict(e=None)), ('null slot_mult', dict(mu=None)),
        ('m NULL with beta1 != 0', dict(m=None)),
        ('misaligned w', dict(off={'w': 4}, n=n - 4)), ('misaligned g', dict(off={'g': 4}, n=n - 4)), ('misaligned m', dict(off={'m': 8}, n=n - 4)),
        ('misaligned v', dict(off={'v': 12}, n=n - 4)), ('misaligned ema', dict(off={'s': 4}, n=n - 4)),
        ('slot_end not 8-byte aligned', dict(off={'e': 4})),
        ('n == 0', dict(n=0)), ('n < 0', dict(n=-4)), ('n % 4 != 0', dict(n=n - 2)), ('n % 4 != 0 (odd)', dict(n=n - 3)),
        ('n_slots == 0', dict(ns=0)), ('n_slots < 0', dict(ns=-1)), ('n_slots above the cap', dict(ns=K.ADAM_MAX_SLOTS + 1)),
        ('ema is w', dict(s=w)), ('ema is g', dict(s=g)), ('ema is m', dict(s=m)), ('ema is v', dict(s=v)),
        ('ema overlaps the tail of w', dict(s=w, off={'s': 16 * 4})),
        ('ema overlaps the head of w', dict(s=pool[7 * n:], w=pool[7 * n:], off={'w': -16 * 4})),
        ('slot_end inside w', dict(e=w)), ('slot_end inside g', dict(e=g, off={'e': 8})), ('slot_end inside ema', dict(e=s)),
        ('slot_end reaches into w', dict(e=pool[7 * n:], w=pool[7 * n:], off={'e': -16})),
        ('slot_mult inside v', dict(mu=v)), ('slot_mult inside m', dict(mu=m, off={'mu': 16})), ('slot_mult inside w', dict(mu=w)),
        ('decay < 0', dict(decay=-0.1)), ('decay > 1', dict(decay=1.5)), ('decay NaN', dict(decay=float('nan'))),
    ])
    for name, kw in refused.items():
        rc = call(**kw)
        assert rc != 0, name
        assert 't2i_adam_tf_slots' in _lib.lib.t2i_last_error().decode(), name
        torch.cuda.synchronize()
        assert torch.equal(_bits(pool), _bits(before)), name
        assert torch.equal(ends, tables[0]) and torch.equal(_bits(mult), _bits(tables[1])), name
    with pytest.raises(_lib.T2IError, match='ema_decay'):
        K.adam_tf_slots(w, g, m, v, ends, mult, 1e-3, 0.5, 0.99, ema=s, ema_decay=1.5)
    with pytest.raises(TypeError):
        K.adam_tf_slots(w, g, m, v, ends, mult, 1e-3, 0.5, 0.99, ema=s.double())
    with pytest.raises(TypeError):
        K.adam_tf_slots(w, g, m, v, ends.int(), mult, 1e-3, 0.5, 0.99)
    with pytest.raises(TypeError):
        K.adam_tf_slots(w, g, m, v, ends, mult.double(), 1e-3, 0.5, 0.99)
    with pytest.raises(ValueError):
        K.adam_tf_slots(w, g, m, v, ends, mult, 1e-3, 0.5, 0.99, ema=pool[::2][:n])
    with pytest.raises(ValueError):
        K.adam_tf_slots(w, g, m, v, ends, mult[:, :1].expand(4, 2), 1e-3, 0.5, 0.99)
    with pytest.raises(AssertionError):
        K.adam_tf_slots(w, g, m, v, ends, mult, 1e-3, 0.5, 0.99, ema=pool[4 * n:6 * n])
    with pytest.raises(AssertionError):
        K.adam_tf_slots(w, g, m, v, ends[:3], mult, 1e-3, 0.5, 0.99)
    with pytest.raises(AssertionError):
        K.adam_tf_slots(w, g, None, v, ends, mult, 1e-3, 0.5, 0.99)
    assert torch.equal(_bits(pool), _bits(before))
    # the same arguments, accepted: a device decay (or no shadow) makes the host value irrelevant, m NULL goes with beta1 == 0
    assert call(decay=1.5, decay_dev=dec) == 0 and call(m=None, beta1=0.0) == 0 and call(s=None, decay=float('nan')) == 0
    torch.cuda.synchronize()
    assert not torch.equal(pool[:n], before[:n]) and torch.equal(pool[5 * n:], before[5 * n:])
    assert torch.equal(ends, tables[0]) and torch.equal(_bits(mult), _bits(tables[1]))
    # the largest table the entry takes, all ones: t2i_adam_tf's bits
    cap = K.ADAM_MAX_SLOTS
    _, big_ends, mask = _layout((4,) * cap)
    x0 = _inputs(4 * cap, mask, 7)
    a, b = {k: t.clone() for k, t in x0.items()}, {k: t.clone() for k, t in x0.items()}
    K.adam_tf(a['w'], a['g'], a['m'], a['v'], 1e-3, 0.5, 0.99, 1e-8, 0.5)
    K.adam_tf_slots(b['w'], b['g'], b['m'], b['v'], torch.tensor(big_ends, dtype=torch.int64, device=DEV), torch.ones((cap, 2), device=DEV), 1e-3,
                    0.5, 0.99, 1e-8, 0.5)
    torch.cuda.synchronize()
    _same(b, a, True, None, 'n_slots at the cap')
    assert not torch.equal(b['w'], x0['w'])


# ---- the optimizer --------------------------------------------------------------------------------------------------------------
FAN_INS = (8, 27, 72, 144, 4608)


def _eq_arena(seed):
    """Five 64-element kernels w = c * w-hat, w-hat ~ N(0, 1), c = sqrt(2 / fan_in), and a bias that keeps the multiplier 1."""
    from t2i_amd import optim
    gen = torch.Generator(device=DEV).manual_seed(seed)
    variables, scales = OrderedDict(), OrderedDict()
    for i, f in enumerate(FAN_INS):
        c = math.sqrt(2.0 / f)
        variables['net/l%d/w' % i] = (torch.randn(64, generator=gen, device=DEV) * c).requires_grad_(True)
        scales['net/l%d/w' % i] = c
        if i == 2:
            variables['net/l2/b'] = torch.randn(5, generator=gen, device=DEV).requires_grad_(True)
    return optim.Arena(variables), scales


def _clamped_grads(n, count, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(count):
        g = torch.randn(n, generator=gen, device=DEV)
        out.append(torch.where(g < 0, -1.0, 1.0) * g.abs().clamp(min=1e-3))
    return out


def explicit_ref(w0, grads, c, lr, beta1, beta2, eps, gscale):
    """float64: w-hat = w / c, g-hat = c * g, TF-Adam on w-hat, w = c * w-hat."""
    wh = w0.double() / c
    m, v = torch.zeros_like(wh), torch.zeros_like(wh)
    for t, g in enumerate(grads, 1):
        gh = c * (g.double() * gscale)
        m = beta1 * m + (1.0 - beta1) * gh
        v = beta2 * v + (1.0 - beta2) * gh * gh
        lr_t = lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        wh = wh - lr_t * m / (torch.sqrt(v) + eps)
    return c * wh


def _slot_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('lr', [1e-3, 1e-2])
@pytest.mark.parametrize('beta1', [0.0, 0.5])
def test_adam_tf_slot_scales_is_the_explicit_equalized_form(beta1, lr):
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    (a, scales), (a1, _) = _eq_arena(11), _eq_arena(11)
    w0 = a.flat.detach().clone()
    opt = optim.AdamTF(a, beta1, 0.99, slot_scales=scales)
    ones = optim.AdamTF(a1, beta1, 0.99, slot_scales={})          # the all-ones table: plain Adam on w
    grads = _clamped_grads(a.numel, 5, 12)
    for g in grads:
        for arena, o in ((a, opt), (a1, ones)):
            arena.grad.copy_(g)
            o.step(lr, grad_scale=0.5)
    torch.cuda.synchronize()
    for n, (o, k) in a.offsets.items():
        c = scales.get(n, 1.0)
        ref = explicit_ref(w0[o:o + k], [g[o:o + k] for g in grads], c, lr, beta1, 0.99, 1e-8, 0.5)
        err, err1 = _slot_err(a.flat[o:o + k], ref), _slot_err(a1.flat[o:o + k], ref)
        print('%s c=%.4f beta1=%g lr=%g: folded %.2e, all-ones table %.2e' % (n, c, beta1, lr, err, err1))
        assert err <= BOUND, (n, err)
        if n in scales:
            assert err1 > BOUND, (n, err1)           # ... which plain Adam on w does not meet: the check is not vacuous
        else:
            assert err1 <= BOUND, (n, err1)


def test_first_moment_under_the_beta1_zero_fast_path():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd import optim
    a, scales = _eq_arena(21)
    scales['net/l2/b'] = (3.0, 0.25)
    opt = optim.AdamTF(a, 0.0, 0.99, slot_scales=scales)
    assert opt.skip_m
    g0, g1 = _clamped_grads(a.numel, 2, 22)
    a.grad.copy_(g0)
    opt.step(1e-3, grad_scale=0.3)
    w, v = a.flat.detach().clone(), opt.v.clone()
    a.grad.copy_(g1)
    lr_t = opt.prepare(1e-3)
    # the same step with an m buffer (garbage in it: beta1 == 0 does not read it)
    m = torch.full_like(w, 7.0)
    K.adam_tf_slots(w, a.grad, m, v, opt.slot_end, opt.slot_mult, lr_t, 0.0, 0.99, 1e-8, 0.3)
    opt.apply(grad_scale=0.3)
    torch.cuda.synchronize()
    assert torch.equal(_bits(opt.m), _bits(m)) and torch.equal(_bits(a.flat), _bits(w)) and torch.equal(_bits(opt.v), _bits(v))
    plain = g1 * float(np.float32(0.3))
    o, k = a.offsets['net/l4/w']
    assert not torch.equal(opt.m[o:o + k], plain[o:o + k])                 # (not the unscaled product)
    a.zero_grad()                                                          # an eager zero_grad keeps the moment
    assert torch.equal(_bits(opt.m), _bits(m))


@pytest.mark.parametrize('shadow', [False, True])
def test_captured_apply_replays_with_new_gradients_and_step_size(shadow):
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    from t2i_amd.graphs import capture_mode
    twins = []
    for captured in (False, True):
        a, scales = _eq_arena(31)
        opt = optim.AdamTF(a, 0.0, 0.99, ema_decay=0.9 if shadow else None, slot_scales=scales)
        twins.append((a, opt, captured))
    grads = _clamped_grads(twins[0][0].numel, 4, 32)
    w0 = twins[0][0].flat.detach().clone()
    for a, opt, captured in twins:
        a.grad.copy_(grads[0])                    # one eager step first (it also loads the kernel before any capture)
        opt.step(1e-3)
        if captured:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode=capture_mode()):
                opt.apply(grad_scale=0.5)
        for i in range(3):
            a.grad.copy_(grads[1 + i])
            opt.prepare(1e-3 * (1 + i))           # a new lr_t every step: the bias correction and the step size
            if captured:
                graph.replay()
            else:
                opt.apply(grad_scale=0.5)
        torch.cuda.synchronize()
    (a0, o0, _), (a1, o1, _) = twins
    assert o0.t == o1.t == 4
    assert torch.equal(_bits(a1.flat), _bits(a0.flat)) and torch.equal(_bits(o1.v), _bits(o0.v)) and not torch.equal(a0.flat, w0)
    if shadow:
        assert torch.equal(_bits(o1.ema), _bits(o0.ema)) and not torch.equal(o1.ema, a1.flat)
    else:
        assert o0.ema is None and o1.ema is None


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _make_golden():
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(ROOT, 'tests', 'golden', 'make_golden.py'))
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    return mg


def _c(name, v):
    if name.endswith('/weights'):
        return math.sqrt(2.0 / (v.shape[0] * v.shape[1] * v.shape[2]))
    if name.endswith('/kernel'):
        return math.sqrt(2.0 / v.shape[0])
    return 1.0


def test_pggan_equalized_step_is_the_explicit_form():
    """Stage 3 with the transition at the golden parameters: the flag changes no gradient, and both updates are the float64 explicit
    form computed from the arena the launch read."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    mg = _make_golden()
    gs = np.load(os.path.join(ROOT, 'tests', 'golden', 'pggan_tiny.npz'))
    t = mg.PGGAN_TINY
    assert dict(fmap_base=t['base'], fmap_max=t['cap'], z_dim=t['z_dim'], embed_dim=t['embed_dim'], compr_embed_dim=t['compressed']) == TINY
    f = {k[len('feed/'):]: torch.tensor(gs[k], dtype=torch.float32, device=DEV) for k in gs.files if k.startswith('feed/')}
    feed = {'x': f['x'], 'x_mismatch': f['x_mismatch'], 'cond': f['cond'], 'z': f['z'], 'eps_graph': f['eps'],
            'ca_noise_d': f['ca_noise_d'], 'ca_noise_g': f['ca_noise_g']}
    from t2i_amd import scope as S
    models = []
    for kw in ({}, dict(equalized_lr=True, adam_lr=1e-2)):
        m = PGGAN(t['batch'], mg.PGGAN_STEPS, None, None, None, None, None, mg.PGGAN_STAGE, True, device=DEV, **TINY, **kw)
        m.store.load({k[len('param/'):]: gs[k] for k in gs.files if k.startswith('param/')})
        m.set_alpha(mg.PGGAN_IDX / float(mg.PGGAN_STEPS))
        models.append(m)
    off, on = models
    assert mg.PGGAN_STAGE == 3 and on.adam_lr == 1e-2 and off.adam_lr == 2e-6
    for m in models:
        S.set_default_store(m.store)
        m.d_losses(feed)
    torch.cuda.synchronize()
    assert torch.equal(_bits(on.d_arena.grad), _bits(off.d_arena.grad)) and float(on.d_arena.grad.abs().max()) > 0
    for m in models:
        S.set_default_store(m.store)
        m.g_losses(feed)
    torch.cuda.synchronize()
    assert torch.equal(_bits(on.g_arena.grad), _bits(off.g_arena.grad)) and float(on.g_arena.grad.abs().max()) > 0
    S.set_default_store(on.store)
    scaled = differs = 0
    for arena, opt in ((on.d_arena, on.D_optimizer), (on.g_arena, on.G_optimizer)):
        w0, g = arena.flat.detach().clone(), arena.grad.detach().clone()
        opt.prepare(on.adam_lr)
        opt.apply()
        torch.cuda.synchronize()
        assert torch.equal(_bits(arena.grad), _bits(g))
        for n, v in arena.vars.items():
            o, k = arena.offsets[n]
            c = _c(n, v)
            scaled += c != 1.0
            ref = explicit_ref(w0[o:o + k], [g[o:o + k]], c, on.adam_lr, 0.0, 0.99, 1e-8, 1.0)
            err = _slot_err(arena.flat[o:o + k], ref)
            assert err <= BOUND, (n, c, err)
            if c != 1.0:
                plain = explicit_ref(w0[o:o + k], [g[o:o + k]], 1.0, on.adam_lr, 0.0, 0.99, 1e-8, 1.0)
                differs += _slot_err(arena.flat[o:o + k], plain) > BOUND             # (not plain Adam on w)
        assert not torch.equal(arena.flat, w0)
    assert scaled == 23 and differs >= 20, (scaled, differs)      # 13 generator and 10 critic kernels at stage 3 with the transition


def _feeds(count, size, batch):
    g = torch.Generator(device=DEV).manual_seed(2)
    B, t = batch, TINY
    return [{'x': torch.rand((B, size, size, 3), generator=g, device=DEV) * 2 - 1, 'x_mismatch': torch.rand((B, size, size, 3), generator=g, device=DEV) * 2 - 1,
             'cond': torch.randn((B, t['embed_dim']), generator=g, device=DEV), 'z': torch.randn((B, t['z_dim']), generator=g, device=DEV),
             'eps_graph': torch.rand((B,), generator=g, device=DEV),
             'ca_noise_d': torch.randn((B, t['compr_embed_dim']), generator=g, device=DEV).clamp(-2, 2),
             'ca_noise_g': torch.randn((B, t['compr_embed_dim']), generator=g, device=DEV).clamp(-2, 2)} for _ in range(count)]


def test_pggan_graph_replay_with_every_option_matches_eager():
    """PGGAN(equalized_lr, g_ema, critic_mbstd) at stage 2 with the transition: iterations replayed as hipGraphs == eager launches, bit for
    bit, over 3 iterations: both arenas and the generator's shadow."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    feeds = _feeds(4, 8, 8)
    states = []
    for use_graphs in (False, True):
        m = PGGAN(8, 10, None, None, None, None, None, 2, True, device=DEV, seed=4, equalized_lr=True, adam_lr=1e-3, g_ema=0.999, critic_mbstd=4,
                  **TINY)
        assert m.D_optimizer.slot_end is not None and m.G_optimizer.slot_end is not None and m.mbstd_group == 4
        w0 = m.g_arena.flat.detach().clone()
        m.iteration(1, feeds[0])
        if use_graphs:
            m.enable_graphs(feeds[0])
        outs = [m.iteration(2 + 2 * i, feeds[1 + i]) for i in range(3)]
        torch.cuda.synchronize()
        states.append((m.d_arena.flat.detach().clone(), m.g_arena.flat.detach().clone(), m.G_optimizer.ema.clone(),
                       float(outs[-1]['d']['D_loss']), float(outs[-1]['g']['G_loss'])))
        assert not torch.equal(states[-1][1], w0) and not torch.equal(states[-1][2], states[-1][1]) and not torch.equal(states[-1][2], w0)
    (d0, g0, s0, dl0, gl0), (d1, g1, s1, dl1, gl1) = states
    assert torch.equal(_bits(d0), _bits(d1)) and torch.equal(_bits(g0), _bits(g1)) and torch.equal(_bits(s0), _bits(s1))
    assert dl0 == dl1 and gl0 == gl1 and bool(torch.isfinite(d0).all()) and bool(torch.isfinite(g0).all())


# ---- one command end to end -----------------------------------------------------------------------------------------------------
def test_train_pggan_main_with_the_flags(tmp_path):
    """Stages 1 -> 2t -> 2 on synthetic data: every entry restores the previous one; the checkpoints hold what they hold without the flag
    (plain weights under the same keys)."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan import train_pggan as TP
    from t2i_amd.models.pggan.pggan import PGGAN
    out = str(tmp_path / 'run')
    records = TP.main(['--out', out, '--equalized-lr', '--lr', '1e-3', '--g-ema', '0.999', '--iters', '3', '--first', '0', '--last', '2'])
    assert [(r['stage'], r['trans']) for r in records] == [(1, False), (2, True), (2, False)]
    assert records[0]['restored'] is None
    ck = lambda k: os.path.join(out, 'checkpoints', 'stage%d/' % k)       # noqa: E731
    names = {}
    for k in (1, 2):           # the keys of a stage's checkpoint, from a model built without the flag
        plain = PGGAN(16, 100, None, None, None, None, None, k, False, device='cpu')
        saved = plain.get_variables_up_to_stage(k)
        names[k] = sorted(saved + [n + EMA for n in saved if n.startswith('g_net/')])
        shapes = {n: tuple(plain.store.vars[n].shape) for n in saved}
        z = np.load(os.path.join(ck(k), 'model-2.npz'))
        assert sorted(z.files) == names[k]
        for n in z.files:
            assert z[n].dtype == np.float32 and z[n].shape == shapes[n[:-len(EMA)] if n.endswith(EMA) else n], n
            assert np.isfinite(z[n]).all(), n
        assert any(not np.array_equal(z[n], z[n + EMA]) for n in saved if n.startswith('g_net/'))
        del plain
    plain_keys = lambda k: [n for n in names[k] if not n.endswith(EMA)]     # noqa: E731
    d1, step1, vars1 = records[1]['restored']
    assert os.path.samefile(d1, ck(1)) and step1 == 2 and sorted(vars1) == plain_keys(1)
    d2, step2, vars2 = records[2]['restored']
    assert os.path.samefile(d2, ck(2)) and step2 == 2 and sorted(vars2) == plain_keys(2)
