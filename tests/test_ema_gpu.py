"""The generator weight EMA on the GPU: t2i_adam_tf_ema against t2i_adam_tf and a step-by-step fp32
restatement of the shadow, bit for bit, with t2i_adam_tf itself held to the float64 oracle; its refusals; AdamTF.apply under graph replay; PGGAN(g_ema=...) eager and replayed; the
stage 1 -> 2t -> 2 schedule with shadows in the checkpoints; visualize_pggan.py --ema."""
import ctypes
import math
import os
import random
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_kernels_gpu import relerr  # noqa: E402
from test_pggan_real_gpu import _cfg, data  # noqa: E402,F401

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
EMA = '/ExponentialMovingAverage'
TINY = dict(fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)      # tests/test_pggan.py's widths
BATCH = 3
ADAM_BOUND = 1e-6                  # the project's bound for an Adam launch (test_adam_golden)


def _bits(t):
    return t.detach().reshape(-1).view(torch.int32)


def shadow_ref(s, w_new, decay):
    """s - (1 - d) * (s - w_new) in fp32, one rounded operation at a time, on the host; 1 - d is formed in fp32."""
    s, w_new = s.detach().cpu().numpy().astype(np.float32), w_new.detach().cpu().numpy().astype(np.float32)
    omd = np.float32(1.0) - np.float32(decay)
    diff = (s - w_new).astype(np.float32)
    prod = (omd * diff).astype(np.float32)
    return torch.from_numpy((s - prod).astype(np.float32))


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _inputs(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda: torch.randn(n, generator=g, device=DEV)       # noqa: E731
    return dict(w=r(), g=r() * 3.0, m=r() * 0.1, v=r().abs() * 0.01, s=r())


def _oracle_step(x, lr_t, beta1, beta2, gscale):
    """oracle.np_ops.adam_tf in float64 on the inputs of one launch: the fp32 step size and the scaled gradient as the kernel sees them
    (gscale is a power of two: the product is exact).  At t = 1 the oracle's lr_t is lr * sqrt(1 - beta2) / (1 - beta1)."""
    from oracle import np_ops as O
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)       # noqa: E731
    lr = float(np.float32(lr_t)) * (1.0 - beta1) / math.sqrt(1.0 - beta2)
    return O.adam_tf(f64(x['w']), f64(x['g']) * gscale, f64(x['m']) if beta1 else np.zeros(x['w'].numel()), f64(x['v']), 1, lr, beta1, beta2)


@pytest.mark.parametrize('beta1', [0.0, 0.5])
@pytest.mark.parametrize('n', [1, 3, 4, 1027, 4101])
def test_fused_launch_equals_adam_tf_and_the_host_recursion(n, beta1):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    if n == 4101:
        K.tuning_set('adam_blocks', 2)            # 1026 quads over 512 threads: the grid-stride loop iterates
    try:
        case = 0
        for lr_dev in (False, True):
            for decay in (0.5, 0.999, 1.0):
                for decay_dev in (False, True):
                    case += 1
                    x = _inputs(n, 100 * n + case)
                    lr_t = 3e-3
                    lr_buf = torch.full((4,), lr_t, device=DEV) if lr_dev else None
                    d_buf = torch.full((4,), decay, device=DEV) if decay_dev else None
                    w0, m0, v0 = x['w'].clone(), (x['m'].clone() if beta1 else None), x['v'].clone()
                    K.adam_tf(w0, x['g'], m0, v0, 0.0 if lr_dev else lr_t, beta1, 0.99, 1e-8, 0.5, lr_t_dev=lr_buf)
                    w1, m1, v1, s1 = x['w'].clone(), (x['m'].clone() if beta1 else None), x['v'].clone(), x['s'].clone()
                    # with a device scalar the host value is ignored: pass one that would be refused / wrong
                    K.adam_tf_ema(w1, x['g'], m1, v1, s1, 0.0 if lr_dev else lr_t, beta1, 0.99, 1e-8, 0.5,
                                  7.0 if decay_dev else decay, lr_t_dev=lr_buf, ema_decay_dev=d_buf)
                    torch.cuda.synchronize()
                    what = (n, beta1, lr_dev, decay, decay_dev)
                    assert not torch.equal(w0, x['w']), what
                    # the plain launch against the float64 oracle: the fused launches below are held to its bits
                    w_ref, m_ref, v_ref = _oracle_step(x, lr_t, beta1, 0.99, 0.5)
                    errs = (relerr(w0, w_ref), relerr(v0, v_ref), relerr(m0, m_ref) if beta1 else 0.0)
                    print('adam_tf vs float64 oracle %s: w %.2e v %.2e m %.2e' % ((what,) + errs))
                    assert max(errs) <= ADAM_BOUND, (what, errs)
                    assert torch.equal(_bits(w1), _bits(w0)) and torch.equal(_bits(v1), _bits(v0)), what
                    if beta1:
                        assert torch.equal(_bits(m1), _bits(m0)), what
                    assert torch.equal(_bits(s1.cpu()), _bits(shadow_ref(x['s'], w0, decay))), what
                    if decay == 1.0:
                        assert torch.equal(_bits(s1), _bits(x['s'])), what
                    else:
                        assert not torch.equal(s1, x['s']), what
    finally:
        if n == 4101:
            K.tuning_set('adam_blocks', 2048)


def test_every_refusal_leaves_every_buffer_untouched():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    from t2i_amd import kernels as K
    n = 64
    pool = torch.randn(8 * n, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)
    pool[3 * n:4 * n].abs_()
    before = pool.clone()
    w, g, m, v, s = (pool[i * n:(i + 1) * n] for i in range(5))
    dec = torch.full((4,), 0.5, device=DEV)
    P = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)     # noqa: E731
    st = K._stream()

    def call(w=w, g=g, m=m, v=v, s=s, n=n, beta1=0.5, decay=0.5, decay_dev=None, s_off=0, w_off=0):
        return _lib.lib.t2i_adam_tf_ema(P(w, w_off), P(g), P(m), P(v), P(s, s_off), n, 1e-3, None, beta1, 0.99, 1e-8, 0.5, decay, P(decay_dev), st)

    refused = OrderedDict([
        ('null ema', dict(s=None)),
        ('misaligned ema', dict(s_off=4, n=n - 4)),
        ('ema is w', dict(s=w)), ('ema is g', dict(s=g)), ('ema is m', dict(s=m)), ('ema is v', dict(s=v)),
        ('ema overlaps the tail of w', dict(s=w, s_off=16 * 4)),          # [w + 16, w + 16 + n) reaches into g as well
        ('ema overlaps the head of w', dict(s=pool[7 * n:], w=pool[7 * n:], w_off=-16 * 4)),
        ('n == 0', dict(n=0)), ('n < 0', dict(n=-4)),
        ('decay < 0', dict(decay=-0.1)), ('decay > 1', dict(decay=1.5)), ('decay NaN', dict(decay=float('nan'))),
        ('null w', dict(w=None)), ('null g', dict(g=None)), ('null v', dict(v=None)),
        ('m NULL with beta1 != 0', dict(m=None)),
        ('misaligned w', dict(w_off=4, n=n - 4)),
    ])
    for name, kw in refused.items():
        rc = call(**kw)
        assert rc != 0, name
        assert 't2i_adam_tf_ema' in _lib.lib.t2i_last_error().decode(), name
        torch.cuda.synchronize()
        assert torch.equal(_bits(pool), _bits(before)), name
    with pytest.raises(_lib.T2IError, match='ema_decay'):
        K.adam_tf_ema(w, g, m, v, s, 1e-3, 0.5, 0.99, ema_decay=1.5)
    with pytest.raises(TypeError):
        K.adam_tf_ema(w, g, m, v, s.double(), 1e-3, 0.5, 0.99)
    with pytest.raises(ValueError):
        K.adam_tf_ema(w, g, m, v, pool[::2][:n], 1e-3, 0.5, 0.99)
    with pytest.raises(AssertionError):
        K.adam_tf_ema(w, g, m, v, pool[4 * n:6 * n], 1e-3, 0.5, 0.99)
    assert torch.equal(_bits(pool), _bits(before))
    # the same arguments, accepted: a device decay makes the host value irrelevant, m NULL goes with beta1 == 0
    assert call(decay=1.5, decay_dev=dec) == 0 and call(m=None, beta1=0.0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(pool[:n], before[:n]) and torch.equal(pool[5 * n:], before[5 * n:])


# ---- the optimizer under graph replay --------------------------------------------------------------------------------------------
def _gpu_arena(seed):
    from t2i_amd import optim
    gen = torch.Generator(device=DEV).manual_seed(seed)
    shapes = OrderedDict([('g_net/a/w', (3, 3, 8, 16)), ('g_net/a/b', (16,)), ('g_net/b/w', (37, 5)), ('g_net/b/b', (5,))])
    return optim.Arena(OrderedDict((n, torch.randn(s, generator=gen, device=DEV).requires_grad_(True)) for n, s in shapes.items()))


def test_captured_apply_replays_with_a_changed_decay():
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    from t2i_amd.graphs import capture_mode
    gen = torch.Generator(device=DEV).manual_seed(9)
    twins = []
    for captured in (False, True):
        a = _gpu_arena(3)
        opt = optim.AdamTF(a, 0.0, 0.99, ema_decay=0.9)
        assert torch.equal(opt.ema, a.flat)
        twins.append((a, opt, captured))
    grads = [torch.randn(twins[0][0].numel, generator=gen, device=DEV) for _ in range(4)]
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
            opt.prepare(1e-3)
            if i == 1:
                opt.set_ema_decay(0.25)
            if captured:
                graph.replay()
            else:
                opt.apply(grad_scale=0.5)
        torch.cuda.synchronize()
    (a0, o0, _), (a1, o1, _) = twins
    assert o0.t == o1.t == 4
    assert torch.equal(_bits(a1.flat), _bits(a0.flat)) and torch.equal(_bits(o1.v), _bits(o0.v))
    assert torch.equal(_bits(o1.ema), _bits(o0.ema)) and not torch.equal(o1.ema, a1.flat)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _feeds(count, size):
    g = torch.Generator(device=DEV).manual_seed(2)
    B, t = BATCH, TINY
    return [{'x': torch.rand((B, size, size, 3), generator=g, device=DEV) * 2 - 1, 'x_mismatch': torch.rand((B, size, size, 3), generator=g, device=DEV) * 2 - 1,
             'cond': torch.randn((B, t['embed_dim']), generator=g, device=DEV), 'z': torch.randn((B, t['z_dim']), generator=g, device=DEV),
             'eps_graph': torch.rand((B,), generator=g, device=DEV),
             'ca_noise_d': torch.randn((B, t['compr_embed_dim']), generator=g, device=DEV).clamp(-2, 2),
             'ca_noise_g': torch.randn((B, t['compr_embed_dim']), generator=g, device=DEV).clamp(-2, 2)} for _ in range(count)]


@pytest.fixture(scope='module')
def model_runs():
    """Stage 2 with the fade-in branch, three iterations (the first eager, then eager or replayed), with and without g_ema."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    feeds = _feeds(3, 8)
    runs = {}
    for graphs in (False, True):
        for g_ema in (None, 0.5):
            m = PGGAN(BATCH, 10, None, None, None, None, None, 2, True, device=DEV, seed=4, g_ema=g_ema, **TINY)
            snaps = [m.g_arena.flat.detach().clone()]
            for i in range(3):
                if i == 1 and graphs:
                    m.enable_graphs(feeds[0])
                m.iteration(1 + i, feeds[i])
                torch.cuda.synchronize()
                snaps.append(m.g_arena.flat.detach().clone())
            runs[graphs, g_ema] = (m, snaps)
    return runs


@pytest.mark.parametrize('graphs', [False, True])
def test_model_shadow_is_the_host_recursion_and_the_step_is_unchanged(model_runs, graphs):
    plain, _ = model_runs[graphs, None]
    m, snaps = model_runs[graphs, 0.5]
    assert plain.G_optimizer.ema is None
    assert torch.equal(_bits(m.d_arena.flat), _bits(plain.d_arena.flat)) and torch.equal(_bits(m.g_arena.flat), _bits(plain.g_arena.flat))
    assert not torch.equal(snaps[0], snaps[3])
    s = snaps[0].cpu()
    for w in snaps[1:]:
        s = shadow_ref(s, w, 0.5)
    assert torch.equal(_bits(m.G_optimizer.ema.cpu()), _bits(s))
    assert m.D_optimizer.ema is None


def test_ema_weights_swaps_and_restores(model_runs, monkeypatch):
    from t2i_amd import scope as S
    m, _ = model_runs[False, 0.5]
    S.set_default_store(m.store)                  # (the fixture built other models after this one)
    flat, ema = m.g_arena.flat.detach().clone(), m.G_optimizer.ema.clone()
    assert not torch.equal(flat, ema)
    g = torch.Generator(device=DEV).manual_seed(8)
    z, cond = torch.randn((BATCH, TINY['z_dim']), generator=g, device=DEV), torch.randn((BATCH, TINY['embed_dim']), generator=g, device=DEV)
    m.set_alpha(0.5)
    torch.manual_seed(0)
    outside = m.sampler(z, cond).clone()
    with m.ema_weights() as same:
        assert same is m
        assert torch.equal(_bits(m.g_arena.flat), _bits(ema)) and torch.equal(_bits(m.G_optimizer.ema), _bits(flat))
        torch.manual_seed(0)
        inside = m.sampler(z, cond).clone()
    assert torch.equal(_bits(m.g_arena.flat), _bits(flat)) and torch.equal(_bits(m.G_optimizer.ema), _bits(ema))
    torch.manual_seed(0)
    assert torch.equal(m.sampler(z, cond), outside)
    assert inside.shape == outside.shape and not torch.equal(inside, outside)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)      # what a capture in progress answers
    with pytest.raises(RuntimeError, match='capture'):
        with m.ema_weights():
            pass
    monkeypatch.undo()
    assert torch.equal(_bits(m.g_arena.flat), _bits(flat)) and torch.equal(_bits(m.G_optimizer.ema), _bits(ema))


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
def _dataset(size):
    from t2i_amd.data import SyntheticTextDataset
    from t2i_amd.utils.config import AttrDict
    dcfg = AttrDict({'MODEL': {'Z_DIM': TINY['z_dim'], 'OUTPUT_SIZE': size, 'EMBED_DIM': TINY['embed_dim'], 'IMAGE_SHAPE': {'W': size, 'H': size, 'D': 3}},
                     'TRAIN': {'BATCH_SIZE': BATCH}})
    return SyntheticTextDataset(dcfg, DEV, seed=5, num_examples=512)              # 64 test examples: one sample grid


def test_schedule_carries_the_shadows_through_the_stages(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan import eval_pggan as E
    from t2i_amd.models.pggan.pggan import PGGAN
    from t2i_amd.utils.config import AttrDict
    root = str(tmp_path)
    ck = lambda k: os.path.join(root, 'ckpt', 'stage%d/' % k)       # noqa: E731
    sp = lambda name: os.path.join(root, 'samples', name) + '/'     # noqa: E731
    quiet = lambda s: None                                          # noqa: E731

    def stage(k, trans, read, sub):
        return PGGAN(BATCH, 100, ck(k), ck(read), _dataset(4 * 2 ** (k - 1)), sp(sub), None, k, trans, device=DEV, seed=10 + k, g_ema=0.5, **TINY)

    def check_file(m, k):
        z = np.load(os.path.join(ck(k), 'model-3.npz'))
        saved = m.get_variables_up_to_stage(k)
        assert sorted(z.files) == sorted(saved + [n + EMA for n in saved if n.startswith('g_net/')])
        assert sorted(f for f in os.listdir(m.sample_path) if f.endswith('.png')) == ['train_00_0003.png', 'train_ema_00_0003.png']
        a, ema = m.g_arena, m.G_optimizer.ema
        for n in saved:
            if n.startswith('g_net/'):                  # written from the state the run ended in
                o, c = a.offsets[n]
                assert np.array_equal(z[n + EMA].reshape(-1).view(np.int32), _bits(ema[o:o + c]).cpu().numpy()), n
                assert np.array_equal(z[n].reshape(-1).view(np.int32), _bits(a.flat[o:o + c]).cpu().numpy()), n
        assert any(not np.array_equal(z[n], z[n + EMA]) for n in saved if n.startswith('g_net/'))
        return z

    m1 = stage(1, False, 1, 'stage1')
    m1.train(max_steps=4, log=quiet, side_effects=True, final_sample=True)
    z1 = check_file(m1, 1)

    # 2t: the restore alone first (max_steps=1: no iteration, nothing written)
    m2 = stage(2, True, 1, 'stage_t2')
    init = m2.g_arena.flat.detach().clone()
    assert m2.train(max_steps=1, log=quiet, side_effects=True) is None and not os.path.exists(ck(2))
    restored = set(m2.restored[2])
    assert restored == set(z1.files) - {f for f in z1.files if f.endswith(EMA)}
    a, ema = m2.g_arena, m2.G_optimizer.ema
    new = [n for n in a.names if n not in restored]
    assert new and any('/conv_stage_1/' in n for n in new) and any('/rgb_stage_1/' in n for n in new)
    for n in a.names:
        o, c = a.offsets[n]
        if n in restored:                               # the file's variable and the file's shadow
            assert np.array_equal(z1[n].reshape(-1).view(np.int32), _bits(a.flat[o:o + c]).cpu().numpy()), n
            assert np.array_equal(z1[n + EMA].reshape(-1).view(np.int32), _bits(ema[o:o + c]).cpu().numpy()), n
        else:                                           # a new layer: its fresh initial values, in both
            assert torch.equal(_bits(a.flat[o:o + c]), _bits(init[o:o + c])) and torch.equal(_bits(ema[o:o + c]), _bits(init[o:o + c])), n
    m2.train(max_steps=4, log=quiet, side_effects=True, final_sample=True)
    check_file(m2, 2)

    m3 = stage(2, False, 2, 'stage2')
    m3.train(max_steps=4, log=quiet, side_effects=True, final_sample=True)
    z3 = check_file(m3, 2)
    assert m3.restored[1] == 3

    # the averaged generator at save time == the checkpoint read with ema=True
    g = torch.Generator(device=DEV).manual_seed(21)
    z, cond = torch.randn((BATCH, TINY['z_dim']), generator=g, device=DEV), torch.randn((BATCH, TINY['embed_dim']), generator=g, device=DEV)
    with torch.no_grad():
        live = torch.clamp(m3.generator(z, cond, stages=2, t=False, reuse=True, cond_noise=False)[0].float(), -1.0, 1.0).clone()
        with m3.ema_weights():
            want = torch.clamp(m3.generator(z, cond, stages=2, t=False, reuse=True, cond_noise=False)[0].float(), -1.0, 1.0).clone()
    cfg = AttrDict({'CHECKPOINT_DIR': os.path.join(root, 'ckpt')})
    r = E.stage_model(cfg, 2, BATCH, None, DEV, **TINY)
    E.restore_generator(r, ema=True)
    for n, v in r.store.vars.items():
        assert np.array_equal(z3[n + EMA].view(np.int32), _bits(v).cpu().numpy().reshape(v.shape)), n
    assert torch.equal(E.generate(r, z, cond, cond_noise=False), want)
    E.restore_generator(r)
    assert torch.equal(E.generate(r, z, cond, cond_noise=False), live) and not torch.equal(live, want)


# ---- one command end to end -----------------------------------------------------------------------------------------------------
def test_visualize_pggan_reads_the_shadows(data):  # noqa: F811
    """tests/test_pggan_real_gpu.py's narrow stage-4 generator, its checkpoint written with shadows: --ema draws every sheet from
    them; a checkpoint without shadows cannot be read that way."""
    import t2i_amd  # noqa: F401
    from t2i_amd import optim
    from t2i_amd.models.pggan import visualize_pggan as VP
    from t2i_amd.models.pggan.eval_pggan import load_stage_dataset, stage_model
    from t2i_amd.utils.config import config_from_yaml
    from t2i_amd.utils.saver import Saver, save
    from PIL import Image
    widths = dict(fmap_base=64, fmap_max=32)
    paths = {}
    for kind in ('ema', 'plain'):
        path, _ = _cfg(data['root'], data['dir'], ckpt='ckpt_' + kind)
        cfg = config_from_yaml(path)
        ds = load_stage_dataset(cfg, 4, DEV)
        m = stage_model(cfg, 4, 64, ds, DEV, **widths)
        shadows = None
        if kind == 'ema':
            opt = optim.AdamTF(optim.Arena(m.store.trainable_variables('g_net')), 0.0, 0.99, ema_decay=0.999)
            with torch.no_grad():
                opt.ema.mul_(0.5)
            shadows = [opt]
        saved = save(Saver(m.store, var_list=['g_net'], shadows=shadows), None, m.check_dir_read, 1)
        assert any(f.endswith(EMA) for f in np.load(saved).files) == (kind == 'ema')
        paths[kind] = (path, cfg)
        del m
    path, cfg = paths['ema']
    np.random.seed(6); random.seed(6); torch.manual_seed(6)
    out = VP.main(['--cfg', path, '--interp', '1', '--stage', '4', '--ema'], **widths)
    vis = os.path.join(cfg.SAMPLE_DIR, 'flowers_visual')
    for kind, n, shape in (('z_interp', 1, (288, 256, 3)), ('cond_interp', 1, (320, 256, 3)), ('cap', 1, (288, 256, 3)),
                           ('special_cap', 3, (288, 256, 3))):
        assert len(out[kind]) == n and all(s.shape == shape for s in out[kind]), kind
        names = sorted(f for f in os.listdir(os.path.join(vis, kind)) if f.endswith('.png'))
        assert names == sorted('%s%d.png' % ('cap' if kind == 'special_cap' else kind, i) for i in range(n))
        assert np.asarray(Image.open(os.path.join(vis, kind, names[0]))).shape == shape
    with pytest.raises(KeyError) as e:
        VP.main(['--cfg', paths['plain'][0], '--interp', '1', '--stage', '4', '--ema'], **widths)
    assert EMA in str(e.value) and 'trained without EMA' in str(e.value)
