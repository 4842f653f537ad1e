"""Spectral normalisation, host side (no GPU): the float64 restatement (tests/sn_cases.py) against autograd and numpy's SVD, the slot
table optim.SpectralNorm builds, every refusal in Python and every refusal of the two C entries (ctypes with fabricated pointers: no
launch), the declarations, and PGGAN's critic_sn argument."""
import ctypes
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


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SC.NORMALISED)
def test_restated_gradient_equals_autograd(name):
    """Autograd through raw / (v^T raw u), u and v constants, against grad_raw: 1e-12 of the tensor's scale."""
    shape = SC.ARENA[name]
    R, C = SC.matrix_shape(shape)
    rng = np.random.default_rng(7)
    raw = SC.arena_values()[name].astype(np.float64)
    u, v, sigma = SC.iterate(raw.reshape(R, C), SC.first_u(C, rng), 3)
    G = rng.standard_normal(shape)
    rt = torch.tensor(raw, requires_grad=True)
    sig = torch.tensor(v) @ rt.reshape(R, C) @ torch.tensor(u)
    assert abs(float(sig.detach()) - sigma) <= 1e-12 * sigma                          # sigma = |M^T v| = v^T M u with the new u and v
    (rt / sig * torch.tensor(G)).sum().backward()
    W = SC.normalised(raw, sigma)
    assert SC.relerr(SC.grad_raw(G, W, u, v, sigma), rt.grad.numpy()) <= 1e-12


def test_restated_sigma_reaches_the_top_singular_value():
    """After the 15 warm-up iterations from the file's seed, sigma lies in [0.95, 1 + 1e-9] sigma_top for every matrix of the arena."""
    rng = np.random.default_rng(SC.SEED + 2)
    vals = SC.arena_values()
    for name in SC.NORMALISED:
        R, C = SC.matrix_shape(SC.ARENA[name])
        M = vals[name].astype(np.float64).reshape(R, C)
        _, _, sigma = SC.iterate(M, SC.first_u(C, rng), SC.WARMUP)
        top = float(np.linalg.svd(M, compute_uv=False)[0])
        print('%s [%d, %d]: sigma / sigma_top = %.6f' % (name, R, C, sigma / top))
        assert 0.95 * top <= sigma <= (1.0 + 1e-9) * top, (name, sigma, top)


def test_restated_adam_is_the_docstring_formula():
    w, g, v = np.array([1.0, -2.0]), np.array([0.5, -0.25]), np.array([0.01, 0.04])
    w1, m1, v1 = SC.adam_tf(w, g, v, t=3, lr=1e-3, beta1=0.5, beta2=0.9, m=np.array([0.1, 0.2]))
    lr_t = 1e-3 * np.sqrt(1 - 0.9 ** 3) / (1 - 0.5 ** 3)
    m = 0.5 * np.array([0.1, 0.2]) + 0.5 * g
    vv = 0.9 * v + 0.1 * g * g
    assert np.allclose(m1, m, rtol=0, atol=1e-16) and np.allclose(v1, vv, rtol=0, atol=1e-16)
    assert np.allclose(w1, w - lr_t * m / (np.sqrt(vv) + 1e-8), rtol=0, atol=1e-16)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _arena(values=None, names=None):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd import optim
    values = SC.arena_values() if values is None else values
    vs = OrderedDict((n, torch.tensor(values[n]).requires_grad_()) for n in (names or values))
    with K.dry_run():
        return optim.Arena(vs)


def test_the_table_spectral_norm_builds():
    from t2i_amd import kernels as K
    from t2i_amd import optim
    arena = _arena()
    with K.dry_run():
        sn = optim.SpectralNorm(arena, list(reversed(SC.NORMALISED)), seed=3, warmup=2)      # any order in: arena order in the table
    assert sn.names == SC.NORMALISED
    host = sn.table.host
    assert host.dtype == np.int64 and host.shape == (len(SC.NORMALISED), K.SPECTRAL_COLS) and tuple(sn.table.dev.shape) == host.shape
    assert np.array_equal(sn.table.dev.numpy(), host)
    uo = vo = po = 0
    max_items = 1
    for row, n in zip(host, SC.NORMALISED):
        R, C = SC.matrix_shape(SC.ARENA[n])
        rb, items = K.spectral_items(R, C)
        assert tuple(row) == (arena.offsets[n][0], R, C, uo, vo, po, 1), n
        assert uo % 4 == 0 and vo % 4 == 0 and po % 4 == 0 and rb * C <= 8192 and rb <= 2048 and (items - 1) * rb < R <= items * rb
        uo, vo, po, max_items = uo + (C + 3) // 4 * 4, vo + (R + 3) // 4 * 4, po + (items * C + items + (C + 63) // 64 + 3) // 4 * 4, max(max_items, items)
    assert (sn.table.nu, sn.table.nv, sn.table.part_floats, sn.table.max_items, sn.table.numel) == (uo, vo, po, max_items, arena.numel)
    assert K.spectral_items(2048, 64) == (128, 16) and K.spectral_items(576, 128) == (64, 9) and K.spectral_items(40, 1) == (40, 1)
    assert K.spectral_items(8192, 1) == (2048, 4) and K.spectral_items(5, 10000) == (1, 5) and max_items == 16
    assert sn.u.numel() == uo and sn.v.numel() == vo and sn.sigma.numel() == len(SC.NORMALISED) and sn.ws.numel() == sn.table.ws_floats >= po
    assert torch.equal(sn.raw, arena.flat) and sn.raw.data_ptr() != arena.flat.data_ptr()
    # u: N(0, 1) from the seed on the CPU, normalised, zeros in the padding; the same for the same seed, another for another
    gen = torch.Generator().manual_seed(3)
    for row in host:
        C, o = int(row[2]), int(row[3])
        d = torch.randn(C, generator=gen, dtype=torch.float32)
        assert torch.equal(sn.u[o:o + C], d / max(float(d.norm()), 1e-12))
        assert not sn.u[o + C:o + (C + 3) // 4 * 4].any()
    with K.dry_run():
        assert torch.equal(optim.SpectralNorm(arena, SC.NORMALISED, seed=3).u, sn.u)
        assert not torch.equal(optim.SpectralNorm(arena, SC.NORMALISED, seed=4).u, sn.u)
    only = sn.table.only([1, 4])
    assert list(only.host[:, 6]) == [0, 1, 0, 0, 1, 0, 0, 0, 0] and np.array_equal(only.host[:, :6], host[:, :6]) and list(host[:, 6]) == [1] * 9
    # the state keys, and a verbatim round trip
    sd = sn.state_dict()
    assert list(sd)[:4] == ['d_net/a/weights/spectral_raw', 'd_net/a/weights/spectral_u', 'd_net/a/weights/spectral_v', 'd_net/a/weights/spectral_sigma']
    assert len(sd) == 4 * len(SC.NORMALISED) and tuple(sd['d_net/odd/kernel/spectral_raw'].shape) == (7, 5)
    assert tuple(sd['d_net/odd/kernel/spectral_u'].shape) == (5,) and tuple(sd['d_net/odd/kernel/spectral_v'].shape) == (7,)
    sd['d_net/odd/kernel/spectral_sigma'] = torch.tensor([2.5])
    sd['d_net/odd/kernel/spectral_v'] = torch.arange(7.0)
    sn.load_state_dict({k: v for k, v in sd.items() if k.startswith('d_net/odd/')})
    assert float(sn.sigma[sn.index['d_net/odd/kernel']]) == 2.5 and torch.equal(sn.state_tensor('d_net/odd/kernel/spectral_v'), torch.arange(7.0))
    assert float(sn.sigma.sum()) == 2.5 + len(SC.NORMALISED) - 1


# ---- refusals in Python -------------------------------------------------------------------------------------------------------------
def test_spectral_norm_and_adam_refusals():
    from t2i_amd import kernels as K
    from t2i_amd import optim
    arena = _arena()
    with K.dry_run():
        with pytest.raises(KeyError, match='not a variable'):
            optim.SpectralNorm(arena, ['d_net/nothing/weights'])
        for n in ('d_net/a/biases', 'd_net/b/gamma'):
            with pytest.raises(ValueError, match='at least 2 dimensions'):
                optim.SpectralNorm(arena, [n])
        with pytest.raises(ValueError, match='named twice'):
            optim.SpectralNorm(arena, [SC.ALONE, SC.ALONE])
        with pytest.raises(ValueError, match='no variable'):
            optim.SpectralNorm(arena, [])
        for w in (-1, 1.5, True):
            with pytest.raises(ValueError, match='warmup'):
                optim.SpectralNorm(arena, [SC.ALONE], warmup=w)
        sn = optim.SpectralNorm(arena, SC.NORMALISED)
        for it in (-1, 1.0, True):
            with pytest.raises(ValueError, match='iterations'):
                sn.normalize(it)
        with pytest.raises(KeyError, match='not normalised'):
            sn.sync(['d_net/a/biases'])
        with pytest.raises(KeyError, match='not a state key'):
            sn.load_state_dict({'d_net/a/biases/spectral_raw': torch.zeros(16)})
        with pytest.raises(KeyError, match='not a state key'):
            sn.load_state_dict({'d_net/odd/kernel/spectral_w': torch.zeros(7, 5)})
        with pytest.raises(KeyError, match='is missing'):
            sn.load_state_dict({'d_net/odd/kernel/spectral_raw': torch.zeros(7, 5)})
        bad = {k: v for k, v in sn.state_dict().items() if k.startswith('d_net/odd/')}
        bad['d_net/odd/kernel/spectral_u'] = torch.zeros(6)
        with pytest.raises(ValueError, match='shape'):
            sn.load_state_dict(bad)
        with pytest.raises(ValueError, match='do not combine'):
            optim.AdamTF(arena, 0.0, 0.99, ema_decay=0.999, spectral=sn)
        with pytest.raises(ValueError, match='SpectralNorm over this'):
            optim.AdamTF(arena, 0.0, 0.99, spectral='yes')
        with pytest.raises(ValueError, match='SpectralNorm over this'):
            optim.AdamTF(_arena(), 0.0, 0.99, spectral=sn)                                      # another arena's
        opt = optim.AdamTF(arena, 0.0, 0.99, spectral=sn, slot_scales={SC.ALONE: 0.5})          # slot_scales combine with it
        opt.prepare(1e-3)
        opt.apply()
        assert opt.spectral is sn and opt.slot_end is not None and optim.AdamTF(arena, 0.0, 0.99).spectral is None
    with pytest.raises(RuntimeError, match='no CPU path'):
        sn.normalize(1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        sn.grad_()


def test_spectral_table_refusals():
    from t2i_amd import kernels as K
    ok = [(0, 48, 3, 16), (48, 35, 7, 5), (84, 40, 40, 1)]
    tab = K.spectral_table(ok, 124, 'cpu')
    assert tab.n_slots == 3 and tab.max_items == 1 and tab.max_col_blocks == 1 and tab.part_floats == 20 + 8 + 4 and (tab.nu, tab.nv) == (16 + 8 + 4, 4 + 8 + 40)
    for slots, numel, word in (([], 124, 'slots'), ([(0, 4, 2, 2)] * (K.SPECTRAL_MAX_SLOTS + 1), 1 << 20, 'slots'),
                               (ok, 0, 'multiple of 4'), (ok, 126, 'multiple of 4'),
                               ([(0, 48, 3, 15)], 124, 'cannot be the matrix'), ([(0, 48, 0, 16)], 124, 'cannot be the matrix'),
                               ([(0, 48, 48, 0)], 124, 'cannot be the matrix'), ([(0, 48, -3, -16)], 124, 'cannot be the matrix'),
                               ([(2, 48, 3, 16)], 124, 'misaligned'), ([(-4, 48, 3, 16)], 124, 'misaligned'),
                               ([(80, 48, 3, 16)], 124, 'outside the arena'),
                               ([ok[1], ok[0]], 124, 'out of order'), ([ok[0], (44, 35, 7, 5)], 124, 'overlaps'),
                               ([ok[1], (80, 40, 40, 1)], 124, 'overlaps'),                       # inside the padding of the 35-element slot
                               ([(0, 1 << 36, 1 << 6, 1 << 30)], 1 << 37, 'cannot be the matrix'),
                               ([(0, 1 << 36, 1 << 29, 1 << 7)], 1 << 37, 'work items')):
        with pytest.raises(ValueError, match=word):
            K.spectral_table(slots, numel, 'cpu')


def test_the_wrappers_refuse_on_the_host():
    from t2i_amd import kernels as K
    tab = K.spectral_table([(0, 48, 3, 16), (48, 35, 7, 5)], 84, 'cpu')
    flat, raw, grad = torch.zeros(84), torch.zeros(84), torch.zeros(84)
    u, v, sigma, ws = torch.zeros(tab.nu), torch.zeros(tab.nv), torch.ones(2), torch.zeros(tab.ws_floats)
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.spectral_normalize(flat, raw, tab, u, v, sigma, ws)
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.spectral_grad_(grad, flat, tab, u, v, sigma, ws)
    with K.dry_run():
        K.spectral_normalize(flat, raw, tab, u, v, sigma, ws, iterations=0)
        K.spectral_grad_(grad, flat, tab, u, v, sigma, ws)
        for it in (-1, K.SPECTRAL_MAX_ITERATIONS + 1, 1.0, True):
            with pytest.raises(ValueError, match='iterations'):
                K.spectral_normalize(flat, raw, tab, u, v, sigma, ws, iterations=it)
        with pytest.raises(TypeError, match='spectral_table'):
            K.spectral_normalize(flat, raw, tab.host, u, v, sigma, ws)
        with pytest.raises(TypeError, match='float32'):
            K.spectral_normalize(flat.double(), raw, tab, u, v, sigma, ws)
        with pytest.raises(TypeError, match='float32'):
            K.spectral_grad_(grad, flat, tab, u.double(), v, sigma, ws)
        with pytest.raises(ValueError, match='contiguous'):
            K.spectral_grad_(torch.zeros(168)[::2], flat, tab, u, v, sigma, ws)
        for args in ((torch.zeros(88), raw, tab, u, v, sigma, ws), (flat, torch.zeros(80), tab, u, v, sigma, ws),
                     (flat, raw, tab, torch.zeros(tab.nu + 4), v, sigma, ws), (flat, raw, tab, u, torch.zeros(tab.nv - 4), sigma, ws),
                     (flat, raw, tab, u, v, torch.ones(3), ws), (flat, raw, tab, u, v, sigma, torch.zeros(tab.ws_floats - 1))):
            with pytest.raises(ValueError, match='elements'):
                K.spectral_normalize(*args)
            with pytest.raises(ValueError, match='elements'):
                K.spectral_grad_(*args)


# ---- the entries refuse bad arguments before any launch ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    so = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    return _lib


def test_entries_are_declared_and_the_abi_version_stays(lib):
    assert lib.ABI_VERSION == 13 and lib.lib.t2i_version() == 13
    for name, nargs in (('t2i_spectral_workspace_bytes', 1), ('t2i_spectral_grad', 15), ('t2i_spectral_normalize', 17)):
        assert name in lib.SIGNATURES and hasattr(lib.lib, name) and len(lib.SIGNATURES[name][1]) == nargs, name
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    assert 'size_t t2i_spectral_workspace_bytes(' in header and 'int t2i_spectral_grad(' in header and 'int t2i_spectral_normalize(' in header
    from t2i_amd import kernels as K
    for name, value in (('T2I_SPECTRAL_MAX_SLOTS', K.SPECTRAL_MAX_SLOTS), ('T2I_SPECTRAL_MAX_ITEMS (1 <<', 22),
                        ('T2I_SPECTRAL_MAX_ITERATIONS', K.SPECTRAL_MAX_ITERATIONS), ('T2I_SPECTRAL_COLS', K.SPECTRAL_COLS)):
        assert '#define %s %d' % (name, value) in header, name
    assert K.SPECTRAL_MAX_ITEMS == 1 << 22
    build = open(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 'build.sh')).read()
    assert build.count('t2i_spectral') == 2 and ' t2i_spectral ' in build and '"$OUT/t2i_spectral.o"' in build   # the compile list and the link line
    assert os.path.exists(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 't2i_spectral.hip'))


def test_the_workspace_query(lib):
    ws = lib.lib.t2i_spectral_workspace_bytes
    assert ws(1) == 256 and ws(64) == 256 and ws(65) == 512 and ws(1 << 20) == 4 << 20
    from t2i_amd import kernels as K
    for part in (4, 28, 64, 68, 2252):
        tab = K.spectral_table([(0, part, 1, part)], part, 'cpu')
        assert tab.part_floats == (part + 1 + (part + 63) // 64 + 3) // 4 * 4 and tab.ws_floats * 4 == ws(tab.part_floats), part
    for bad in (0, -1, (1 << 42) + 1):
        assert ws(bad) == 0, bad


P = ctypes.c_void_p
A_, B_, TAB, U_, V_, SIG, WS = P(0x10000000), P(0x20000000), P(0x28000000), P(0x30000000), P(0x38000000), P(0x40000000), P(0x60000000)
N, NS, ITEMS, NU, NV, PART, BIG = 4096, 3, 2, 64, 512, 256, 1 << 30


def _refusals(fn, ok, name, lib, extra=(), d=0):
    """ok: (a, b, n, table, n_slots, max_items) + d more + (u, nu, v, nv, sigma) + middle + (part_floats, ws, ws_bytes); the stream is
    appended.  d: how far the arguments behind max_items are shifted (t2i_spectral_normalize has max_col_blocks there)."""
    k = len(ok) - 3                                                     # index of part_floats

    def put(i, v, base=ok):
        return base[:i] + (v,) + base[i + 1:]
    need = lib.lib.t2i_spectral_workspace_bytes(PART)
    bad = [put(0, None), put(1, None), put(3, None), put(6 + d, None), put(8 + d, None), put(10 + d, None), put(k + 1, None),      # a NULL pointer
           put(2, 0), put(2, -4), put(2, 4098), put(2, (1 << 40) + 4),                                                 # n
           put(7 + d, 0), put(7 + d, 62), put(7 + d, -4), put(7 + d, N + 4), put(9 + d, 0), put(9 + d, 510), put(9 + d, N + 4),                    # nu, nv
           put(4, 0), put(4, -1), put(4, 2049),                                                                        # n_slots
           put(5, 0), put(5, -3), put(5, (1 << 22) + 1), put(5, N + 1),                                                # max_items
           put(k, 0), put(k, -8), put(k, 4 * N + 8 * NS + 1),                                                              # part_floats
           put(k + 2, 0), put(k + 2, need - 1),                                                                        # a short workspace
           put(0, P(0x10000004)), put(1, P(0x20000008)), put(6 + d, P(0x30000004)), put(8 + d, P(0x38000008)), put(10 + d, P(0x40000002)),
           put(3, P(0x28000004)), put(k + 1, P(0x60000008)),                                                           # misaligned
           put(1, A_), put(1, P(0x10000000 + 4 * N - 16)), put(6 + d, A_), put(8 + d, P(0x20000000 + 16)), put(10 + d, P(0x30000000 + 16)),
           put(8 + d, P(0x30000000 + 4 * NU - 16)), put(3, A_), put(3, P(0x38000000 + 8)), put(3, P(0x40000000 + 8)),
           put(k + 1, B_), put(k + 1, U_), put(k + 1, P(0x28000000 + 16)), put(k + 1, P(0x40000000 - need + 16)),
           put(10 + d, P(0x60000000 + 32))]                                                                                # overlapping
    for args in bad + [put(i, v) for i, v in extra]:
        assert fn(*args, None) == -1, ' '.join(str(getattr(a, 'value', a)) for a in args)
        msg = lib.lib.t2i_last_error()
        assert name in msg and b'bad argument' in msg, (args, msg)


def test_spectral_grad_refuses_bad_arguments(lib):
    ok = (A_, B_, N, TAB, NS, ITEMS, U_, NU, V_, NV, SIG, PART, WS, BIG)
    _refusals(lib.lib.t2i_spectral_grad, ok, b't2i_spectral_grad', lib)


def test_spectral_normalize_refuses_bad_arguments(lib):
    ok = (A_, B_, N, TAB, NS, ITEMS, 1, U_, NU, V_, NV, SIG, 1, PART, WS, BIG)
    _refusals(lib.lib.t2i_spectral_normalize, ok, b't2i_spectral_normalize', lib, d=1,
              extra=((6, 0), (6, -2), (6, (1 << 22) + 1), (6, N + 1), (12, -1), (12, 65)))
    assert b'iterations = 65' in lib.lib.t2i_last_error()


# ---- the model's argument -------------------------------------------------------------------------------------------------------------
def test_pggan_critic_sn_is_validated_as_a_bool():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan import train_pggan
    from t2i_amd.models.pggan.pggan import PGGAN
    for bad in (1, 'yes', None, 0):
        with pytest.raises(ValueError, match='critic_sn must be True or False'):
            PGGAN(4, 10, None, None, None, None, None, 2, False, build_model=False, device='cpu', critic_sn=bad)
    assert PGGAN(4, 10, None, None, None, None, None, 2, False, build_model=False, device='cpu').critic_sn is False
    m = PGGAN(4, 10, None, None, None, None, None, 2, False, build_model=False, device='cpu', critic_sn=True)
    assert m.critic_sn is True and m.critic_spectral is None and m.spectral_synced is None
    assert PGGAN.kernel_names(OrderedDict([('d_net/x/weights', torch.zeros(3, 3, 2, 2)), ('d_net/x/biases', torch.zeros(2)),
                                           ('d_net/y/kernel', torch.zeros(4, 1)), ('d_net/y/weights', torch.zeros(4, 1)),
                                           ('d_net/z/gamma', torch.zeros(2, 2))])) == ['d_net/x/weights', 'd_net/y/kernel']
    assert '--critic-sn' in open(train_pggan.__file__).read()
