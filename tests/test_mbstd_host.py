"""Minibatch standard deviation without a GPU: the new exports in header and binding within ABI v13, the entry
points' refusals on the host (before any launch), and the `critic_mbstd` switch of PGGAN: its validation, the group it picks, and the one
variable whose shape it changes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('t2i_minibatch_stddev_workspace_bytes', 't2i_minibatch_stddev_fwd', 't2i_minibatch_stddev_bwd', 't2i_minibatch_stddev_bwd2')


def test_new_exports_in_header_and_binding():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    declared = set(re.findall(r'\b(t2i_[a-z0-9_]+)\s*\(', header))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.lib.t2i_version() == 13 and _lib.ABI_VERSION == 13


def test_workspace_bytes():
    """One float per workgroup of the scalar form (which cuts a (group, chunk) finest); 0 for a shape the entry points refuse"""
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    ws = _lib.lib.t2i_minibatch_stddev_workspace_bytes
    src = open(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 't2i_ops.hip')).read()
    assert re.search(r'constexpr int kMbBlockUnits = kThreads;', src) and re.search(r'constexpr int kThreads = (\d+);', src)
    units = int(re.search(r'constexpr int kThreads = (\d+);', src).group(1))          # units (floats here) of a (group, chunk) per workgroup
    assert int(ws(32, 4, 4, 512, 4, 4)) == 8 * 4 * -(-4 * 4 * 128 // units) * 4 > 0
    assert int(ws(8, 1, 1, 3, 4, 1)) == 2 * 1 * 1 * 4
    assert int(ws(8, 3, 5, 6, 4, 2)) == 2 * 2 * 1 * 4
    assert int(ws(6, 4, 4, 16, 4, 4)) == 0 and int(ws(8, 4, 4, 16, 17, 4)) == 0 and int(ws(8, 4, 4, 6, 4, 4)) == 0


def test_the_entry_points_refuse_bad_arguments_on_the_host():
    """Validation happens before any launch: a host buffer stands in for the tensors, and nothing may be enqueued"""
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    L = _lib.lib
    big = 1 << 20

    def calls(B, H, W, C, G, F, x=p, out=p, ws=p, wsn=big, eps=1e-8, bwd=True):
        """-> the return codes of _fwd, _bwd2 and (bwd=True) _bwd.  Every call made from this file has a refused argument: _bwd takes no
        workspace, so the workspace cases leave it out — a call that passes validation would enqueue a kernel on host addresses."""
        rc = [L.t2i_minibatch_stddev_fwd(x, B, H, W, C, G, F, eps, out, ws, wsn, None),
              L.t2i_minibatch_stddev_bwd2(p, x, p, B, H, W, C, G, F, eps, out, p, ws, wsn, None)]
        if bwd:
            rc.append(L.t2i_minibatch_stddev_bwd(p, x, B, H, W, C, G, F, eps, out, None))
        return tuple(rc)
    bad = [(6, 2, 2, 8, 4, 1),        # B % G
           (8, 2, 2, 8, 0, 1),        # G = 0
           (34, 2, 2, 8, 17, 1),      # G = 17
           (8, 2, 2, 8, 4, 3),        # C % F
           (8, 2, 2, 8, 4, 0)]        # F = 0
    for shape in bad:
        rc = calls(*shape)
        assert all(r == -1 for r in rc), (shape, rc)
        assert b'minibatch_stddev' in L.t2i_last_error()
    assert all(r == -1 for r in calls(8, 2, 2, 8, 4, 1, x=None))
    assert all(r == -1 for r in calls(8, 2, 2, 8, 4, 1, eps=0.0)) and all(r == -1 for r in calls(8, 2, 2, 8, 4, 1, eps=-1.0))
    assert all(r == -1 for r in calls(8, 2, 2, 8, 4, 1, out=None))
    assert L.t2i_minibatch_stddev_bwd(None, p, 8, 2, 2, 8, 4, 1, 1e-8, p, None) == -1
    assert L.t2i_minibatch_stddev_bwd2(None, p, p, 8, 2, 2, 8, 4, 1, 1e-8, p, p, p, big, None) == -1
    assert L.t2i_minibatch_stddev_bwd2(p, p, None, 8, 2, 2, 8, 4, 1, 1e-8, p, p, p, big, None) == -1
    assert L.t2i_minibatch_stddev_bwd2(p, p, p, 8, 2, 2, 8, 4, 1, 1e-8, p, None, p, big, None) == -1
    need = int(L.t2i_minibatch_stddev_workspace_bytes(8, 2, 2, 8, 4, 1))
    assert need > 0
    for ws, wsn in ((None, big), (p, need - 1), (p, 0)):
        rc = calls(8, 2, 2, 8, 4, 1, ws=ws, wsn=wsn, bwd=False)
        assert rc == (-1, -1), rc
        assert b'workspace' in L.t2i_last_error()


def test_the_operator_refuses_before_any_launch_on_the_host():
    """utils.ops.minibatch_stddev[_stat]: every refusal names the operator and precedes the kernels' own 'no CPU path' error"""
    import torch
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    x = torch.zeros(8, 2, 2, 8)
    for fn in (ops.minibatch_stddev, ops.minibatch_stddev_stat):
        for kw in (dict(group_size=3), dict(group_size=17), dict(group_size=0), dict(num_features=3), dict(num_features=0), dict(eps=0.0)):
            with pytest.raises(ValueError, match='minibatch_stddev'):
                fn(x, **kw)
        with pytest.raises(ValueError, match='minibatch_stddev'):
            fn(x.bfloat16())
        with pytest.raises(ValueError, match='minibatch_stddev'):
            fn(x[0])
        with pytest.raises(ValueError, match='minibatch_stddev'):
            fn(torch.zeros(34, 1, 1, 4), group_size=17)


@pytest.mark.parametrize('bad', [0, -1, 'x', 2.0, True])
def test_critic_mbstd_is_validated_before_anything_is_built(bad):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    with pytest.raises(ValueError, match='critic_mbstd'):
        PGGAN(2, 100, None, None, None, None, None, 2, False, device='cpu', critic_mbstd=bad, build_model=False)
    with pytest.raises(ValueError, match='critic_mbstd'):
        PGGAN(2, 100, None, None, None, None, None, 2, False, device='cpu', critic_mbstd=bad)


def test_the_group_is_the_largest_divisor_of_the_batch():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    mk = lambda b, g: PGGAN(b, 100, None, None, None, None, None, 2, False, device='cpu', critic_mbstd=g, build_model=False).mbstd_group
    assert mk(6, 4) == 3 and mk(8, 4) == 4 and mk(4, 4) == 4 and mk(7, 4) == 1 and mk(3, 4) == 3 and mk(64, 4) == 4
    assert mk(64, 100) == 16 and mk(6, 1) == 1 and mk(2, None) is None
    assert PGGAN.mbstd_features(512) == 4 and PGGAN.mbstd_features(16) == 4 and PGGAN.mbstd_features(8) == 1 and PGGAN.mbstd_features(24) == 1


@pytest.mark.parametrize('stage,trans', [(1, False), (3, True)])
def test_only_the_first_filter_of_the_last_block_grows(stage, trans):
    """A dry build (K.dry_run inside build_model): the same variable names with and without the layer, for critic and generator; only
    d_net/conv_stage_0/Conv/weights changes shape, by F input channels; batch 6 with critic_mbstd=4 runs groups of 3"""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    kw = dict(device='cpu', fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)
    shapes = {}
    for mb in (None, 4):
        m = PGGAN(6, 100, None, None, None, None, None, stage, trans, critic_mbstd=mb, **kw)
        assert m.mbstd_group == (None if mb is None else 3)
        shapes[mb] = {s: [(n, tuple(v.shape)) for n, v in m.store.trainable_variables(s).items()] for s in ('d_net', 'g_net')}
        assert list(m.d_arena.names) == [n for n, _ in shapes[mb]['d_net']]
    assert shapes[None]['g_net'] == shapes[4]['g_net']
    assert [n for n, _ in shapes[None]['d_net']] == [n for n, _ in shapes[4]['d_net']]
    changed = [(a, b) for a, b in zip(shapes[None]['d_net'], shapes[4]['d_net']) if a != b]
    assert len(changed) == 1
    (name, s0), (_, s1) = changed[0]
    channels = 16                                     # get_dnf(0) = min(32 * 2, 16): a multiple of 16 => F = 4
    assert name == 'd_net/conv_stage_0/Conv/weights' and PGGAN.mbstd_features(channels) == 4
    assert s0 == (3, 3, channels + 16, 16) and s1 == (3, 3, channels + 16 + 4, 16)
