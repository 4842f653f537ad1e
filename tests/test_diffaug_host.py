"""Differentiable augmentation without a GPU: the three exports in header and binding within ABI v13, the
entry points' refusals on the host (before any launch), the operator's refusals on CPU tensors, the parameter draw on the CPU, and the
`diffaug` switch of PGGAN."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import diffaug_cases as DC  # noqa: E402

NEW_EXPORTS = ('t2i_diff_augment_workspace_bytes', 't2i_diff_augment_fwd', 't2i_diff_augment_adj')
COLOR, TRANSLATION, CUTOUT = 1, 2, 4


def test_new_exports_in_header_and_binding():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    from t2i_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    declared = set(re.findall(r'\b(t2i_[a-z0-9_]+)\s*\(', header))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.lib.t2i_version() == 13 and _lib.ABI_VERSION == 13
    assert re.search(r'T2I_DIFFAUG_COLOR = 1, T2I_DIFFAUG_TRANSLATION = 2, T2I_DIFFAUG_CUTOUT = 4', header)
    assert (K.DIFFAUG_COLOR, K.DIFFAUG_TRANSLATION, K.DIFFAUG_CUTOUT) == (COLOR, TRANSLATION, CUTOUT)
    assert 't2i_augment' in open(os.path.join(ROOT, 'text-to-image_amd', 'csrc', 'build.sh')).read()


def test_workspace_bytes():
    """One float per 4096 floats of a sample, per sample, with 'color'; nothing without it or for a refused shape.  The cut depends on
    H, W and C alone: B only multiplies."""
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    ws = _lib.lib.t2i_diff_augment_workspace_bytes
    assert int(ws(2, 4, 4, 3, 7)) == 2 * 1 * 4
    assert int(ws(2, 64, 64, 3, 1)) == 2 * 3 * 4 and int(ws(5, 64, 64, 3, 5)) == 5 * 3 * 4
    assert int(ws(1, 256, 256, 3, 7)) == 48 * 4
    assert int(ws(1, 37, 37, 3, 1)) == 2 * 4                  # 4107 floats: a ragged second chunk
    assert int(ws(2, 64, 64, 3, 6)) == 0 and int(ws(2, 64, 64, 3, 2)) == 0
    assert int(ws(0, 4, 4, 3, 7)) == 0 and int(ws(65536, 1, 1, 1, 7)) == 0 and int(ws(2, 4, 0, 3, 7)) == 0
    assert int(ws(2, 32768, 32768, 3, 7)) == 0


def test_the_entry_points_refuse_bad_arguments_on_the_host():
    """Validation happens before any launch: a host buffer stands in for the tensors, so a call that passed it would enqueue a kernel
    on host addresses — every call made here has a refused argument."""
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    L = _lib.lib
    x = (ctypes.c_float * 4096)()
    y = (ctypes.c_float * 4096)()
    P = (ctypes.c_float * 64)()
    W = (ctypes.c_float * 64)()
    px, py, pP, pW = (ctypes.cast(b, ctypes.c_void_p) for b in (x, y, P, W))
    big = 1 << 20

    def both(B, H, Wd, C, policy, x=px, P=pP, out=py, ws=pW, wsn=big):
        return (L.t2i_diff_augment_fwd(x, P, B, H, Wd, C, policy, 1, out, ws, wsn, None),
                L.t2i_diff_augment_adj(x, P, B, H, Wd, C, policy, out, ws, wsn, None))
    for shape in ((0, 4, 4, 3), (2, 0, 4, 3), (2, 4, 0, 3), (2, 4, 4, 0), (-1, 4, 4, 3), (65536, 1, 1, 1), (2, 32769, 1, 1), (2, 1, 32769, 1),
                  (4, 32768, 32768, 3)):
        assert both(*shape, 7) == (-1, -1), shape
        assert b'diff_augment' in L.t2i_last_error()
    for policy in (0, 8, 9, 15, -1, 1 << 20):                              # an unknown bit, or no bit at all
        assert both(2, 4, 4, 3, policy) == (-1, -1), policy
        assert b'policy' in L.t2i_last_error()
    assert both(2, 4, 4, 3, 7, x=None) == (-1, -1)
    assert both(2, 4, 4, 3, 7, P=None) == (-1, -1)
    assert both(2, 4, 4, 3, 7, out=None) == (-1, -1)
    assert both(2, 4, 4, 3, 7, out=px) == (-1, -1)                          # in place: the kernels gather
    assert both(2, 4, 4, 3, 6, out=ctypes.c_void_p(px.value + 8)) == (-1, -1) and b'overlap' in L.t2i_last_error()
    need = int(L.t2i_diff_augment_workspace_bytes(2, 4, 4, 3, 7))
    assert need == 8
    for ws, wsn in ((None, big), (pW, need - 1), (pW, 0)):
        assert both(2, 4, 4, 3, 7, ws=ws, wsn=wsn) == (-1, -1), (ws, wsn)
        assert b'workspace' in L.t2i_last_error()
        assert both(2, 4, 4, 3, 1, ws=ws, wsn=wsn) == (-1, -1)


def _stacked(t):
    from t2i_amd import stacked as ST
    return ST.Stacked(t, t.clone())


def test_the_operator_refuses_before_any_launch_on_the_host():
    """utils.ops.diff_augment: every refusal names the operator and precedes the kernels' own 'no CPU path' error"""
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    x, P = torch.zeros(2, 4, 4, 3), DC.identity_table(2)
    with pytest.raises(ValueError, match='diff_augment'):
        ops.diff_augment(x.bfloat16(), P)
    with pytest.raises(NotImplementedError, match='diff_augment'):
        ops.diff_augment(_stacked(x), P)
    with pytest.raises(ValueError, match='diff_augment'):
        ops.diff_augment(x[0], P)
    with pytest.raises(ValueError, match='diff_augment.*non-contiguous'):
        ops.diff_augment(torch.zeros(2, 3, 4, 4).permute(0, 2, 3, 1), P)
    for policy in ('colour', 'color,', '', 'color translation', None, 7, 'color,flip'):
        with pytest.raises(ValueError, match='diff_augment.*policy'):
            ops.diff_augment(x, P, policy)
    for bad in (DC.identity_table(3), DC.identity_table(2)[:, :8], DC.identity_table(2).double(), DC.identity_table(2).reshape(-1), [0.0] * 18):
        with pytest.raises(ValueError, match='diff_augment.*params'):
            ops.diff_augment(x, bad)
    with pytest.raises(ValueError, match='diff_augment.*params'):
        ops.diff_augment(x, torch.zeros(9, 2).t())                         # right shape, wrong strides
    with pytest.raises(RuntimeError, match='no CPU path'):                  # and an accepted call on CPU tensors has no fallback
        ops.diff_augment(x, P)
    assert ops.diff_augment_policy('cutout, color') == COLOR | CUTOUT and ops.diff_augment_policy(DC.ALL) == 7


@pytest.mark.parametrize('H,W', [(4, 4), (5, 7), (256, 256)])
def test_the_parameter_draw_on_the_cpu(H, W):
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    n = 4096
    gen = torch.Generator().manual_seed(7)
    P = ops.diff_augment_params(n, H, W, DC.ALL, generator=gen)
    assert tuple(P.shape) == (n, 9) and P.dtype == torch.float32 and P.device.type == 'cpu'
    b, s, c = P[:, 0], P[:, 1], P[:, 2]
    assert float(b.min()) >= -0.5 and float(b.max()) <= 0.5 and float(b.min()) < -0.45 and float(b.max()) > 0.45
    assert float(s.min()) >= 0.0 and float(s.max()) <= 2.0 and float(s.min()) < 0.1 and float(s.max()) > 1.9
    assert float(c.min()) >= 0.5 and float(c.max()) <= 1.5 and float(c.min()) < 0.55 and float(c.max()) > 1.45
    assert torch.equal(P[:, 3:], P[:, 3:].round())                          # integer-valued geometry
    for col, size in ((3, H), (4, W)):
        r = int(size / 8.0 + 0.5)
        assert sorted(set(P[:, col].tolist())) == [float(v) for v in range(-r, r + 1)]
    for col, size in ((5, H), (7, W)):
        ext = int(size / 2.0 + 0.5)
        lo, hi = P[:, col], P[:, col + 1]
        assert bool((lo >= 0).all()) and bool((hi <= size).all()) and bool((hi > lo).all())           # non-empty, inside the image
        assert int((hi - lo).max()) == ext and int((hi - lo).min()) == ext - ext // 2                  # whole, and clipped at a border
        assert float(lo.min()) == 0.0 and float(hi.max()) == float(size)
    # the same generator state gives the same table; `out=` is written in place and returned
    again = ops.diff_augment_params(n, H, W, DC.ALL, generator=torch.Generator().manual_seed(7))
    assert torch.equal(P, again)
    out = torch.full((n, 9), 99.0)
    got = ops.diff_augment_params(n, H, W, DC.ALL, generator=torch.Generator().manual_seed(7), out=out)
    assert got is out and torch.equal(out, P)
    # a policy that is absent gets identity columns
    ident = DC.identity_table(n)
    for policy, cols in (('color', (0, 1, 2)), ('translation', (3, 4)), ('cutout', (5, 6, 7, 8)), ('cutout,color', (0, 1, 2, 5, 6, 7, 8))):
        Q = ops.diff_augment_params(n, H, W, policy, generator=torch.Generator().manual_seed(3), out=torch.full((n, 9), 99.0))
        rest = [j for j in range(9) if j not in cols]
        assert torch.equal(Q[:, rest], ident[:, rest]), policy
        assert all(float(Q[:, j].std()) > 0 for j in cols), policy


def test_the_parameter_draw_refuses_bad_arguments():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    with pytest.raises(ValueError, match='diff_augment_params.*policy'):
        ops.diff_augment_params(4, 8, 8, 'flip')
    with pytest.raises(ValueError, match='diff_augment_params'):
        ops.diff_augment_params(0, 8, 8)
    with pytest.raises(ValueError, match='diff_augment_params.*out'):
        ops.diff_augment_params(4, 8, 8, out=torch.zeros(4, 8))
    with pytest.raises(ValueError, match='diff_augment_params.*out'):
        ops.diff_augment_params(4, 8, 8, out=torch.zeros(4, 9, dtype=torch.float64))


def test_the_float64_restatement_on_a_case_worked_by_hand():
    """One 2x2x2 sample: b = 1, s = 0 (each pixel becomes its channel mean), c = 2 (twice the distance from the sample mean), a shift
    one row down, the right column cut"""
    x = torch.tensor([[[[0.0, 2.0], [1.0, 3.0]], [[4.0, 6.0], [5.0, 7.0]]]], dtype=torch.float64)
    P = torch.tensor([[1.0, 0.0, 2.0, 1, 0, 0, 2, 1, 2]], dtype=torch.float64)
    # u1 = x + 1; pixel means 2, 3, 6, 7; sample mean 4.5; contrast: 2 m - 4.5 = -0.5, 1.5, 7.5, 9.5
    want = torch.tensor([[[[0.0, 0.0], [0.0, 0.0]], [[-0.5, -0.5], [0.0, 0.0]]]], dtype=torch.float64)
    assert torch.equal(DC.ref_T(x, P), want)
    assert torch.equal(DC.ref_T(x, P, 'translation'), torch.cat([torch.zeros_like(x[:, :1]), x[:, :1]], 1))
    assert torch.equal(DC.ref_T(x, DC.identity_table(1, torch.float64)), x)


@pytest.mark.parametrize('bad', ['colour', '', 'color,', 7, True, ('color',)])
def test_diffaug_is_validated_before_anything_is_built(bad):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    with pytest.raises(ValueError, match='diffaug'):
        PGGAN(2, 100, None, None, None, None, None, 2, False, device='cpu', diffaug=bad, build_model=False)


def test_the_flag_is_kept_and_the_default_is_none():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    mk = lambda **kw: PGGAN(2, 100, None, None, None, None, None, 2, False, device='cpu', build_model=False, **kw)
    assert mk().diffaug is None and mk(diffaug=None).diffaug is None
    assert mk(diffaug='color').diffaug == 'color' and mk(diffaug='cutout,translation,color').diffaug == 'cutout,translation,color'


@pytest.mark.parametrize('stage,trans', [(1, False), (3, True)])
def test_a_dry_build_has_the_same_variables_with_and_without_the_flag(stage, trans):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    kw = dict(device='cpu', fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)
    shapes = []
    for aug in (None, DC.ALL):
        m = PGGAN(4, 100, None, None, None, None, None, stage, trans, diffaug=aug, **kw)
        shapes.append([(n, tuple(v.shape)) for n, v in m.store.vars.items()])
    assert shapes[0] == shapes[1] and len(shapes[0]) > 0


def test_the_command_line_refuses_a_bad_policy(capsys):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan import train_pggan
    with pytest.raises(SystemExit) as e:
        train_pggan.main(['--diffaug', 'color,flip', '--bench'])
    assert e.value.code == 2 and 'diffaug' in capsys.readouterr().err
