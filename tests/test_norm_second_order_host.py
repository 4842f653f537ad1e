"""Second-order layer_norm / pixel_norm without a GPU: the new exports in header and binding within ABI v13, and the `critic_norm`
switch of PGGAN (its refusal, and the LayerNorm variables a normalised critic creates under d_net)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ('t2i_pixel_norm_bwd2', 't2i_layer_norm_bwd2_workspace_bytes', 't2i_layer_norm_bwd2_sums', 't2i_layer_norm_bwd2_apply')


def test_new_exports_in_header_and_binding():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    declared = set(re.findall(r'\b(t2i_[a-z0-9_]+)\s*\(', header))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.lib.t2i_version() == 13 and _lib.ABI_VERSION == 13
    assert int(_lib.lib.t2i_layer_norm_bwd2_workspace_bytes(3)) == 3 * 256 * 5 * 4 and int(_lib.lib.t2i_layer_norm_bwd2_workspace_bytes(0)) == 0


def test_the_double_backward_entry_points_refuse_bad_arguments_on_the_host():
    """Validation happens before any launch: tanh, a negative lrelu slope and a missing activation output are T2I_ERR_INVALID"""
    import ctypes
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    from t2i_amd import kernels as K
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    L = _lib.lib
    for act, alpha in ((K.ACT_TANH, 0.0), (K.ACT_LRELU, -0.5), (7, 0.0)):
        assert L.t2i_pixel_norm_bwd2(p, p, p, p, 2, 8, act, alpha, p, p, None) != 0
        assert L.t2i_layer_norm_bwd2_sums(p, p, p, p, p, 2, 8, 8, act, alpha, p, p, 4096, None) != 0
        assert L.t2i_layer_norm_bwd2_apply(p, p, p, p, p, p, p, 2, 8, 8, act, alpha, p, p, None, None) != 0
    assert L.t2i_layer_norm_bwd2_sums(p, p, p, None, p, 2, 8, 8, K.ACT_RELU, 0.0, p, p, 4096, None) != 0       # relu needs y
    assert L.t2i_layer_norm_bwd2_sums(p, p, p, None, p, 2, 8, 3, K.ACT_NONE, 0.0, p, p, 4096, None) != 0       # C does not divide a sample
    assert L.t2i_pixel_norm_bwd2(p, p, None, p, 2, 8, K.ACT_NONE, 0.0, p, p, None) != 0


def test_critic_norm_is_validated_before_anything_is_built():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    with pytest.raises(ValueError, match='critic_norm'):
        PGGAN(2, 100, None, None, None, None, None, 2, False, device='cpu', critic_norm='batch', build_model=False)
    with pytest.raises(ValueError, match='critic_norm'):
        PGGAN(2, 100, None, None, None, None, None, 2, False, device='cpu', critic_norm='batch')


@pytest.mark.parametrize('stage,trans', [(1, False), (3, True)])
def test_layer_norm_variables_of_a_normalised_critic(stage, trans):
    """Variable creation is a dry pass (K.dry_run inside build_model): the normalised critic's LayerNorm variables carry TF's automatic
    names under d_net, after the convolution they follow; 'pixel' and None create none; the generator's are untouched."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    kw = dict(device='cpu', fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)
    names, g_names = {}, {}
    for norm in (None, 'layer', 'pixel'):
        m = PGGAN(2, 100, None, None, None, None, None, stage, trans, critic_norm=norm, **kw)
        names[norm] = list(m.store.trainable_variables('d_net'))
        g_names[norm] = list(m.store.trainable_variables('g_net'))
        assert list(m.d_arena.names) == names[norm]
    assert g_names['layer'] == g_names[None] == g_names['pixel']
    ln = [n for n in names['layer'] if '/LayerNorm' in n]
    expect = []
    for i in range(stage - 1, -1, -1):
        for k in ('LayerNorm', 'LayerNorm_1'):
            expect += ['d_net/conv_stage_%d/%s/beta' % (i, k), 'd_net/conv_stage_%d/%s/gamma' % (i, k)]
    assert ln == expect
    assert [n for n in names['layer'] if n not in ln] == names[None] == names['pixel']
    assert not any('LayerNorm' in n for n in names[None])
    i = names['layer'].index('d_net/conv_stage_0/LayerNorm/beta')
    assert names['layer'][i - 1] == 'd_net/conv_stage_0/Conv/biases' and names['layer'][i + 2] == 'd_net/conv_stage_0/Conv_1/weights'
