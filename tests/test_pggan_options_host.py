"""PGGAN's options said once (models/pggan/options.py), without a device: the order in which the generator skeleton creates its variables
(from which the arena layout, the slot tables and the checkpoint files follow), the one validator behind the constructor and the flags,
utils.saver.latest_checkpoint, and restore_generator's two refusals from one look into the archive."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_pggan_real_host import no_device  # noqa: E402,F401

TINY = dict(fmap_base=32, fmap_max=16, z_dim=8, embed_dim=32, compr_embed_dim=16)


def _pggan(stage=2, trans=True, **kw):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.pggan import PGGAN
    return PGGAN(4, 10, None, None, None, None, None, stage, trans, device='cpu', **dict(TINY, **kw))


# ---- variable order: recorded from the commit before the two skeletons became one (stage 2, trans=True, the TINY widths) ---------------
G_TRUNK = [('g_net/conv_stage_0/dense/kernel', (32, 16)), ('g_net/conv_stage_0/dense/bias', (16,)), ('g_net/conv_stage_0/dense_1/kernel', (32, 16)),
           ('g_net/conv_stage_0/dense_1/bias', (16,)), ('g_net/conv_stage_0/dense_2/kernel', (24, 256)), ('g_net/conv_stage_0/dense_2/bias', (256,)),
           ('g_net/conv_stage_0/LayerNorm/beta', (256,)), ('g_net/conv_stage_0/LayerNorm/gamma', (256,))]
G_MAPPING = [('g_net/mapping/dense/kernel', (24, 16)), ('g_net/mapping/dense/bias', (16,)), ('g_net/mapping/dense_1/kernel', (16, 16)),
             ('g_net/mapping/dense_1/bias', (16,)), ('g_net/mapping/dense_2/kernel', (16, 16)), ('g_net/mapping/dense_2/bias', (16,)),
             ('g_net/mapping/dense_3/kernel', (16, 16)), ('g_net/mapping/dense_3/bias', (16,)), ('g_net/mapping/w_avg', (16,))]
G_RGB_0 = [('g_net/rgb_stage_0/Conv/weights', (2, 2, 16, 9)), ('g_net/rgb_stage_0/Conv/biases', (9,)),
           ('g_net/rgb_stage_0/Conv_1/weights', (1, 1, 9, 3)), ('g_net/rgb_stage_0/Conv_1/biases', (3,))]
G_RGB_1 = [('g_net/rgb_stage_1/Conv/weights', (2, 2, 16, 9)), ('g_net/rgb_stage_1/Conv/biases', (9,)),
           ('g_net/rgb_stage_1/Conv_1/weights', (1, 1, 9, 3)), ('g_net/rgb_stage_1/Conv_1/biases', (3,))]
D_BLOCKS = [('d_net/rgb_stage_0/Conv/weights', (1, 1, 3, 16)), ('d_net/rgb_stage_0/Conv/biases', (16,)), ('d_net/rgb_stage_1/Conv/weights', (1, 1, 3, 16)),
            ('d_net/rgb_stage_1/Conv/biases', (16,)), ('d_net/conv_stage_1/Conv/weights', (3, 3, 16, 16)), ('d_net/conv_stage_1/Conv/biases', (16,)),
            ('d_net/conv_stage_1/Conv_1/weights', (3, 3, 16, 16)), ('d_net/conv_stage_1/Conv_1/biases', (16,)),
            ('d_net/conv_stage_0/dense/kernel', (32, 16)), ('d_net/conv_stage_0/dense/bias', (16,))]
D_TAIL = [('d_net/conv_stage_0/Conv/biases', (16,)), ('d_net/conv_stage_0/Conv_1/weights', (4, 4, 16, 16)), ('d_net/conv_stage_0/Conv_1/biases', (16,)),
          ('d_net/conv_stage_0/dense_1/kernel', (16, 1)), ('d_net/conv_stage_0/dense_1/bias', (1,))]
D_NET = D_BLOCKS + [('d_net/conv_stage_0/Conv/weights', (3, 3, 32, 16))] + D_TAIL
D_NET_MBSTD = D_BLOCKS + [('d_net/conv_stage_0/Conv/weights', (3, 3, 36, 16))] + D_TAIL          # four statistic channels more
PLAIN = G_TRUNK + [
    ('g_net/conv_stage_0/Conv/weights', (3, 3, 16, 16)), ('g_net/conv_stage_0/Conv/biases', (16,)), ('g_net/conv_stage_0/LayerNorm_1/beta', (16,)),
    ('g_net/conv_stage_0/LayerNorm_1/gamma', (16,)), ('g_net/conv_stage_0/Conv_1/weights', (3, 3, 16, 16)), ('g_net/conv_stage_0/Conv_1/biases', (16,)),
    ('g_net/conv_stage_0/LayerNorm_2/beta', (16,)), ('g_net/conv_stage_0/LayerNorm_2/gamma', (16,))] + G_RGB_0 + [
    ('g_net/conv_stage_1/Conv/weights', (3, 3, 16, 16)), ('g_net/conv_stage_1/Conv/biases', (16,)), ('g_net/conv_stage_1/LayerNorm/beta', (16,)),
    ('g_net/conv_stage_1/LayerNorm/gamma', (16,)), ('g_net/conv_stage_1/Conv_1/weights', (3, 3, 16, 16)), ('g_net/conv_stage_1/Conv_1/biases', (16,)),
    ('g_net/conv_stage_1/LayerNorm_1/beta', (16,)), ('g_net/conv_stage_1/LayerNorm_1/gamma', (16,))] + G_RGB_1
STYLE = G_TRUNK + G_MAPPING + [
    ('g_net/conv_stage_0/Conv/weights', (3, 3, 16, 16)), ('g_net/conv_stage_0/Conv/biases', (16,)), ('g_net/conv_stage_0/StyleMod/noise_strength', (16,)),
    ('g_net/conv_stage_0/StyleMod/style/kernel', (16, 32)), ('g_net/conv_stage_0/StyleMod/style/bias', (32,)),
    ('g_net/conv_stage_0/Conv_1/weights', (3, 3, 16, 16)), ('g_net/conv_stage_0/Conv_1/biases', (16,)),
    ('g_net/conv_stage_0/StyleMod_1/noise_strength', (16,)), ('g_net/conv_stage_0/StyleMod_1/style/kernel', (16, 32)),
    ('g_net/conv_stage_0/StyleMod_1/style/bias', (32,))] + G_RGB_0 + [
    ('g_net/conv_stage_1/Conv/weights', (3, 3, 16, 16)), ('g_net/conv_stage_1/Conv/biases', (16,)), ('g_net/conv_stage_1/StyleMod/noise_strength', (16,)),
    ('g_net/conv_stage_1/StyleMod/style/kernel', (16, 32)), ('g_net/conv_stage_1/StyleMod/style/bias', (32,)),
    ('g_net/conv_stage_1/Conv_1/weights', (3, 3, 16, 16)), ('g_net/conv_stage_1/Conv_1/biases', (16,)),
    ('g_net/conv_stage_1/StyleMod_1/noise_strength', (16,)), ('g_net/conv_stage_1/StyleMod_1/style/kernel', (16, 32)),
    ('g_net/conv_stage_1/StyleMod_1/style/bias', (32,))] + G_RGB_1
STYLE_QUIET = G_TRUNK + G_MAPPING + [
    ('g_net/conv_stage_0/Conv/weights', (3, 3, 16, 16)), ('g_net/conv_stage_0/Conv/biases', (16,)), ('g_net/conv_stage_0/StyleMod/style/kernel', (16, 32)),
    ('g_net/conv_stage_0/StyleMod/style/bias', (32,)), ('g_net/conv_stage_0/Conv_1/weights', (3, 3, 16, 16)), ('g_net/conv_stage_0/Conv_1/biases', (16,)),
    ('g_net/conv_stage_0/StyleMod_1/style/kernel', (16, 32)), ('g_net/conv_stage_0/StyleMod_1/style/bias', (32,))] + G_RGB_0 + [
    ('g_net/conv_stage_1/Conv/weights', (3, 3, 16, 16)), ('g_net/conv_stage_1/Conv/biases', (16,)), ('g_net/conv_stage_1/StyleMod/style/kernel', (16, 32)),
    ('g_net/conv_stage_1/StyleMod/style/bias', (32,)), ('g_net/conv_stage_1/Conv_1/weights', (3, 3, 16, 16)), ('g_net/conv_stage_1/Conv_1/biases', (16,)),
    ('g_net/conv_stage_1/StyleMod_1/style/kernel', (16, 32)), ('g_net/conv_stage_1/StyleMod_1/style/bias', (32,))] + G_RGB_1


@pytest.mark.parametrize('kw,expected', [
    ({}, PLAIN + D_NET), (dict(style_dim=16), STYLE + D_NET), (dict(style_dim=16, style_noise=False), STYLE_QUIET + D_NET),
    (dict(critic_mbstd=4, equalized_lr=True), PLAIN + D_NET_MBSTD)], ids=['plain', 'style', 'style_quiet', 'mbstd_eqlr'])
def test_variables_are_created_in_the_recorded_order(kw, expected):
    m = _pggan(**kw)
    assert list(m.store.vars) == [n for n, _ in expected]
    assert [(n, tuple(v.shape)) for n, v in m.store.vars.items()] == expected


# ---- one validator, two voices ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('keyword,kw,flag,argv', [
    ('g_ema', dict(g_ema=1.5), '--g-ema', ['--g-ema', '1.5']),
    ('adam_lr', dict(adam_lr=0.0), '--lr', ['--lr', '0']),
    ('diffaug_p', dict(diffaug='color', diffaug_p=1.5), '--diffaug-p', ['--diffaug', 'color', '--diffaug-p', '1.5']),
    ('critic_mbstd', dict(critic_mbstd=0), '--critic-mbstd', ['--critic-mbstd', '0']),
    ('style_dim', dict(style_dim=0), '--style-dim', ['--style-dim', '0']),
    ('truncation_psi', dict(style_dim=16, truncation_psi=float('nan')), '--truncation-psi', ['--style-dim', '16', '--truncation-psi', 'nan']),
    ('resample_filter', dict(resample_filter=(1, -1)), '--resample-filter', ['--resample-filter', '1,-1'])])
def test_one_check_speaks_of_the_keyword_and_of_the_flag(tmp_path, no_device, capsys, keyword, kw, flag, argv):  # noqa: F811
    from t2i_amd.models.pggan import eval_pggan, options
    with pytest.raises(ValueError) as e:
        _pggan(build_model=False, **kw)
    assert keyword in str(e.value) and flag not in str(e.value)
    with pytest.raises(ValueError) as spoken:                   # the same sentence, the keyword's name replaced by the flag's
        options.validated(4, label=options.flag, **kw)
    assert str(spoken.value) == str(e.value).replace(keyword, flag)
    run = str(tmp_path / 'run')
    with pytest.raises(SystemExit) as e:
        no_device.main(['--out', run, '--first', '0', '--last', '0', '--iters', '2'] + argv)
    assert e.value.code == 2 and flag in capsys.readouterr().err and not os.path.exists(run)
    if keyword == 'truncation_psi':                             # a reader's flag: the trainer's parser refuses it unheard; the evaluator hears it
        with pytest.raises(SystemExit) as e:
            eval_pggan.main(['--cfg', str(tmp_path / 'none.yml')] + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and str(spoken.value) in err


# ---- latest_checkpoint --------------------------------------------------------------------------------------------------------------
def test_latest_checkpoint_is_the_archive_the_state_file_names(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.utils.saver import latest_checkpoint
    d = str(tmp_path / 'stage1')
    assert latest_checkpoint(d) is None                         # no directory
    os.makedirs(d)
    open(os.path.join(d, 'model-40.npz'), 'wb').close()
    assert latest_checkpoint(d) is None                         # no state file
    open(os.path.join(d, 'checkpoint'), 'w').write('model_checkpoint_path: "model-60.npz"\n')
    assert latest_checkpoint(d) is None                         # the state file names a missing archive
    open(os.path.join(d, 'checkpoint'), 'w').write('model_checkpoint_path: "model-40.npz"\n')
    assert latest_checkpoint(d) == os.path.join(d, 'model-40.npz')
    open(os.path.join(d, 'model-80.npz'), 'wb').close()         # newer, but not the one the state file names
    assert latest_checkpoint(d) == os.path.join(d, 'model-40.npz')


# ---- one open, both refusals --------------------------------------------------------------------------------------------------------
def test_restore_generator_refuses_style_then_taps_before_it_reads_a_variable(tmp_path, monkeypatch):
    from t2i_amd.models.pggan import eval_pggan as E
    from t2i_amd.models.pggan import options
    from t2i_amd.models.pggan.pggan import RESAMPLE_KEY
    from t2i_amd.utils.config import AttrDict
    from t2i_amd.utils.saver import save
    cfg = AttrDict({'CHECKPOINT_DIR': str(tmp_path)})
    writer = _pggan(stage=1, trans=False, style_dim=16, resample_filter=(1, 3, 3, 1))
    path = save(writer._savers()[0], None, os.path.join(cfg.CHECKPOINT_DIR, 'stage1/'), 5)
    assert RESAMPLE_KEY in np.load(path).files
    opened = []
    load = np.load
    monkeypatch.setattr(options.np, 'load', lambda *a, **k: (opened.append(a[0]), load(*a, **k))[1])
    mark = 'g_net/conv_stage_0/dense_2/kernel'
    for kw, message in ((dict(), r'--style-dim 16 --mapping-layers 4.*no --style-dim.*pass the same --style-dim'),
                        (dict(style_dim=16, resample_filter=(1, 2, 1)), r'0\.125, 0\.375, 0\.375, 0\.125.*0\.25, 0\.5, 0\.25.*pass the same --resample-filter')):
        reader = E.stage_model(cfg, 1, 4, None, torch.device('cpu'), **dict(TINY, **kw))
        with torch.no_grad():
            reader.store.vars[mark].fill_(0.25)
        del opened[:]
        with pytest.raises(RuntimeError, match=message):
            E.restore_generator(reader)
        assert opened == [path]
        assert bool((reader.store.vars[mark].detach() == 0.25).all())
    same = E.stage_model(cfg, 1, 4, None, torch.device('cpu'), style_dim=16, resample_filter=(2, 6, 6, 2), **TINY)
    E.restore_generator(same)
    assert torch.equal(same.store.vars[mark], writer.store.vars[mark])
