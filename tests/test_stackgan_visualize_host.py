"""StackGAN's caption visualisers, host side (no GPU): the host statement of the reference's float imresize(..., 'nearest')
(utils/visualize.py stage_imgs_host) against Pillow and visualize_last_stage.bytescale, the argument rules of `--visualize` /
`--interp` in stageI/run.py and stageII/run.py, and the declaration of t2i_bytescale_nearest."""
import os
import re
import sys

import numpy as np
import pytest
import yaml
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CFG = os.path.join(ROOT, 'text-to-image_amd', 'models', 'stackgan')


def _images():
    """Hand-made float32 images [4, 6, 6, 3]: a ramp inside [-1, 1], a constant image (cscale 0 -> 1), values outside [-1, 1],
    and seeded noise."""
    ramp = np.linspace(-1.0, 1.0, 6 * 6 * 3, dtype=np.float32).reshape(6, 6, 3)
    const = np.full((6, 6, 3), 0.3, np.float32)
    beyond = (ramp * np.float32(1.7) + np.float32(0.4)).astype(np.float32)
    noise = np.random.default_rng(0).standard_normal((6, 6, 3)).astype(np.float32)
    return np.stack([ramp, const, beyond, noise])


def test_stage_imgs_host_is_bytescale_then_pillow_nearest():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan.visualize_last_stage import bytescale, stage_sample
    from t2i_amd.utils.visualize import stage_imgs_host
    x = _images()
    assert x[2].min() < -1.0 and x[2].max() > 1.0
    for size in (4, 6, 16, 128):
        got = stage_imgs_host(x, size)
        assert got.shape == (4, size, size, 3) and got.dtype == np.uint8
        for i in range(4):
            u8 = bytescale((x[i] + np.float32(1.0)) * np.float32(127.5))
            assert u8.dtype == np.uint8
            want = np.array(Image.fromarray(u8).resize((size, size), Image.NEAREST))
            assert np.array_equal(got[i], want), (size, i)
            if i != 1 and size >= 6:                                    # (a smaller sheet can skip the extreme pixels)
                assert got[i].min() == 0 and got[i].max() == 255          # the image's own min and max
        assert np.all(got[1] == 0)                                        # constant: (v - cmin) * 255 / 1 = 0
        # the whole PGGAN statement, its / 127.5 - 1 included
        assert np.array_equal(stage_sample([x], size)[0], got / 127.5 - 1.0)
    # nearest: output pixel (r, c) is source pixel (floor((r + 0.5) * h / size), floor((c + 0.5) * w / size))
    big = stage_imgs_host(x, 16)
    src = stage_imgs_host(x, 6)                                           # the identity resize: the quantised source
    idx = ((np.arange(16) + 0.5) * 6 / 16).astype(int)
    assert np.array_equal(big, src[:, idx][:, :, idx])
    # one channel goes through Pillow as a grey image
    one = stage_imgs_host(x[:, :, :, :1], 16)
    assert one.shape == (4, 16, 16, 1)
    u8 = bytescale((x[3, :, :, 0] + np.float32(1.0)) * np.float32(127.5))
    assert np.array_equal(one[3, :, :, 0], np.array(Image.fromarray(u8).resize((16, 16), Image.NEAREST)))


def _cfg(tmp_path, stage, train_flag=True):
    cfg = yaml.safe_load(open(os.path.join(CFG, stage, 'cfg', 'flowers.yml')))
    d = str(tmp_path / stage)
    cfg.update(DATASET_DIR=d + '/data/', CHECKPOINT_DIR=d + '/ckpt/', LOGS_DIR=d + '/logs/', SAMPLE_DIR=d + '/samples/')
    cfg['TRAIN']['FLAG'] = train_flag
    cfg['EVAL']['FLAG'] = False
    cfgs = tmp_path.parent / (tmp_path.name + '_cfgs')            # the configs live beside tmp_path, which must stay empty
    cfgs.mkdir(exist_ok=True)
    path = str(cfgs / ('%s_%d.yml' % (stage, train_flag)))
    yaml.safe_dump(cfg, open(path, 'w'))
    return path


@pytest.mark.parametrize('stage', ['stageI', 'stageII'])
def test_visualize_argument_rules_come_before_any_directory(tmp_path, stage):
    import t2i_amd  # noqa: F401
    if stage == 'stageI':
        from t2i_amd.models.stackgan.stageI import run
        extra, vis = [], 'visualize_stagei.py'
    else:
        from t2i_amd.models.stackgan.stageII import run
        extra, vis = ['--cfg_stage_I', _cfg(tmp_path, 'stageI')], 'visualize_stageiI.py'
    train = _cfg(tmp_path, stage)
    no_train = _cfg(tmp_path, stage, train_flag=False)
    with pytest.raises(ValueError, match='--interp'):                      # --interp needs --visualize
        run.main(['--cfg', train, '--train', '--interp', '2'] + extra)
    with pytest.raises(ValueError, match='--interp'):
        run.main(['--cfg', no_train, '--interp', '1'] + extra)
    with pytest.raises(ValueError, match='--interp'):                      # and is >= 0
        run.main(['--cfg', train, '--visualize', '--interp', '-1'] + extra)
    with pytest.raises(ValueError, match='synthetic'):
        run.main(['--cfg', train, '--visualize', '--synthetic'] + extra)
    with pytest.raises(ValueError, match='synthetic'):
        run.main(['--cfg', no_train, '--visualize', '--interp', '3', '--synthetic'] + extra)
    with pytest.raises(SystemExit):                                        # one mode at a time
        run.main(['--cfg', train, '--visualize', '--train'] + extra)
    with pytest.raises(SystemExit):
        run.main(['--cfg', train, '--visualize', '--eval', 'is'] + extra)
    # TRAIN.FLAG: False with no mode still raises, still names the reference's visualiser file, and says how to get it
    with pytest.raises(NotImplementedError, match=vis) as e:
        run.main(['--cfg', no_train] + extra)
    assert 'pass --visualize for it' in str(e.value) and 'not built' not in str(e.value)
    assert list(tmp_path.iterdir()) == []                                  # no directory was created


def test_bytescale_nearest_is_declared_and_the_abi_version_stays():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib, kernels
    assert _lib.ABI_VERSION == 13 and _lib.lib.t2i_version() == 13
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    assert 'ABI version, currently 13' in header
    for name in ('t2i_bytescale_nearest', 't2i_bytescale_nearest_workspace_bytes'):
        assert name in _lib.SIGNATURES and re.search(r'\b%s\s*\(' % name, header), name
        assert getattr(_lib.lib, name) is not None
    assert len(_lib.SIGNATURES['t2i_bytescale_nearest'][1]) == 10 and len(_lib.SIGNATURES['t2i_bytescale_nearest_workspace_bytes'][1]) == 4
    assert callable(kernels.bytescale_nearest)
    # the workspace query needs no device: two floats per (image, chunk of 8192 elements), 0 for a shape the entry point refuses
    q = _lib.lib.t2i_bytescale_nearest_workspace_bytes
    assert q(8, 256, 256, 3) >= 8 * 24 * 2 * 4 and q(1, 4, 4, 3) >= 8
    assert q(0, 4, 4, 3) == 0 and q(1, 0, 4, 3) == 0 and q(1, 4, 4, 5) == 0 and q(1, 4, 4, 0) == 0
    # the wrapper refuses what the kernel does not take before it touches a device
    import torch
    for bad in (torch.zeros(2, 4, 4, 3, dtype=torch.float64), torch.zeros(2, 4, 4, 5), torch.zeros(4, 4, 3), torch.zeros(0, 4, 4, 3)):
        with pytest.raises(ValueError, match='bytescale_nearest'):
            kernels.bytescale_nearest(bad, 8)
    with pytest.raises(ValueError, match='bytescale_nearest'):
        kernels.bytescale_nearest(torch.zeros(1, 4, 4, 3), 0)
