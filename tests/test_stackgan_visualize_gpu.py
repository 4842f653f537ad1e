"""StackGAN's caption visualisers on the GPU: t2i_bytescale_nearest bit for bit against the host statement (scipy's bytescale as
models/pggan/visualize_last_stage.py states it + Pillow's NEAREST), both generators' eval-mode passes on the fused and on the
unfused norm path against the float64 oracle, and stageI/run.py / stageII/run.py --visualize end to end on tiny pickled data."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_stackgan_eval_gpu import _make_cfg  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
G_IMG_TOL = 1e-5                # DESIGN §4.23 / tests/test_gancls_real_gpu.py: the eval-mode generator against float64, of max |ref|


def _seed(s):
    np.random.seed(s); random.seed(s); torch.manual_seed(s)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _batch(N, h, C, seed, first=0):
    """Image i is of kind (i + first) % 4: seeded normal data scaled into [-1, 1] (0) or well beyond it (3), a constant image (1),
    a flat image whose minimum sits in the first pixel and whose maximum is the very last element (2)."""
    rng = np.random.default_rng(seed)
    x = np.empty((N, h, h, C), np.float32)
    for i in range(N):
        kind = (i + first) % 4
        if kind == 0:
            x[i] = np.clip(rng.standard_normal((h, h, C)) * 0.4, -1, 1)
        elif kind == 3:
            x[i] = rng.standard_normal((h, h, C)) * 1.6 + 0.2
        elif kind == 1:
            x[i] = np.float32(rng.uniform(-1, 1))
        else:
            x[i] = rng.uniform(-0.25, 0.25, (h, h, C))
            x[i, 0, 0, 0] = -0.93
            x[i].reshape(-1)[-1] = 0.97
    return x


def _check_kernel(x, size):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.utils.visualize import stage_imgs_host
    xd = torch.from_numpy(x).to(DEV)
    got = K.bytescale_nearest(xd, size)
    again = K.bytescale_nearest(xd, size)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (x.shape[0], size, size, x.shape[3])
    assert torch.equal(got, again)                                        # no atomics: identical bytes from call to call
    want = stage_imgs_host(x, size)
    bad = int((got.cpu().numpy() != want).sum())
    assert bad == 0, '%d of %d bytes differ (x %s -> %d)' % (bad, want.size, x.shape, size)


@pytest.mark.parametrize('N', [1, 8, 64])
@pytest.mark.parametrize('h,size', [(64, 128), (256, 128), (4, 128), (38, 128), (128, 128), (256, 64)])
def test_bytescale_nearest_bit_for_bit(N, h, size):
    for first in (range(4) if N == 1 else (0,)):                          # a single image takes each kind in turn
        _check_kernel(_batch(N, h, 3, 1000 * N + h + size + first, first), size)


def test_bytescale_nearest_one_channel_and_odd_sizes():
    _check_kernel(_batch(8, 64, 1, 5), 128)
    _check_kernel(_batch(5, 5, 1, 6), 64)              # 25 elements per image: the scalar first pass and the byte-wise second
    _check_kernel(_batch(3, 37, 3, 7), 64)             # 4107 elements: images that start off a 16-byte boundary
    _check_kernel(_batch(4, 128, 3, 8), 256)           # 49152 elements: six whole chunks per image, upscaled


def test_bytescale_nearest_refuses_bad_arguments_before_any_launch():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib, kernels as K
    L = _lib.lib
    x = torch.from_numpy(_batch(2, 8, 3, 0)).to(DEV)
    y = torch.full((2, 16, 16, 3), 7, dtype=torch.uint8, device=DEV)
    need = int(L.t2i_bytescale_nearest_workspace_bytes(2, 8, 8, 3))
    assert need > 0
    ws = torch.zeros(max(need, 256), dtype=torch.uint8, device=DEV)
    px, py, pw = (ctypes.c_void_p(t.data_ptr()) for t in (x, y, ws))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(x=px, N=2, h=8, w=8, C=3, size=16, y=py, ws=pw, ws_bytes=need)
    cases = [dict(x=None), dict(y=None), dict(ws=None), dict(N=0), dict(N=-1), dict(h=0), dict(w=0), dict(size=0), dict(size=-4),
             dict(C=0), dict(C=5), dict(ws_bytes=need - 1), dict(ws_bytes=0)]
    for change in cases:
        a = dict(good, **change)
        rc = L.t2i_bytescale_nearest(a['x'], a['N'], a['h'], a['w'], a['C'], a['size'], a['y'], a['ws'], a['ws_bytes'], stream)
        assert rc != 0, change
        assert b't2i_bytescale_nearest' in L.t2i_last_error(), change
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and bool((ws == 0).all())                 # nothing was launched: neither buffer was written
    assert L.t2i_bytescale_nearest(px, 2, 8, 8, 3, 16, py, pw, need, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, K.bytescale_nearest(x, 16))


# ---- the generators' inference norms -------------------------------------------------------------------------------------------
def _models(cfg1_path, cfg2_path, B, widths):
    """Both generators over oracle-initialised variables with moving statistics that are not the identity.
    -> (Stage-II model (its .stagei is Stage I), the float64 variables, the oracle configs)."""
    from collections import OrderedDict
    import t2i_amd  # noqa: F401
    from oracle import torch_stackgan as SG
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan as S1
    from t2i_amd.models.stackgan.stageII.model import ConditionalGan as S2
    from t2i_amd.utils.config import config_from_yaml
    c1, c2 = config_from_yaml(cfg1_path), config_from_yaml(cfg2_path)
    c1.TRAIN.BATCH_SIZE = c2.TRAIN.BATCH_SIZE = B
    for c in (c1, c2):
        for k, v in widths.items():
            c.MODEL[k] = v
    m = S2(S1(c1, build_model=False, device=DEV), c2, build_model=False)
    with K_dry(), torch.no_grad():
        z = torch.empty(B, c1.MODEL.Z_DIM, device=DEV)
        phi = torch.empty(B, c1.MODEL.EMBED_DIM, device=DEV)
        img64, _, _ = m.stagei.generator(z, phi, reuse=False, is_training=False)
        m.generator(img64, phi, reuse=False, is_training=False)
    o1 = SG.Cfg(z_dim=c1.MODEL.Z_DIM, embed_dim=c1.MODEL.EMBED_DIM, compressed=c1.MODEL.COMPRESSED_EMBED_DIM, gf=c1.MODEL.GF_DIM,
                df=c1.MODEL.DF_DIM, batch=B)
    o2 = SG.Cfg(z_dim=c2.MODEL.Z_DIM, embed_dim=c2.MODEL.EMBED_DIM, compressed=c2.MODEL.COMPRESSED_EMBED_DIM, gf=c2.MODEL.GF_DIM,
                df=c2.MODEL.DF_DIM, batch=B, out_size=256)
    init = SG.init_variables(o2, stage=2, cfg1=o1, seed=0, dtype=torch.float32)
    rng = np.random.default_rng(3)
    values = {}
    for n, v in init.items():
        if n not in m.store.vars:
            continue                                                     # the discriminator's: neither generator reads them
        a = v.numpy()
        if n.endswith('moving_mean'):
            a = (rng.standard_normal(a.shape) * 0.1).astype(np.float32)
        elif n.endswith('moving_variance'):
            a = rng.uniform(0.8, 1.25, a.shape).astype(np.float32)
        values[n] = a
    assert set(values) == set(m.store.vars)
    m.store.load(values)
    P = OrderedDict((n, v.detach().double().cpu()) for n, v in m.store.vars.items())
    return m, P, o1, o2


def K_dry():
    from t2i_amd import kernels as K
    return K.dry_run()


@pytest.mark.parametrize('width', ['reduced', 'full'])
def test_eval_generators_fused_and_unfused_match_float64(width):
    """The Stage-I generator and the chain Stage I -> Stage II at B = 8 in eval mode, conditioning noise off, on the fused and on the
    unfused norm path, each against oracle.torch_stackgan's float64 eval-mode generators over the same variables and moving
    statistics; and the fused pass is the shorter launch sequence.
    Measured on an MI355X (max |got - ref| over the tanh output, max |ref| ~ 1): see DESIGN §4.24."""
    from bench_incep_train import count_launches
    from oracle import torch_stackgan as SG
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan as S1
    from t2i_amd.models.stackgan.stageII.model import ConditionalGan as S2
    cfgs = os.path.join(ROOT, 'text-to-image_amd', 'models', 'stackgan')
    widths = dict(Z_DIM=8, EMBED_DIM=32, COMPRESSED_EMBED_DIM=16, GF_DIM=8, DF_DIM=8) if width == 'reduced' else {}
    B = 8
    m, P, o1, o2 = _models(os.path.join(cfgs, 'stageI', 'cfg', 'flowers.yml'), os.path.join(cfgs, 'stageII', 'cfg', 'flowers.yml'), B, widths)
    assert S1.fused_infer is True and S2.fused_infer is True             # the default both samplers, evaluators and visualisers get
    rng = np.random.default_rng(5)
    z64 = torch.tensor(rng.standard_normal((B, o1.z_dim)))
    c64 = torch.tensor(rng.standard_normal((B, o1.embed_dim)))
    with torch.no_grad():
        V = SG.Vars(P)
        ref1, _, _ = SG.stage1_generator(V, o1, z64, c64, None, train=False)
        ref2, _, _ = SG.stage2_generator(V, o2, ref1, c64, None, train=False)
    ref1, ref2 = ref1.numpy(), ref2.numpy()
    z, cond = z64.float().to(DEV), c64.float().to(DEV)

    def stage_i():
        with torch.no_grad():
            return m.stagei.generator(z, cond, reuse=True, is_training=False, cond_noise=False)[0]

    def chain():
        with torch.no_grad():
            return m.generator(stage_i(), cond, reuse=True, is_training=False, cond_noise=False)[0]

    got, launches = {}, {}
    for fused in (True, False):
        m.fused_infer = m.stagei.fused_infer = fused
        got[fused] = (stage_i().double().cpu().numpy(), chain().double().cpu().numpy())
        launches[fused] = (count_launches(stage_i), count_launches(chain))
    m.fused_infer = m.stagei.fused_infer = True
    assert tuple(got[True][0].shape) == (B, 64, 64, 3) and tuple(got[True][1].shape) == (B, 256, 256, 3)
    errs = {}
    for fused in (True, False):
        for name, g, ref in (('stage I', got[fused][0], ref1), ('chain', got[fused][1], ref2)):
            scale = float(np.abs(ref).max())
            assert scale > 1e-3
            errs[(name, fused)] = float(np.abs(g - ref).max()) / scale
    print('eval-mode StackGAN generators, %s width, B=8, against float64 (of max |ref|): ' % width
          + ', '.join('%s %s %.2e' % (n, 'fused' if f else 'unfused', e) for (n, f), e in sorted(errs.items()))
          + '; launches per pass (stage I, chain): fused %s, unfused %s' % (launches[True], launches[False]))
    for key, e in errs.items():
        assert e <= G_IMG_TOL, (key, e, errs)
    for i in (0, 1):
        assert launches[True][i] is not None and launches[False][i] is not None
        assert launches[True][i] < launches[False][i], launches


# ---- the visualisers, end to end -----------------------------------------------------------------------------------------------
N_TRAIN, N_TEST, BATCH = 12, 9, 8
SPECIAL_SMALL = [8, 3, 0]


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """Stage I trained 3 updates at batch 8 on 12 train / 9 test images (76 x 76), then Stage II 3 updates (304 x 304) on top."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.stackgan.stageI import run as run1
    from t2i_amd.models.stackgan.stageII import run as run2
    root = str(tmp_path_factory.mktemp('stackgan_vis'))
    p1, c1 = _make_cfg(root, 'stageI', N_TRAIN, N_TEST, BATCH, SAMPLE_PERIOD=2, CHECKPOINT_PERIOD=2)
    p2, c2 = _make_cfg(root, 'stageII', N_TRAIN, N_TEST, BATCH, SAMPLE_PERIOD=2, CHECKPOINT_PERIOD=2)
    _seed(0)
    run1.main(['--cfg', p1, '--train', '--steps', '3', '--graphs', '0'])
    _seed(1)
    run2.main(['--cfg_stage_I', p1, '--cfg', p2, '--train', '--steps', '3', '--graphs', '0'])
    torch.cuda.synchronize()
    assert os.path.isfile(os.path.join(c1['CHECKPOINT_DIR'], 'checkpoint')) and os.path.isfile(os.path.join(c2['CHECKPOINT_DIR'], 'checkpoint'))
    return dict(root=root, p1=p1, c1=c1, p2=p2, c2=c2)


def _with_dirs(path, root, tag, **dirs):
    """A copy of the yml at `path` with some directories replaced."""
    cfg = yaml.safe_load(open(path))
    cfg.update(dirs)
    out = os.path.join(root, tag + '.yml')
    yaml.safe_dump(cfg, open(out, 'w'))
    return out


def _vis_cfgs(trained, tag):
    """Configs that write their sheets to a directory of their own."""
    root = trained['root']
    p1 = _with_dirs(trained['p1'], root, tag + '_s1', SAMPLE_DIR=os.path.join(root, tag, 's1') + '/')
    p2 = _with_dirs(trained['p2'], root, tag + '_s2', SAMPLE_DIR=os.path.join(root, tag, 's2') + '/')
    return p1, p2


def _check_neighbours(res, nb, cfg, orig, s):
    """float64 brute force over the train split with the returned crop table (tests/test_gancls_real_gpu.py's, at any size)."""
    import joblib
    from t2i_amd.utils.utils import denormalize_images
    train = np.asarray(joblib.load(os.path.join(cfg['DATASET_DIR'], 'train', '%dimages.pickle' % orig)))
    samples, (row0, col0, flip) = res['samples'], res['crops']
    Q, N = samples.shape[0], train.shape[0]
    assert Q == 8 and N == N_TRAIN and row0.shape == (Q, N) and samples.shape[1:] == (s, s, 3) and np.abs(samples).max() <= 1.0
    assert nb.shape == (3 * s, 8 * s, 3) and np.array_equal(nb, res['neighb'])                  # caption, samples, neighbours
    fake = samples.astype(np.float64)
    for q in range(Q):
        rows = row0[q][:, None] + np.arange(s)
        cols = np.where(flip[q][:, None] != 0, col0[q][:, None] + s - 1 - np.arange(s), col0[q][:, None] + np.arange(s))
        crops = train[np.arange(N)[:, None, None], rows[:, :, None], cols[:, None, :], :]
        real = (crops.astype(np.float32) * np.float32(2. / 255) - np.float32(1.)).astype(np.float64)
        j = int(np.argmin(((fake[q][None] - real) ** 2).sum(axis=(1, 2, 3))))
        assert res['neighbour_ids'][q] == j
        np.testing.assert_array_equal(res['neighbours'][q], real[j].astype(np.float32))
        np.testing.assert_array_equal(nb[s:2 * s, s * q:s * (q + 1)], denormalize_images(samples[q]))
        np.testing.assert_array_equal(nb[2 * s:3 * s, s * q:s * (q + 1)], denormalize_images(real[j].astype(np.float32)))


def _first_special_independently(stage, p1, p2, seed):
    """The first special-position batch by a fresh model and plain generator calls: the objects run.py --visualize builds, in its
    order, then the visualiser's draws replayed by hand.  -> host float32 [B, s, s, 3]."""
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan as S1
    from t2i_amd.models.stackgan.stageI.visualize_stagei import StageIVisualizer
    from t2i_amd.models.stackgan.stageII.model import ConditionalGan as S2
    from t2i_amd.models.stackgan.stageII.visualize_stageii import StageIIVisualizer
    from t2i_amd.models.wgancls.run import load_dataset
    from t2i_amd.utils.config import config_from_yaml
    _seed(seed)
    if stage == 1:
        cfg = config_from_yaml(p1)
        m = S1(cfg, build_model=False)
        vis = StageIVisualizer(None, m, load_dataset(cfg, m.device), cfg)
    else:
        cfg = config_from_yaml(p2)
        m = S2(S1(config_from_yaml(p1), build_model=False), cfg, build_model=False)
        vis = StageIIVisualizer(None, m, load_dataset(cfg, m.device), cfg)
    vis._restore_generator()
    test = vis.dataset.test
    np.random.randint(0, test.num_examples)                              # dataset_pos
    _, cond, _, _ = test.next_batch_test(1, SPECIAL_SMALL[0], 1)
    z = torch.as_tensor(np.random.standard_normal(size=(BATCH, 8)).astype(np.float32), device=DEV)
    cond = torch.as_tensor(np.tile(np.asarray(cond[0].cpu() if torch.is_tensor(cond[0]) else cond[0], np.float32).reshape(1, -1), (BATCH, 1)), device=DEV)
    with torch.no_grad():
        if stage == 1:
            img = m.generator(z, cond, reuse=True, is_training=False, cond_noise=True)[0]
        else:
            img64 = m.stagei.generator(z, cond, reuse=True, is_training=False)[0]
            img = m.generator(img64, cond, reuse=True, is_training=False, cond_noise=True)[0]
    return img.float().cpu().numpy()


def test_visualize_needs_the_special_positions_and_the_checkpoints(trained, monkeypatch):
    from t2i_amd.models.stackgan.stageI import run as run1, visualize_stagei as VS
    from t2i_amd.models.stackgan.stageII import run as run2
    p1, p2 = _vis_cfgs(trained, 'errors')
    with pytest.raises(ValueError, match='special test position 1126'):    # the flowers positions on a 9-image test split
        run1.main(['--cfg', p1, '--visualize'])
    with pytest.raises(ValueError, match='special test position 1126'):
        run2.main(['--cfg_stage_I', p1, '--cfg', p2, '--visualize'])
    monkeypatch.setitem(VS.SPECIAL, 'flowers', SPECIAL_SMALL)
    root = trained['root']
    e1 = _with_dirs(p1, root, 'empty_s1', CHECKPOINT_DIR=os.path.join(root, 'empty_ckpt_1') + '/')
    e2 = _with_dirs(p2, root, 'empty_s2', CHECKPOINT_DIR=os.path.join(root, 'empty_ckpt_2') + '/')
    with pytest.raises(LookupError, match=r'Could not load any checkpoints$'):
        run1.main(['--cfg', e1, '--visualize'])
    with pytest.raises(LookupError, match=r'Could not load any checkpoints for stage I$'):
        run2.main(['--cfg_stage_I', e1, '--cfg', p2, '--visualize'])
    with pytest.raises(LookupError, match=r'Could not load any checkpoints for stage II$'):
        run2.main(['--cfg_stage_I', p1, '--cfg', e2, '--visualize'])


def test_stage_i_visualize_end_to_end(trained, monkeypatch):
    from t2i_amd.models.stackgan.stageI import run as run1, visualize_stagei as VS
    from t2i_amd.utils.utils import denormalize_images
    monkeypatch.setitem(VS.SPECIAL, 'flowers', SPECIAL_SMALL)
    p1, p2 = _vis_cfgs(trained, 'stage1')
    _seed(5)
    res = run1.main(['--cfg', p1, '--visualize'])
    vis = os.path.join(trained['root'], 'stage1', 's1', 'data_visual')
    assert sorted(os.listdir(vis)) == ['neighb', 'special_cap']
    assert sorted(os.listdir(os.path.join(vis, 'special_cap'))) == ['cap0.png', 'cap1.png', 'cap2.png']
    for i in range(3):
        im = np.array(Image.open(os.path.join(vis, 'special_cap', 'cap%d.png' % i)))
        assert im.shape == (2 * 64, 8 * 64, 3) and np.array_equal(im, res['special_cap'][i])      # caption row + 8 images
        assert np.any(im[:64] != 255)
    want = _first_special_independently(1, p1, p2, 5)
    sheet = res['special_cap'][0]
    for q in range(8):
        np.testing.assert_array_equal(sheet[64:128, 64 * q:64 * (q + 1)], denormalize_images(want[q]))
    nb = np.array(Image.open(os.path.join(vis, 'neighb', 'neighb.png')))
    _check_neighbours(res, nb, trained['c1'], 76, 64)
    # --interp 2 adds the interpolation and captioned sheets, two of each
    run1.main(['--cfg', p1, '--visualize', '--interp', '2'])
    assert sorted(os.listdir(vis)) == ['cap', 'cond_interp', 'neighb', 'special_cap', 'z_interp']
    for kind, shape in (('z_interp', (128, 512, 3)), ('cond_interp', (192, 512, 3)), ('cap', (128, 512, 3))):
        assert sorted(os.listdir(os.path.join(vis, kind))) == ['%s%d.png' % (kind, i) for i in (0, 1)]
        assert np.array(Image.open(os.path.join(vis, kind, kind + '1.png'))).shape == shape


def test_stage_ii_visualize_end_to_end(trained, monkeypatch):
    from t2i_amd.models.stackgan.stageI import visualize_stagei as VS
    from t2i_amd.models.stackgan.stageII import run as run2
    from t2i_amd.utils import visualize as V
    from t2i_amd.utils.utils import denormalize_images
    monkeypatch.setitem(VS.SPECIAL, 'flowers', SPECIAL_SMALL)
    p1, p2 = _vis_cfgs(trained, 'stage2')
    # what the two generators of the stage sheet hand back, recorded on the way into gen_multiple_stage_img
    seen = []
    inner = V.gen_multiple_stage_img

    def recording(gens, cond, z_dim, batch_size, size=128):
        def wrap(gen):
            def g(z, c):
                out = gen(z, c)
                seen.append((np.array(z), np.array(V._host(out))))
                return out
            return g
        return inner([wrap(g) for g in gens], cond, z_dim, batch_size, size=size)
    monkeypatch.setattr(V, 'gen_multiple_stage_img', recording)
    _seed(7)
    res = run2.main(['--cfg_stage_I', p1, '--cfg', p2, '--visualize', '--interp', '1'])
    vis = os.path.join(trained['root'], 'stage2', 's2', 'data_visual')
    assert sorted(os.listdir(vis)) == ['cap', 'cond_interp', 'neighb', 'special_cap', 'stages', 'z_interp']
    for kind, names in (('cap', ['cap0.png']), ('cond_interp', ['cond_interp0.png']), ('z_interp', ['z_interp0.png']),
                        ('stages', ['stage0.png']), ('special_cap', ['cap0.png', 'cap1.png', 'cap2.png']), ('neighb', ['neighb.png'])):
        assert sorted(os.listdir(os.path.join(vis, kind))) == names, kind
    for kind, name, shape in (('z_interp', 'z_interp0', (512, 2048, 3)), ('cond_interp', 'cond_interp0', (768, 2048, 3)),
                              ('cap', 'cap0', (512, 2048, 3)), ('special_cap', 'cap2', (512, 2048, 3))):
        assert np.array(Image.open(os.path.join(vis, kind, name + '.png'))).shape == shape
    # the stage sheet: a caption row, 8 Stage-I images, the 8 chain images of the same z, all 128 x 128
    st = np.array(Image.open(os.path.join(vis, 'stages', 'stage0.png')))
    assert st.shape == (3 * 128, 8 * 128, 3) and np.array_equal(st, res['stages'][0])
    assert len(seen) == 2 and np.array_equal(seen[0][0], seen[1][0])                              # one z draw for both generators
    assert seen[0][1].shape == (BATCH, 64, 64, 3) and seen[1][1].shape == (BATCH, 256, 256, 3)
    for row, (_, imgs) in enumerate(seen):
        want = denormalize_images(V.stage_imgs_host(imgs[:8], 128) / 127.5 - 1.0)
        for q in range(8):
            np.testing.assert_array_equal(st[128 * (row + 1):128 * (row + 2), 128 * q:128 * (q + 1)], want[q])
    nb = np.array(Image.open(os.path.join(vis, 'neighb', 'neighb.png')))
    _check_neighbours(res, nb, trained['c2'], 304, 256)
    # the special sheets of a run without rounds equal an independent chain call
    _seed(9)
    res = run2.main(['--cfg_stage_I', p1, '--cfg', p2, '--visualize'])
    want = _first_special_independently(2, p1, p2, 9)
    sheet = res['special_cap'][0]
    for q in range(8):
        np.testing.assert_array_equal(sheet[256:512, 256 * q:256 * (q + 1)], denormalize_images(want[q]))
