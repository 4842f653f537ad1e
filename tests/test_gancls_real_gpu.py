"""GAN-CLS on (tiny, fabricated) real data, on the GPU: the one-launch inference batch norm (t2i_bn_infer) against its float64
statement, the eval-mode generator at full width on the fused and on the unfused norm path against the float64 oracle, the
trainer's side effects and exact resume, the evaluator (IS / FID / IMD) and the caption visualiser."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_eval_gpu import inception  # noqa: E402,F401
from test_gancls_real_host import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, np_bn_infer  # noqa: E402
from test_visualize import _write_split  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
FWD_TOL = 1e-5                  # tests/test_kernels_gpu.py:13 — the project's forward bound against float64 (what bn_apply is held to there)
BF16_REL = 2.0 ** -8            # one round-to-nearest bf16 rounding of the float64 result (8 significand bits: half an ulp <= 2^-8 relative)
G_IMG_TOL = 1e-5                # tests/test_fullsize_gpu.py: _cgan_steps(img_tol=1e-5) — GAN-CLS's forward ('G (tanh output)', scale 1.0)
N_TRAIN, N_TEST, BATCH = 24, 70, 8


def relerr(got, ref):
    """tests/test_kernels_gpu.py:42 — max |got - ref| / max |ref|."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
GEN_NORMS = [(4, 4, 1024), (4, 4, 256), (8, 8, 512), (8, 8, 128), (16, 16, 256), (32, 32, 128)]      # every rank-4 norm of the generator
ODD_SHAPES = [(3, 5, 7, 128),        # 105 rows: not a multiple of the 32 rows a workgroup takes at C = 128
              (5, 3, 3, 6),          # C % 4 != 0: the scalar form
              (3, 1030),             # C % 4 != 0 and two channel tiles
              (2, 2052),             # three channel tiles, the last one 4 channels wide
              (7, 4, 4, 1024)]


def _bn_case(shape, seed, dtype):
    rng = np.random.default_rng(seed)
    C = shape[-1]
    x = (rng.standard_normal(shape) * 2 + 0.5).astype(np.float32)
    r = rng.standard_normal(shape).astype(np.float32)
    vec = [a.astype(np.float32) for a in (1 + 0.3 * rng.standard_normal(C), 0.2 * rng.standard_normal(C), 0.5 * rng.standard_normal(C),
                                          rng.uniform(0.3, 3.0, C))]
    xd, rd = torch.from_numpy(x).to(DEV).to(dtype), torch.from_numpy(r).to(DEV).to(dtype)
    return xd, rd, [torch.from_numpy(v).to(DEV) for v in vec], xd.double().cpu().numpy(), rd.double().cpu().numpy(), vec


def _check_bn(K, shape, dtype, seed):
    xd, rd, vd, x, r, v = _bn_case(shape, seed, dtype)
    worst = 0.0
    for act, res, res_act in ((ACT_NONE, False, ACT_NONE), (ACT_RELU, False, ACT_NONE), (ACT_LRELU, False, ACT_NONE), (ACT_TANH, False, ACT_NONE),
                              (ACT_NONE, True, ACT_RELU), (ACT_RELU, True, ACT_LRELU), (ACT_TANH, True, ACT_NONE), (ACT_LRELU, True, ACT_TANH)):
        got = K.bn_infer(xd, *vd, 1e-5, act, 0.2, rd if res else None, res_act, 0.1)
        ref = np_bn_infer(x, *v, 1e-5, act, 0.2, r if res else None, res_act, 0.1)
        assert got.dtype == dtype and tuple(got.shape) == tuple(shape)
        g = got.double().cpu().numpy()
        scale = max(np.abs(ref).max(), 1e-30)
        if dtype == torch.float32:
            err = float(np.abs(g - ref).max() / scale)
            assert err <= FWD_TOL, (shape, act, res, res_act, err)
        else:
            # the float64 result rounded once to bf16, of a value that itself is within the fp32 bound
            over = np.abs(g - ref) - (BF16_REL * np.abs(ref) + FWD_TOL * scale)
            err = float(np.abs(g - ref).max() / scale)
            assert over.max() <= 0.0, (shape, act, res, res_act, float(over.max()), err)
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize('B', [8, 64])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_bn_infer_generator_norm_shapes(B, dtype):
    """Every norm of the eval-mode generator at full width — rank 4 and the rank-2 [B, 16384] of the dense layer — with and without
    residual, every activation."""
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    for i, hwc in enumerate(GEN_NORMS + [(16384,)]):
        err = _check_bn(K, (B,) + hwc, dtype, 100 * B + i)
        print('bn_infer %s B=%d %s: max error %.2e of max |ref|' % (hwc, B, dtype, err))


@pytest.mark.parametrize('shape', ODD_SHAPES, ids=[str(s) for s in ODD_SHAPES])
def test_bn_infer_tails_and_scalar_form(shape):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    _check_bn(K, shape, torch.float32, len(shape) + shape[-1])
    if shape[-1] % 4 == 0:
        _check_bn(K, shape, torch.bfloat16, 7 + shape[-1])
    else:
        x = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
        v = [torch.ones(shape[-1], device=DEV)] * 4
        from t2i_amd._lib import T2IError
        with pytest.raises(T2IError, match='bf16 tensors need'):
            K.bn_infer(x, *v)


def test_bn_infer_equals_the_unfused_path_through_ops():
    """ops.batch_norm(fused_infer=True[, residual]) against batch_norm(train=False) + add: the same variables, FWD_TOL apart; the unfused
    path is unchanged by the flag's existence (bit-equal to its own restatement)."""
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K, scope as S
    from t2i_amd.utils import ops
    st = S.set_default_store(S.VariableStore(device=DEV, seed=0))
    x = torch.randn(4, 8, 8, 64, device=DEV)
    r = torch.randn(4, 8, 8, 64, device=DEV)
    with torch.no_grad(), S.variable_scope('t', reuse=False):
        ops.batch_norm(x, train=False, name='bn')
    for n, v in st.vars.items():
        with torch.no_grad():
            v.copy_(torch.rand_like(v) + 0.5)
    with torch.no_grad(), S.variable_scope('t', reuse=True):
        old = ops.add(r, ops.batch_norm(x, train=False, name='bn', act=None), act=ops.relu)
        new = ops.batch_norm(x, train=False, name='bn', act=None, fused_infer=True, residual=r, res_act=ops.relu)
        plain_old = ops.batch_norm(x, train=False, name='bn', act=ops.lrelu_act(0.2))
        plain_new = ops.batch_norm(x, train=False, name='bn', act=ops.lrelu_act(0.2), fused_infer=True)
    g, b, mm, mv = (st.vars['t/bn/' + k] for k in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
    scale = g / torch.sqrt(mv + 1e-5)
    assert torch.equal(plain_old, K.bn_apply(x, scale.contiguous(), (b - mm * scale).contiguous(), K.ACT_LRELU, 0.2))
    assert relerr(new, old.double().cpu().numpy()) <= FWD_TOL and relerr(plain_new, plain_old.double().cpu().numpy()) <= FWD_TOL
    with pytest.raises(ValueError, match='fused_infer'):
        with S.variable_scope('t', reuse=True):
            ops.batch_norm(x, train=True, name='bn', fused_infer=True)


# ---- the generator at full width -------------------------------------------------------------------------------------------------
def test_eval_generator_full_width_fused_and_unfused_match_float64():
    """GF 128, z 100, B = 8 (the yml): two training iterations move every moving average, then the eval-mode generator on the fused
    and on the unfused norm path against oracle.torch_gancls.generator(train=False) in float64 over the same variables."""
    from collections import OrderedDict
    import t2i_amd  # noqa: F401
    from oracle import torch_gancls as GC
    from t2i_amd.models.gancls.model import GanCls
    from t2i_amd.models.gancls.trainer import GanClsTrainer
    from t2i_amd.utils.config import config_from_yaml
    cfg = config_from_yaml(os.path.join(ROOT, 'text-to-image_amd', 'models', 'gancls', 'cfg', 'flowers.yml'))
    B = 8
    cfg.TRAIN.BATCH_SIZE = B
    ocfg = GC.Cfg(batch=B)
    m = GanCls(cfg, device=DEV)
    m.store.load({n: v.numpy() for n, v in GC.init_variables(ocfg, seed=0, dtype=torch.float32).items()})
    f = {k: v.to(DEV) for k, v in GC.synthetic_feed(ocfg, seed=1, dtype=torch.float32).items()}
    hf = {'inputs': f['x'], 'wrong_inputs': f['x_mismatch'], 'phi_inputs': f['cond'], 'z': f['z']}
    tr = GanClsTrainer(None, m, None, cfg)
    for _ in range(2):
        tr.iteration(hf)
    torch.cuda.synchronize()
    mm = m.store.vars['g_net/BatchNorm_4/moving_mean'].detach().cpu().numpy()
    mv = m.store.vars['g_net/BatchNorm_4/moving_variance'].detach().cpu().numpy()
    assert np.abs(mm).max() > 1e-4 and np.abs(mv - 1).max() > 1e-3           # the statistics have moved
    P = OrderedDict((n, v.detach().double().cpu()) for n, v in m.store.vars.items())
    ev = GC.synthetic_feed(ocfg, seed=5, dtype=torch.float64)
    with torch.no_grad():
        ref = GC.generator(P, ocfg, ev['z'], ev['cond'], train=False).numpy()
    z, cond = ev['z'].float().to(DEV), ev['cond'].float().to(DEV)
    assert GanCls.fused_infer is True
    fused = m.sampler(z, cond)
    m.fused_infer = False
    unfused = m.sampler(z, cond)
    m.fused_infer = True
    e_f = float(np.abs(fused.double().cpu().numpy() - ref).max())
    e_u = float(np.abs(unfused.double().cpu().numpy() - ref).max())
    print('eval-mode generator B=8 against float64: fused %.2e, unfused %.2e (absolute; tanh output, scale 1)' % (e_f, e_u))
    assert np.abs(ref).max() > 1e-3
    assert e_u <= G_IMG_TOL, e_u
    assert e_f <= G_IMG_TOL, e_f


# ---- a tiny pickled data set, trained to the first periodic checkpoint ----------------------------------------------------------
def _make_cfg(root, ckpt='ckpt', **eval_keys):
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'text-to-image_amd', 'models', 'gancls', 'cfg', 'flowers.yml')))
    cfg.update(DATASET_DIR=root + '/data/flowers/', CHECKPOINT_DIR=root + '/%s/' % ckpt, LOGS_DIR=root + '/logs/', SAMPLE_DIR=root + '/samples/')
    cfg['MODEL'].update(Z_DIM=8, EMBED_DIM=32, COMPRESSED_EMBED_DIM=16, GF_DIM=8, DF_DIM=8)
    cfg['TRAIN'].update(FLAG=False, BATCH_SIZE=BATCH, SAMPLE_NUM=64)
    cfg['EVAL'].update(**eval_keys)
    path = os.path.join(root, 'gancls_%d.yml' % len([n for n in os.listdir(root) if n.endswith('.yml')]))
    yaml.safe_dump(cfg, open(path, 'w'))
    return path, cfg


def _seed(s):
    np.random.seed(s); random.seed(s); torch.manual_seed(s)


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """run.py --train --steps 501 on 24 train / 70 test images at batch 8: 3 updates per epoch, counter 100 ... 500 write grids,
    counter 2 and 502 write checkpoints, and the run stops right behind the checkpoint of counter 502."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.gancls import run
    root = str(tmp_path_factory.mktemp('gancls'))
    rng = np.random.default_rng(0)
    _write_split(root + '/data/flowers', 'train', N_TRAIN, rng, 32)
    _write_split(root + '/data/flowers', 'test', N_TEST, rng, 32)
    path, cfg = _make_cfg(root)
    _seed(0)
    trainer = run.main(['--cfg', path, '--train', '--steps', '501'])
    torch.cuda.synchronize()
    return dict(root=root, path=path, cfg=cfg, trainer=trainer)


def test_train_side_effects(trained):
    cfg = trained['cfg']
    upe = N_TRAIN // BATCH
    grids = sorted(n for n in os.listdir(cfg['SAMPLE_DIR']) if n.endswith('.png'))
    want = ['train_%02d_%04d.png' % divmod(c - 2, upe) for c in (100, 200, 300, 400, 500)]     # counter c is reached behind update c - 2 (0-based)
    assert grids == sorted(want), grids
    grid = np.asarray(Image.open(os.path.join(cfg['SAMPLE_DIR'], want[0])))
    assert grid.shape == (8 * 64, 8 * 64, 3) and grid.std() > 0                                 # 64 samples, 8 x 8
    assert sorted(os.listdir(cfg['CHECKPOINT_DIR'])) == ['checkpoint', 'model-2.npz', 'model-502.npz']
    assert 'model-502.npz' in open(os.path.join(cfg['CHECKPOINT_DIR'], 'checkpoint')).read()
    z = np.load(os.path.join(cfg['CHECKPOINT_DIR'], 'model-502.npz'))
    from oracle import torch_gancls as GC
    names = set(GC.variable_shapes(GC.Cfg(z_dim=8, embed_dim=32, compressed=16, gf=8, df=8)))
    assert names <= set(z.files)                                  # every global variable under the reference's tf.layers name
    for key in ('g_net/BatchNorm/moving_mean', 'd_net/BatchNorm_6/moving_variance', 'G_optim/g_net/conv2d_3/kernel/Adam',
                'G_optim/g_net/conv2d_3/kernel/Adam_1', 'D_optim/d_net/conv2d/kernel/Adam', 'D_optim/t', 'G_optim/t'):
        assert key in z.files, key
    assert int(z['D_optim/t']) == 501 and int(z['G_optim/t']) == 501
    assert np.abs(z['g_net/BatchNorm/moving_mean']).max() > 0 and np.abs(z['G_optim/g_net/conv2d_3/kernel/Adam']).max() > 0
    tr = trained['trainer']
    assert getattr(tr, '_graphs', None) is not None and tr.start_counter == 1


def _restart_data_at_first_feed(tr, ds, seed):
    """The data order and every seed of the run, restored right in front of the next batch: the reference checkpoints neither, so both arms of
    the resume comparison restart them at the checkpoint."""
    make_feed = tr.make_feed

    def first():
        _seed(seed)
        tr.gen.manual_seed(seed)
        ds.train._perm = np.arange(ds.train.num_examples)
        ds.train._index_in_epoch = 0
        tr.make_feed = make_feed
        return make_feed()
    tr.make_feed = first


def test_resume_is_exact(trained):
    """501 + 7 updates in one run against 501 updates, a checkpoint, and 7 updates by fresh objects that load it: every variable,
    both Adam moments and the step counts bit-identical."""
    from t2i_amd.models.gancls.model import GanCls
    from t2i_amd.models.gancls.trainer import GanClsTrainer
    from t2i_amd.models.wgancls.run import load_dataset
    from t2i_amd.utils.config import config_from_yaml
    quiet = lambda s: None  # noqa: E731
    from t2i_amd import scope as S
    a = trained['trainer']
    S.set_default_store(a.model.store)
    _restart_data_at_first_feed(a, a.dataset, 77)
    a.train(max_updates=7, log=quiet, graphs=True)                   # continues in memory: nothing is read back
    torch.cuda.synchronize()
    cfg = config_from_yaml(trained['path'])
    _seed(123)
    m = GanCls(cfg)
    ds = load_dataset(cfg, m.device)
    b = GanClsTrainer(None, m, ds, cfg)
    _restart_data_at_first_feed(b, ds, 77)
    b.train(max_updates=7, log=quiet, side_effects=True, graphs=True)
    torch.cuda.synchronize()
    assert b.start_counter == 502 and m is not a.model
    assert list(m.store.vars) == list(a.model.store.vars)
    for n, v in m.store.vars.items():
        assert torch.equal(v, a.model.store.vars[n]), n
    for oa, ob in ((a.D_optim, b.D_optim), (a.G_optim, b.G_optim)):
        assert oa.t == ob.t == 508 and torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v)
    assert sorted(os.listdir(cfg.CHECKPOINT_DIR)) == ['checkpoint', 'model-2.npz', 'model-502.npz']      # nothing new was due


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eval_cfg(trained, inception):  # noqa: F811
    arrays = dict(inception[0])
    arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] = arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] * np.float32(0.05)
    root = trained['root']
    incep_dir = os.path.join(root, 'incep')
    os.makedirs(incep_dir)
    np.savez(os.path.join(incep_dir, 'model-7.npz'), **arrays)
    open(os.path.join(incep_dir, 'checkpoint'), 'w').write('model_checkpoint_path: "model-7.npz"\n')
    real_dir = os.path.join(root, 'real', 'jpg')
    os.makedirs(real_dir)
    rng = np.random.default_rng(11)
    for i, shape in enumerate([(80, 100, 3), (64, 64, 3), (70, 90), (120, 77, 3), (66, 66, 3)]):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(os.path.join(real_dir, 'image_%d.jpg' % i), quality=95)
    return _make_cfg(root, INCEP_CHECKPOINT_DIR=incep_dir + '/', SAMPLE_SIZE=8, SIZE=16, INCEP_BATCH_SIZE=4, NUM_CLASSES=20,
                     ACT_STAT_PATH=os.path.join(root, 'fid', 'stats.npz'), R_IMG_PATH=os.path.join(root, 'real'))


def _evaluator(eval_cfg, seed, fused=True):
    """The objects run.py --eval builds, in its order (so that equal seeds give equal draws)."""
    from t2i_amd.models.gancls.eval_gancls import GanClsEval
    from t2i_amd.models.gancls.model import GanCls
    from t2i_amd.models.wgancls.run import load_dataset
    from t2i_amd.utils.config import config_from_yaml
    _seed(seed)
    cfg = config_from_yaml(eval_cfg[0])
    m = GanCls(cfg, build_model=False)
    m.fused_infer = fused
    return GanClsEval(sess=None, model=m, dataset=load_dataset(cfg, m.device), cfg=cfg)


def test_eval_inception_equals_scoring_the_unfused_images(eval_cfg):
    from t2i_amd.evaluation import inception_score
    from t2i_amd.models.gancls import run
    _seed(3)
    r = run.main(['--cfg', eval_cfg[0], '--eval', 'is'])
    assert np.isfinite(r['mean']) and np.isfinite(r['std']) and r['mean'] >= 1.0 - 1e-9 and sorted(r['indices']) == list(range(16))
    ev = _evaluator(eval_cfg, 3, fused=False)             # the same draws, the generator on the unfused norm path
    net = ev._inception()
    ev.restore()
    samples = ev._generate(is_training=False)
    assert tuple(samples.shape) == (16, 64, 64, 3)
    m, s, idx = inception_score.get_inception_score(samples, net, 4, 10)
    print('IS fused %r / %r, unfused images scored directly %r / %r; images differ by %.2e' % (
        r['mean'], r['std'], m, s, float((samples - r['samples']).abs().max())))
    assert list(idx) == list(r['indices'])
    # tests/test_eval_gpu.py:299 — the tolerance the wgancls evaluator is held to
    assert abs(r['mean'] - m) <= 1e-4 * abs(m) and abs(r['std'] - s) <= 1e-4 * max(abs(s), 1e-3), (r['mean'], m, r['std'], s)


def test_eval_fid_runs_the_generator_in_training_mode(eval_cfg):
    ev = _evaluator(eval_cfg, 4)
    f = ev.evaluate_fid()
    assert np.isfinite(f['fid']) and os.path.exists(eval_cfg[1]['EVAL']['ACT_STAT_PATH'])
    ck = np.load(os.path.join(eval_cfg[1]['CHECKPOINT_DIR'], 'model-502.npz'))
    for n in ('g_net/BatchNorm/moving_mean', 'g_net/BatchNorm_9/moving_variance'):
        assert np.array_equal(ev.model.store.vars[n].detach().cpu().numpy(), ck[n]), n           # no update op ran
    ev2 = _evaluator(eval_cfg, 4)
    ev2.restore()
    eval_mode = ev2._generate(is_training=False)           # the same draws through the moving statistics
    assert tuple(eval_mode.shape) == tuple(f['samples'].shape) == (16, 64, 64, 3)
    assert float((eval_mode - f['samples']).abs().max()) > 1e-3
    ev3 = _evaluator(eval_cfg, 4)
    ev3.restore()
    assert torch.equal(ev3._generate(is_training=True), f['samples'])


def test_eval_imd_returns_one_distance_per_pair(eval_cfg):
    from t2i_amd.models.gancls import run
    _seed(5)
    r = run.main(['--cfg', eval_cfg[0], '--eval', 'imd', '--incep-batch', '4'])
    d = r['distances']
    assert d.shape == (2 * 8,) and d.dtype == np.float64 and np.isfinite(d).all() and (d >= -1e-12).all() and (d <= 2 + 1e-12).all()
    assert r['mean'] == float(np.mean(d)) and r['std'] == float(np.std(d))


# ---- the visualiser --------------------------------------------------------------------------------------------------------------
def test_visualize_needs_a_checkpoint_and_the_special_positions(trained, monkeypatch):
    from t2i_amd.models.gancls import run, visualize_gancls as VG
    with pytest.raises(ValueError, match='1126'):                        # the reference's positions on a 70-image test split
        run.main(['--cfg', trained['path'], '--visualize'])
    monkeypatch.setattr(VG, 'SPECIAL_POSITIONS', (69, 33, 0))
    empty, _ = _make_cfg(trained['root'], ckpt='empty_ckpt')
    with pytest.raises(LookupError, match='Could not load any checkpoints'):
        run.main(['--cfg', empty, '--visualize'])


def test_visualize_writes_the_sheets_and_the_nearest_train_images(trained, monkeypatch):
    import joblib
    from t2i_amd.models.gancls import run, visualize_gancls as VG
    from t2i_amd.utils.utils import denormalize_images
    monkeypatch.setattr(VG, 'SPECIAL_POSITIONS', (69, 33, 0))
    _seed(5)
    res = run.main(['--cfg', trained['path'], '--visualize'])
    vis = os.path.join(trained['cfg']['SAMPLE_DIR'], 'flowers_visual')
    assert sorted(os.listdir(vis)) == ['neighb', 'special_cap']
    for i in range(3):
        im = np.array(Image.open(os.path.join(vis, 'special_cap', 'cap%d.png' % i)))
        assert im.shape == (2 * 64, 8 * 64, 3) and np.array_equal(im, res['special_cap'][i])      # caption row + 8 images
        assert np.any(im[:64] != 255)
    nb = np.array(Image.open(os.path.join(vis, 'neighb', 'neighb.png')))
    assert nb.shape == (3 * 64, 8 * 64, 3) and np.array_equal(nb, res['neighb'])                  # caption, samples, neighbours
    # float64 brute force over the train split with the returned crop table
    train = np.asarray(joblib.load(os.path.join(trained['cfg']['DATASET_DIR'], 'train', '76images.pickle')))
    samples, (row0, col0, flip) = res['samples'], res['crops']
    Q, N = samples.shape[0], train.shape[0]
    assert Q == 8 and N == N_TRAIN and row0.shape == (Q, N) and np.abs(samples).max() <= 1.0
    fake = samples.astype(np.float64)
    for q in range(Q):
        rows = row0[q][:, None] + np.arange(64)
        cols = np.where(flip[q][:, None] != 0, col0[q][:, None] + 63 - np.arange(64), col0[q][:, None] + np.arange(64))
        crops = train[np.arange(N)[:, None, None], rows[:, :, None], cols[:, None, :], :]
        real = (crops.astype(np.float32) * np.float32(2. / 255) - np.float32(1.)).astype(np.float64)
        j = int(np.argmin(((fake[q][None] - real) ** 2).sum(axis=(1, 2, 3))))
        assert res['neighbour_ids'][q] == j
        np.testing.assert_array_equal(res['neighbours'][q], real[j].astype(np.float32))
        np.testing.assert_array_equal(nb[64:128, 64 * q:64 * (q + 1)], denormalize_images(samples[q]))
        np.testing.assert_array_equal(nb[128:192, 64 * q:64 * (q + 1)], denormalize_images(real[j].astype(np.float32)))
    # --interp 1 adds the interpolation and captioned sheets
    res = run.main(['--cfg', trained['path'], '--visualize', '--interp', '1'])
    for kind, name, shape in (('z_interp', 'z_interp0', (128, 512, 3)), ('cond_interp', 'cond_interp0', (192, 512, 3)),
                              ('cap', 'cap0', (128, 512, 3))):
        im = np.array(Image.open(os.path.join(vis, kind, name + '.png')))
        assert im.shape == shape and np.array_equal(im, res[kind][0])
