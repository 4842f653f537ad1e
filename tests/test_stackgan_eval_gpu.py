"""StackGAN trained and scored on (tiny) pickled data, on the GPU: t2i_cosine_distance against the float64 statement and scipy,
stageI/run.py and stageII/run.py --train with the reference's side effects (captions, grids, checkpoints, resume, the Stage-I
generator under Stage II), and --eval is|fid|imd of both stages against the float64 InceptionV3 oracle of test_eval_gpu.py."""
import os
import pickle
import random
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_eval_gpu import _Oracle, _np_prep, inception  # noqa: E402,F401

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
CFG = os.path.join(ROOT, 'text-to-image_amd', 'models', 'stackgan')


# ---- the cosine kernel -----------------------------------------------------------------------------------------------------
def _cos64(a, b):
    from t2i_amd.evaluation.imd import get_cosine_dist
    return get_cosine_dist(np.asarray(b, np.float64), np.asarray(a, np.float64))


@pytest.mark.parametrize('n', [1, 7, 64])
@pytest.mark.parametrize('d', [1, 3, 2048, 2050])
def test_cosine_kernel_matches_float64_statement(n, d):
    import t2i_amd  # noqa: F401
    from scipy.spatial import distance
    from t2i_amd import kernels as K
    rng = np.random.default_rng(n * 10000 + d)
    for pad in (0, 5):             # contiguous rows (16-byte reads where d % 4 == 0) and strided rows (ld = d + 5)
        A = (rng.standard_normal((n, d + pad)) + 0.3).astype(np.float32)
        B = (rng.standard_normal((n, d + pad)) + 0.3).astype(np.float32)
        if n > 1:
            B[1] = A[1]                                   # identical rows
        ad = torch.from_numpy(A).to(DEV)[:, :d]
        bd = torch.from_numpy(B).to(DEV)[:, :d]
        got = K.cosine_distance(ad, bd).cpu().numpy()
        want = _cos64(A[:, :d], B[:, :d])
        assert got.dtype == np.float64 and got.shape == (n,)
        assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
        if n > 1:
            assert got[1] <= 1e-15
        sp = np.array([distance.cosine(A[i, :d], B[i, :d]) for i in range(n)])
        assert np.abs(got - sp).max() <= 1e-5
        again = K.cosine_distance(ad, bd).cpu().numpy()
        assert np.array_equal(got.view(np.int64), again.view(np.int64))
    Z = torch.zeros((n, d), device=DEV)
    Z2 = torch.from_numpy(A[:, :d].copy()).to(DEV)
    assert np.isnan(K.cosine_distance(Z, Z2).cpu().numpy()).all()
    assert np.isnan(K.cosine_distance(Z2, Z).cpu().numpy()).all()


# ---- tiny pickled data and configs -------------------------------------------------------------------------------------------
def _write_split(root, split, n, rng, emb_dim, orig):
    import joblib
    path = os.path.join(root, split)
    os.makedirs(path)
    joblib.dump(list(rng.integers(0, 256, (n, orig, orig, 3), dtype=np.uint8)), os.path.join(path, '%dimages.pickle' % orig))
    pickle.dump(list(rng.standard_normal((n, 5, emb_dim)).astype(np.float32)), open(os.path.join(path, 'char-CNN-RNN-embeddings.pickle'), 'wb'))
    names = ['jpg/%s_%05d' % (split, i) for i in range(n)]
    classes = [int(c) for c in rng.integers(1, 6, n)]
    pickle.dump(names, open(os.path.join(path, 'filenames.pickle'), 'wb'))
    pickle.dump(classes, open(os.path.join(path, 'class_info.pickle'), 'wb'))
    for name, c in zip(names, classes):
        f = os.path.join(root, 'text_c10', 'class_%05d' % c, name[len('jpg/'):] + '.txt')
        os.makedirs(os.path.dirname(f), exist_ok=True)
        with open(f, 'w') as fh:
            fh.write('\n'.join('%s image %s caption %d of a small bird' % (split, name, k) for k in range(5)) + '\n')


def _make_cfg(root, stage, n_train, n_test, batch, **train):
    cfg = yaml.safe_load(open(os.path.join(CFG, stage, 'cfg', 'flowers.yml')))
    d = os.path.join(root, stage)
    cfg.update(DATASET_DIR=d + '/data/', CHECKPOINT_DIR=d + '/ckpt/', LOGS_DIR=d + '/logs/', SAMPLE_DIR=d + '/samples/')
    cfg['MODEL'].update(Z_DIM=8, EMBED_DIM=32, COMPRESSED_EMBED_DIM=16, GF_DIM=8, DF_DIM=4 if stage == 'stageII' else 8)
    cfg['TRAIN'].update(FLAG=False, BATCH_SIZE=batch, SAMPLE_NUM=batch, EPOCH=50, **train)
    rng = np.random.default_rng(0 if stage == 'stageI' else 1)
    orig = 76 if stage == 'stageI' else 304
    _write_split(d + '/data', 'train', n_train, rng, 32, orig)
    _write_split(d + '/data', 'test', n_test, rng, 32, orig)
    path = os.path.join(root, stage + '.yml')
    yaml.safe_dump(cfg, open(path, 'w'))
    return path, cfg


def _ckpt(directory, step):
    z = np.load(os.path.join(directory, 'model-%d.npz' % step))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """Stage I trained 3 updates (grids and checkpoints every 2), then Stage II 3 updates on top of it."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.stackgan.stageI import run as run1
    from t2i_amd.models.stackgan.stageII import run as run2
    root = str(tmp_path_factory.mktemp('stackgan'))
    p1, c1 = _make_cfg(root, 'stageI', 12, 9, 4, SAMPLE_PERIOD=2, CHECKPOINT_PERIOD=2)
    p2, c2 = _make_cfg(root, 'stageII', 6, 7, 2, SAMPLE_PERIOD=2, CHECKPOINT_PERIOD=3)
    np.random.seed(0); random.seed(0)
    t1 = run1.main(['--cfg', p1, '--train', '--steps', '3', '--graphs', '0'])
    store1 = {n: v.detach().cpu().numpy() for n, v in t1.model.store.vars.items()}
    np.random.seed(1); random.seed(1)
    t2 = run2.main(['--cfg_stage_I', p1, '--cfg', p2, '--train', '--steps', '3', '--graphs', '0'])
    torch.cuda.synchronize()
    return dict(root=root, p1=p1, c1=c1, p2=p2, c2=c2, t1=t1, store1=store1, t2=t2)


def test_stage_i_train_side_effects_and_resume(trained):
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan
    from t2i_amd.models.stackgan.stageI.trainer import ConditionalGanTrainer
    from t2i_amd.models.wgancls.run import load_dataset
    from t2i_amd.utils.config import config_from_yaml
    c1, t1 = trained['c1'], trained['t1']
    samples = sorted(os.listdir(c1['SAMPLE_DIR']))
    # 3 updates per epoch: the counter is 2 after epoch 0 idx 0 and 4 after idx 2
    assert samples == ['captions.txt', 'train_00_0000.png', 'train_00_0002.png'], samples
    assert 'caption 0 of a small bird' in open(os.path.join(c1['SAMPLE_DIR'], 'captions.txt')).read()
    assert sorted(f for f in os.listdir(c1['CHECKPOINT_DIR']) if f.endswith('.npz')) == ['model-2.npz', 'model-4.npz']
    ck = _ckpt(c1['CHECKPOINT_DIR'], 4)
    store = t1.model.store.vars
    assert set(ck) == set(store) and all(n.startswith(('g_net/', 'd_net/')) for n in ck)
    assert not any('Adam' in n for n in ck) and any(n.endswith('moving_mean') for n in ck)
    for n, v in store.items():
        assert ck[n].shape == tuple(v.shape), n
        assert np.array_equal(ck[n], trained['store1'][n]), n            # saved after the run's last update
    # a second run resumes at counter 4, epoch_start 4 // 3 = 1, with the checkpoint's weights and fresh Adam moments
    cfg = config_from_yaml(trained['p1'])
    m = ConditionalGan(cfg)
    tr = ConditionalGanTrainer(None, m, load_dataset(cfg, m.device), cfg)
    seen = {}

    def log(s):
        if 'Load SUCCESS' in s:
            seen.update({n: v.detach().cpu().numpy() for n, v in m.store.vars.items()})
            seen['adam'] = (float(tr.D_optim.m.abs().max()) if tr.D_optim.m is not None else 0.0, tr.D_optim.t)
    tr.train(max_updates=2, log=log, side_effects=True)
    assert (tr.start_counter, tr.epoch_start) == (4, 1)
    assert seen['adam'] == (0.0, 0)
    for n in store:
        assert np.array_equal(seen[n], ck[n]), n
    assert os.path.exists(os.path.join(c1['CHECKPOINT_DIR'], 'model-6.npz'))       # counter 4 -> 6


def test_stage_ii_train_restores_stage_i_and_saves_stage_ii_only(trained, tmp_path, capsys):
    from t2i_amd.models.stackgan.stageII import run as run2
    c2, t2 = trained['c2'], trained['t2']
    ck = _ckpt(c2['CHECKPOINT_DIR'], 2)             # counter % 3 == 2
    assert sorted(f for f in os.listdir(c2['CHECKPOINT_DIR']) if f.endswith('.npz')) == ['model-2.npz']
    assert ck and all(n.startswith(('stageII_g_net/', 'stageII_d_net/')) for n in ck) and not any('Adam' in n for n in ck)
    assert set(ck) == {n for n in t2.model.store.vars if n.startswith('stageII_')}
    assert sorted(os.listdir(c2['SAMPLE_DIR'])) == ['captions.txt', 'train_00_0000.png', 'train_00_0002.png']
    s1 = _ckpt(trained['c1']['CHECKPOINT_DIR'], 4)
    for n, v in t2.model.store.vars.items():          # the Stage-I generator's weights came from its checkpoint (not trained)
        if n.startswith('g_net/') and not n.endswith(('moving_mean', 'moving_variance')):
            assert np.array_equal(v.detach().cpu().numpy(), s1[n]), n
    # a Stage-I config whose checkpoint directory is empty: the reference's warning, and training goes on
    cfg1 = yaml.safe_load(open(trained['p1']))
    cfg1['CHECKPOINT_DIR'] = str(tmp_path / 'none') + '/'
    p1 = str(tmp_path / 's1.yml')
    yaml.safe_dump(cfg1, open(p1, 'w'))
    cfg2 = yaml.safe_load(open(trained['p2']))
    for k in ('CHECKPOINT_DIR', 'SAMPLE_DIR', 'LOGS_DIR'):
        cfg2[k] = str(tmp_path / k.lower()) + '/'
    p2 = str(tmp_path / 's2.yml')
    yaml.safe_dump(cfg2, open(p2, 'w'))
    capsys.readouterr()
    run2.main(['--cfg_stage_I', p1, '--cfg', p2, '--train', '--steps', '1', '--graphs', '0'])
    out = capsys.readouterr().out
    assert '[!] WARNING!!! Failed to load the parameters for stage I generator...' in out
    assert '[!] Load failed for stage II networks...' in out


# ---- evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eval_setup(trained, inception):
    arrays = dict(inception[0])
    arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] = arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] * np.float32(0.05)
    from PIL import Image
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
    paths = {}
    for stage, key, size, ss in (('stageI', 'p1', 12, 4), ('stageII', 'p2', 12, 4)):
        cfg = yaml.safe_load(open(trained[key]))
        cfg['EVAL'].update(INCEP_CHECKPOINT_DIR=incep_dir + '/', SAMPLE_SIZE=ss, SIZE=size, INCEP_BATCH_SIZE=ss,
                           ACT_STAT_PATH=os.path.join(root, 'fid_' + stage, 'stats.npz'), R_IMG_PATH=os.path.join(root, 'real'))
        paths[stage] = os.path.join(root, stage + '_eval.yml')
        yaml.safe_dump(cfg, open(paths[stage], 'w'))
    return arrays, paths, real_dir


def _stage_ii_eval(trained, eval_setup, mode, seed, incep_batch=None):
    from t2i_amd.models.stackgan.stageII.eval_stageii import StageIIEval
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan as S1
    from t2i_amd.models.stackgan.stageII.model import ConditionalGan as S2
    from t2i_amd.models.wgancls.run import load_dataset
    from t2i_amd.utils.config import config_from_yaml
    np.random.seed(seed); random.seed(seed); torch.manual_seed(seed)
    cfg = config_from_yaml(eval_setup[1]['stageII'])
    m = S2(S1(config_from_yaml(trained['p1']), build_model=False), cfg, build_model=False)
    ev = StageIIEval(None, m, load_dataset(cfg, m.device), cfg, incep_batch_size=incep_batch)
    return getattr(ev, {'is': 'evaluate_inception', 'fid': 'evaluate_fid', 'imd': 'evaluate_imd'}[mode])(keep_samples=True)


def test_stage_ii_eval_is_matches_oracle_unshuffled(trained, eval_setup):
    from t2i_amd.evaluation.inception_score import get_inception_from_predictions, softmax32
    from t2i_amd.models.stackgan.stageII import run as run2
    from t2i_amd.utils.utils import denormalize_images
    r = _stage_ii_eval(trained, eval_setup, 'is', 3)
    r2 = _stage_ii_eval(trained, eval_setup, 'is', 3)
    assert (r['mean'], r['std']) == (r2['mean'], r2['std']) and np.array_equal(r['samples'], r2['samples'])
    assert r['samples'].shape == (12, 256, 256, 3)
    logits, _ = _Oracle(eval_setup[0])(_np_prep(denormalize_images(r['samples'])))
    m, s = get_inception_from_predictions(softmax32(logits), 10, verbose=False)
    assert abs(r['mean'] - m) <= 1e-4 * abs(m) and abs(r['std'] - s) <= 1e-4 * max(abs(s), 1e-3), (r['mean'], m, r['std'], s)
    # the entry point runs the same evaluation and returns the numbers
    np.random.seed(3); random.seed(3); torch.manual_seed(3)
    out = run2.main(['--cfg_stage_I', trained['p1'], '--cfg', eval_setup[1]['stageII'], '--eval', 'is'])
    assert (out['mean'], out['std']) == (r['mean'], r['std']) and 'samples' not in out


def test_stage_ii_eval_fid_streams_the_statistics(trained, eval_setup):
    res = [_stage_ii_eval(trained, eval_setup, 'fid', 4, incep_batch=3)]
    path = yaml.safe_load(open(eval_setup[1]['stageII']))['EVAL']['ACT_STAT_PATH']
    stamp = os.stat(path).st_mtime_ns
    res.append(_stage_ii_eval(trained, eval_setup, 'fid', 4, incep_batch=3))
    assert os.stat(path).st_mtime_ns == stamp                      # the real statistics are reused
    f = res[0]
    assert np.isfinite(f['fid']) and f['fid'] == res[1]['fid'] and np.array_equal(f['mu_gen'], res[1]['mu_gen'])
    from t2i_amd.utils.utils import denormalize_images
    _, pre = _Oracle(eval_setup[0])(_np_prep(denormalize_images(f['samples'])))
    assert f['samples'].shape[0] == 12
    mu, sig = pre.mean(0), np.cov(pre, rowvar=False)
    assert np.abs(f['mu_gen'] - mu).max() <= 1e-4 * np.abs(mu).max()
    assert np.abs(f['sigma_gen'] - sig).max() <= 1e-4 * np.abs(sig).max()


def _check_imd(r, arrays):
    from t2i_amd.utils.utils import denormalize_images
    _, pr = _Oracle(arrays)(_np_prep(denormalize_images(r['real'])))
    _, pg = _Oracle(arrays)(_np_prep(denormalize_images(r['gen'])))
    want = _cos64(pr, pg)
    assert r['distances'].shape == want.shape and np.abs(r['distances'] - want).max() <= 1e-4, np.abs(r['distances'] - want).max()
    assert abs(r['mean'] - want.mean()) <= 1e-4 and abs(r['std'] - want.std()) <= 1e-4


def test_stage_ii_eval_imd_matches_oracle(trained, eval_setup):
    r = _stage_ii_eval(trained, eval_setup, 'imd', 5, incep_batch=3)
    assert r['real'].shape == r['gen'].shape == (12, 256, 256, 3)
    _check_imd(r, eval_setup[0])


def test_stage_i_eval_is_fid_imd_match_oracle(trained, eval_setup):
    from t2i_amd.evaluation.inception_score import get_inception_from_predictions, softmax32
    from t2i_amd.models.stackgan.stageI import run as run1
    from t2i_amd.models.stackgan.stageI.eval_stagei import StageIEval
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan
    from t2i_amd.models.wgancls.run import load_dataset
    from t2i_amd.utils.config import config_from_yaml
    from t2i_amd.utils.utils import denormalize_images
    arrays, paths = eval_setup[0], eval_setup[1]
    out = []
    for _ in range(2):
        np.random.seed(3); random.seed(3); torch.manual_seed(3)
        out.append(run1.main(['--cfg', paths['stageI'], '--eval', 'is']))
    r = out[0]
    assert (r['mean'], r['std']) == (out[1]['mean'], out[1]['std']) and sorted(r['indices']) == list(range(12))
    samples = denormalize_images(r['samples'].cpu().numpy())
    logits, _ = _Oracle(arrays)(_np_prep(samples[r['indices']]))
    m, s = get_inception_from_predictions(softmax32(logits), 10, verbose=False)
    assert abs(r['mean'] - m) <= 1e-4 * abs(m) and abs(r['std'] - s) <= 1e-4 * max(abs(s), 1e-3), (r['mean'], m, r['std'], s)
    np.random.seed(4); random.seed(4); torch.manual_seed(4)
    f = run1.main(['--cfg', paths['stageI'], '--eval', 'fid', '--incep-batch', '2'])
    assert np.isfinite(f['fid'])
    _, pre = _Oracle(arrays)(_np_prep(denormalize_images(f['samples'].cpu().numpy())))
    assert np.abs(f['mu_gen'] - pre.mean(0)).max() <= 1e-4 * np.abs(pre.mean(0)).max()
    np.random.seed(5); random.seed(5); torch.manual_seed(5)
    cfg = config_from_yaml(paths['stageI'])
    mdl = ConditionalGan(cfg, build_model=False)
    r = StageIEval(None, mdl, load_dataset(cfg, mdl.device), cfg, incep_batch_size=3).evaluate_imd(keep_samples=True)
    assert r['real'].shape == r['gen'].shape == (12, 64, 64, 3)
    _check_imd(r, arrays)


def test_stored_and_streamed_modes_see_the_same_images(trained, eval_setup):
    """The one evaluator core, stored and streamed: the same draws, the same kernels, the same order, so the generated images and
    the global np.random state behind them are equal to the bit (FID's path: training-mode batch norm, no shuffle)."""
    from t2i_amd.models.stackgan.stageI.eval_stagei import StageIEval
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan
    from t2i_amd.models.wgancls.run import load_dataset
    from t2i_amd.utils.config import config_from_yaml

    class Streamed(StageIEval):
        stored = False
    assert StageIEval.stored
    runs = []
    for cls in (StageIEval, Streamed):
        np.random.seed(6); random.seed(6); torch.manual_seed(6)
        cfg = config_from_yaml(eval_setup[1]['stageI'])
        mdl = ConditionalGan(cfg, build_model=False)
        f = cls(None, mdl, load_dataset(cfg, mdl.device), cfg, incep_batch_size=2).evaluate_fid(keep_samples=True)
        runs.append((f['samples'], np.random.get_state()))
    (stored, state_a), (streamed, state_b) = runs
    assert torch.is_tensor(stored) and stored.is_cuda and isinstance(streamed, np.ndarray)      # the device store / the host copies
    assert streamed.shape == (12, 64, 64, 3) and np.array_equal(stored.cpu().numpy(), streamed)
    assert state_a[0] == state_b[0] and np.array_equal(state_a[1], state_b[1]) and state_a[2:] == state_b[2:]


def test_compute_imd_on_image_folders(eval_setup):
    from t2i_amd.evaluation import imd
    from t2i_amd.evaluation.fid import load_inception_data
    from t2i_amd.models.inception.model import load_inception_inference
    arrays, real_dir = eval_setup[0], eval_setup[2]
    imgs = load_inception_data(real_dir, alphabetic=True)
    gen = [np.ascontiguousarray(im[::-1]) for im in imgs]          # flipped copies: distances well away from 0
    net = load_inception_inference(20, os.path.join(os.path.dirname(os.path.dirname(real_dir)), 'incep'), DEV)
    mean, std, d = imd.compute_imd(imgs, gen, net, 2)
    assert d.shape == (4,)
    _, pr = _Oracle(arrays)(_np_prep(imgs[:4]))
    _, pg = _Oracle(arrays)(_np_prep(gen[:4]))
    want = _cos64(pr, pg)
    assert np.abs(d - want).max() <= 1e-4 and abs(mean - want.mean()) <= 1e-4 and abs(std - want.std()) <= 1e-4
