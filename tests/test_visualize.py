"""The caption visualiser: utils/visualize.py helpers against in-test restatements of the reference's semantics (CPU), the
argument checks of t2i_nearest_images (CPU, nothing launched), and `run.py --visualize` end to end on a tiny pickled data set
with caption files (GPU): sheets, the neighbour search against a float64 brute force, and the reference's draw order."""
import ctypes
import os
import pickle
import random

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- helpers (CPU) -------------------------------------------------------------------------------------------------------
def test_slerp_lerp_directions_and_range():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import visualize as V
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(8), rng.standard_normal(8)
    assert V.slerp(a, b, 0) is a and V.slerp(a, b, 1) is b
    np.testing.assert_array_equal(V.lerp(a, b, 1), a)
    np.testing.assert_array_equal(V.lerp(a, b, 0), b)
    om = np.arccos(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
    for miu in (0.25, 0.5, 0.9):
        want = np.sin((1 - miu) * om) / np.sin(om) * a + np.sin(miu * om) / np.sin(om) * b
        np.testing.assert_allclose(V.slerp(a, b, miu), want, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(V.lerp(a, b, miu), miu * a + (1 - miu) * b, rtol=0, atol=0)
    for f in (V.slerp, V.lerp):
        for bad in (-0.01, 1.01):
            with pytest.raises(ValueError):
                f(a, b, bad)


def test_interpolated_batch_lengths_and_order():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import visualize as V
    a, b = np.array([1.0, 0.0]), np.array([0.0, 1.0])
    for bs in (4, 8, 16, 64):
        s = V.get_interpolated_batch(a, b, bs, 'slerp')
        assert len(s) == bs and len(V.get_interpolated_batch(a, b, bs, 'lerp')) == bs
        np.testing.assert_array_equal(s[0], b)         # slerp: miu = 1 first -> b ... miu = 0 last -> a
        np.testing.assert_array_equal(s[-1], a)
        l = V.get_interpolated_batch(a, b, bs, 'lerp')
        np.testing.assert_array_equal(l[0], a)         # lerp: the other way round
        np.testing.assert_array_equal(l[-1], b)
    assert len(V.get_interpolated_batch(a, b, 6, 'slerp')) == 7      # float arange overshoot, kept from the reference
    with pytest.raises(ValueError, match='batches of 6'):
        V.gen_noise_interp_img(lambda z, c: z, np.zeros(3, np.float32), 2, 6)


def test_captions_and_sheets():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import visualize as V
    assert V.preporcess_caption is V.preprocess_caption
    assert V.preprocess_caption('this flower is red') == 'This flower is red.'
    assert V.preprocess_caption('Petals.') == 'Petals.'
    rng = np.random.default_rng(1)
    batch = rng.uniform(-1, 1, (16, 64, 64, 3)).astype(np.float32)
    den = ((batch + 1.0) * 127.5).astype(np.uint8)
    sheet = V.prepare_img_for_captioning(batch, bottom=False)
    assert sheet.dtype == np.uint8 and sheet.shape == (3 * 64, 8 * 64, 3)
    assert np.all(sheet[:64] == 255)
    for i in range(16):
        r, c = divmod(i, 8)
        np.testing.assert_array_equal(sheet[64 * (r + 1):64 * (r + 2), 64 * c:64 * (c + 1)], den[i])
    tall = V.prepare_img_for_captioning(batch[:8], bottom=True)
    assert tall.shape == (3 * 64, 8 * 64, 3) and np.all(tall[-64:] == 255) and np.all(tall[:64] == 255)
    small = V.prepare_img_for_captioning(batch[:4], bottom=False)
    assert small.shape == (2 * 64, 4 * 64, 3)


def test_save_cap_batch_writes_the_caption_row_only(tmp_path):
    import t2i_amd  # noqa: F401
    from PIL import Image
    from t2i_amd.utils import visualize as V
    rng = np.random.default_rng(2)
    batch = rng.uniform(-1, 1, (8, 64, 64, 3)).astype(np.float32)
    path = str(tmp_path / 'a' / 'b.png')
    sheet = V.save_cap_batch(batch, 'a flower with many yellow petals and a dark brown center that is round', path)
    np.testing.assert_array_equal(np.array(Image.open(path)), sheet)
    np.testing.assert_array_equal(sheet[64:], V.prepare_img_for_captioning(batch, bottom=False)[64:])
    assert np.any(sheet[:64] != 255)
    fs = 64 // 3 - 2
    # split at the first space at or after character 50: a second line, one font size lower
    assert np.any(sheet[10 + fs:10 + 2 * fs] != 255)
    one_line = V.save_cap_batch(batch, 'short caption', str(tmp_path / 'c.png'))
    assert np.any(one_line[:10 + fs] != 255) and np.all(one_line[10 + fs + 4:64] == 255)
    interp = V.save_interp_cap_batch(batch, 'top', 'bottom', str(tmp_path / 'd.png'))
    assert interp.shape == (3 * 64, 8 * 64, 3) and np.any(interp[:64] != 255) and np.any(interp[-64:] != 255)
    np.testing.assert_array_equal(interp[64:128], sheet[64:128])


def test_write_caption_draws_text():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import visualize as V
    white = np.full((64, 256, 3), 255, np.uint8)
    assert np.all(V.write_caption(white, '', 19, 10) == 255)
    drawn = V.write_caption(white, 'Pink petals.', 19, 10)
    assert drawn.shape == white.shape and np.any(drawn != 255) and np.all(white == 255)


def test_nearest_images_rejects_bad_arguments_before_launching():
    """Every call below is invalid, so nothing is launched and no pointer is touched (the pointers are dummies)."""
    import t2i_amd  # noqa: F401
    from t2i_amd._lib import lib
    P = ctypes.c_void_p(4096)
    ws = ctypes.c_void_p(8192)
    need = lib.t2i_nearest_images_workspace_bytes(8, 100)
    assert need >= 8 * 100 * 8 and lib.t2i_nearest_images_workspace_bytes(0, 100) == 0

    def call(N=100, S=76, tabs=(P, P, P), Q=8, out=64, wsn=None, src=P, wsp=ws):
        return lib.t2i_nearest_images(src, N, S, *tabs, P, Q, out, -1.0, 1.0, P, P, wsp, need if wsn is None else wsn, None)
    assert call(N=0) == -1
    assert call(Q=0) == -1
    assert call(out=0) == -1
    assert call(out=77) == -1
    assert call(N=2 ** 31) == -1
    assert call(tabs=(P, None, P)) == -1
    assert call(tabs=(None, None, None)) == -1               # identity crop needs S == out_size
    assert call(src=None) == -1
    assert b'bad argument' in lib.t2i_last_error()
    assert call(wsn=need - 1) == -2
    assert call(wsp=None) == -2
    assert b'workspace' in lib.t2i_last_error()


def test_run_visualize_mode_errors(tmp_path):
    """--visualize with --synthetic has no uint8 store to search; --train and --visualize exclude each other."""
    import t2i_amd  # noqa: F401
    from t2i_amd.models.wgancls import run
    path = _make_cfg(tmp_path, data=False)
    with pytest.raises(ValueError, match='synthetic'):
        run.main(['--cfg', path, '--visualize', '--synthetic'])
    with pytest.raises(SystemExit):
        run.main(['--cfg', path, '--visualize', '--train'])


# ---- end to end (GPU) ----------------------------------------------------------------------------------------------------
def _write_split(root, split, n, rng, emb_dim):
    import joblib
    path = os.path.join(root, split)
    os.makedirs(path)
    joblib.dump(list(rng.integers(0, 256, (n, 76, 76, 3), dtype=np.uint8)), os.path.join(path, '76images.pickle'))
    pickle.dump(list(rng.standard_normal((n, 5, emb_dim)).astype(np.float32)), open(os.path.join(path, 'char-CNN-RNN-embeddings.pickle'), 'wb'))
    names = ['jpg/%s_%05d' % (split, i) for i in range(n)]
    classes = [int(c) for c in rng.integers(1, 6, n)]
    pickle.dump(names, open(os.path.join(path, 'filenames.pickle'), 'wb'))
    pickle.dump(classes, open(os.path.join(path, 'class_info.pickle'), 'wb'))
    for name, c in zip(names, classes):       # <workdir>/text_c10/class_%05d/<name>.txt, five captions each
        f = os.path.join(root, 'text_c10', 'class_%05d' % c, name[len('jpg/'):] + '.txt')
        os.makedirs(os.path.dirname(f), exist_ok=True)
        with open(f, 'w') as fh:
            fh.write('\n'.join('%s image %s caption %d of a flower with long thin petals that are yellow' % (split, name, k)
                               for k in range(5)) + '\n')


def _make_cfg(tmp_path, n_train=12, n_test=9, batch=4, data=True):
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'text-to-image_amd', 'models', 'wgancls', 'cfg', 'flowers.yml')))
    d = str(tmp_path)
    cfg.update(DATASET_DIR=d + '/data/flowers/', CHECKPOINT_DIR=d + '/ckpt/', LOGS_DIR=d + '/logs/', SAMPLE_DIR=d + '/samples/')
    cfg['MODEL'].update(Z_DIM=8, EMBED_DIM=32, COMPRESSED_EMBED_DIM=16, GF_DIM=8, DF_DIM=8)
    cfg['TRAIN'].update(FLAG=False, BATCH_SIZE=batch, SAMPLE_NUM=batch, SAMPLE_PERIOD=100, SUMMARY_PERIOD=100, MAX_STEPS=3)
    if data:
        rng = np.random.default_rng(0)
        _write_split(d + '/data/flowers', 'train', n_train, rng, 32)
        _write_split(d + '/data/flowers', 'test', n_test, rng, 32)
    path = d + '/cfg.yml'
    yaml.safe_dump(cfg, open(path, 'w'))
    return path


def _replay_crops(seed, n_test, n_train, B, z_dim, Q, imsize=64, S=76):
    """The reference's draws from the seeds: the two Dataset constructors (test, then train: one shuffle each), dataset_pos,
    the three special positions (one crop each + z), the neighbour batch (B crops + z), then one crop per train image and
    per query, query by query."""
    np.random.seed(seed); random.seed(seed)
    np.random.shuffle(np.arange(n_test)); np.random.shuffle(np.arange(n_train))
    np.random.randint(0, n_test)

    def crops(n):
        out = np.zeros((3, n), np.int32)
        for i in range(n):
            h1 = int(np.floor((S - imsize) * np.random.random()))
            w1 = int(np.floor((S - imsize) * np.random.random()))
            out[:, i] = (w1, h1, 1 if random.random() > 0.5 else 0)
        return out
    for _ in range(3):
        crops(1); np.random.standard_normal(size=(B, z_dim))
    crops(B); np.random.standard_normal(size=(B, z_dim))
    return crops(Q * n_train).reshape(3, Q, n_train)


@pytest.mark.gpu
def test_run_visualize_end_to_end(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import joblib
    from PIL import Image
    import t2i_amd  # noqa: F401
    from t2i_amd.models.wgancls import run
    path = _make_cfg(tmp_path)
    np.random.seed(0); random.seed(0)
    run.main(['--cfg', path, '--train', '--steps', '3', '--graphs', '0'])
    assert os.path.exists(str(tmp_path / 'ckpt' / 'model-2.npz'))

    np.random.seed(5); random.seed(5)
    res = run.main(['--cfg', path, '--visualize'])
    vis = str(tmp_path / 'samples' / 'flowers_visual')
    assert sorted(os.listdir(vis)) == ['neighb', 'special_cap']
    for i in range(3):
        im = np.array(Image.open(os.path.join(vis, 'special_cap', 'cap%d.png' % i)))
        assert im.shape == (2 * 64, 4 * 64, 3) and np.array_equal(im, res['special_cap'][i])
        assert np.any(im[:64] != 255)                            # the caption of the (clamped) special position
    nb = np.array(Image.open(os.path.join(vis, 'neighb', 'neighb.png')))
    assert nb.shape == (2 * 64, 8 * 64, 3) and np.array_equal(nb, res['neighb'])

    # the neighbour ids: float64 brute force over the returned samples and crop table
    train = np.asarray(joblib.load(str(tmp_path / 'data' / 'flowers' / 'train' / '76images.pickle')))
    samples, (row0, col0, flip) = res['samples'], res['crops']
    Q, N = samples.shape[0], train.shape[0]
    assert Q == 4 and row0.shape == (Q, N)
    fake = np.clip(samples, -1, 1).astype(np.float64)
    for q in range(Q):
        rows = row0[q][:, None] + np.arange(64)
        cols = np.where(flip[q][:, None] != 0, col0[q][:, None] + 63 - np.arange(64), col0[q][:, None] + np.arange(64))
        crops = train[np.arange(N)[:, None, None], rows[:, :, None], cols[:, None, :], :]
        real = (crops.astype(np.float32) * np.float32(2. / 255) - np.float32(1.)).astype(np.float64)
        d2 = ((fake[q][None] - real) ** 2).sum(axis=(1, 2, 3))
        j = int(np.argmin(d2))
        assert res['neighbour_ids'][q] == j
        np.testing.assert_array_equal(res['neighbours'][q], real[j].astype(np.float32))
    # the crop table is the reference loop's draws from the same seeds
    want = _replay_crops(5, 9, 12, 4, 8, Q)
    np.testing.assert_array_equal(row0, want[0])
    np.testing.assert_array_equal(col0, want[1])
    np.testing.assert_array_equal(flip, want[2])

    # --interp 1 adds the interpolation and captioned sheets
    res = run.main(['--cfg', path, '--visualize', '--interp', '1'])
    for kind, name, shape in (('z_interp', 'z_interp0', (128, 256, 3)), ('cond_interp', 'cond_interp0', (192, 256, 3)),
                              ('cap', 'cap0', (128, 256, 3))):
        im = np.array(Image.open(os.path.join(vis, kind, name + '.png')))
        assert im.shape == shape and np.array_equal(im, res[kind][0])

    # no checkpoint: the reference's error
    cfg = yaml.safe_load(open(path))
    cfg['CHECKPOINT_DIR'] = str(tmp_path / 'empty_ckpt') + '/'
    yaml.safe_dump(cfg, open(path, 'w'))
    with pytest.raises(RuntimeError, match='Could not load the checkpoints of the generator'):
        run.main(['--cfg', path, '--visualize'])
