"""The evaluator's host side (no GPU): Pillow's bilinear tables and fixed-point passes, the InceptionV3 layer table, the
Inception-score and Frechet-distance formulas, the grayscale quirk and run.py's --eval arguments."""
import os
import sys

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.mark.parametrize('hw', [(64, 64), (76, 76), (500, 667), (299, 299), (300, 17)])
def test_resize_tables_are_pillows_bit_for_bit(hw):
    from PIL import Image
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.resize import prep_incep_img, resize_u8
    img = np.random.default_rng(hw[0] * 1000 + hw[1]).integers(0, 256, hw + (3,), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img).resize((299, 299), Image.BILINEAR))
    np.testing.assert_array_equal(resize_u8(img, 299, 299), want)
    np.testing.assert_array_equal(prep_incep_img(img), want.astype(np.float32) / 127.5 - 1.)


def test_resize_tables_shape():
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.resize import PRECISION_BITS, bilinear_tables
    b, k = bilinear_tables(64, 299)                     # upscale: support 1, 3 taps
    assert b.shape == (299, 2) and k.shape == (299, 3)
    b, k = bilinear_tables(667, 299)                    # antialiased downscale: support 667 / 299
    assert k.shape == (299, 2 * int(np.ceil(667 / 299)) + 1)
    assert (b[:, 0] >= 0).all() and (b.sum(1) <= 667).all() and (b[:, 1] <= k.shape[1]).all()
    assert np.all(np.abs(k.sum(1) - (1 << PRECISION_BITS)) <= k.shape[1])
    b, k = bilinear_tables(299, 299)                    # identity
    assert (b[:, 0] == np.arange(299)).all() and (k[:, 0] == 1 << PRECISION_BITS).all()


def test_fp64_quotient_rounds_like_fp32_division():
    """The resize kernel computes u / 127.5 in fp64 and rounds to fp32: the same value as numpy's fp32 division, every u."""
    u = np.arange(256, dtype=np.float32)
    np.testing.assert_array_equal((u.astype(np.float64) / 127.5).astype(np.float32) - np.float32(1), u / 127.5 - 1.)


def test_grayscale_resize_quirk():
    """np.resize of a 2-D image to [h, w, 3] repeats the flattened pixels cyclically: channel values come from neighbours."""
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.resize import to_rgb
    g = np.arange(6, dtype=np.uint8).reshape(2, 3)
    out = to_rgb(g)
    assert out.shape == (2, 3, 3)
    np.testing.assert_array_equal(out.reshape(-1), np.tile(np.arange(6), 3))
    assert not np.array_equal(out[..., 1], g)           # not a channel replication
    rgb = np.zeros((2, 2, 3), np.uint8)
    assert to_rgb(rgb) is rgb or np.array_equal(to_rgb(rgb), rgb)


def test_layer_table_names_shapes_and_parameter_count():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception import model as M
    t = M.layer_table(20)
    assert len(t) == 95                                  # 94 conv + batch-norm layers and the logits
    assert t['Conv2d_1a_3x3'] == (3, 3, 3, 32, 2, 'VALID', 149, 149, True)
    assert t['Conv2d_4a_3x3'][6:8] == (71, 71)
    assert t['Mixed_5b/Branch_1/Conv2d_0b_5x5'][:4] == (5, 5, 48, 64)
    assert t['Mixed_5c/Branch_1/Conv_1_0c_5x5'][:4] == (5, 5, 48, 64)
    assert t['Mixed_5c/Branch_1/Conv2d_0b_1x1'][2:4] == (256, 48)
    assert t['Mixed_6a/Branch_0/Conv2d_1a_1x1'] == (3, 3, 288, 384, 2, 'VALID', 17, 17, True)
    assert t['Mixed_6b/Branch_1/Conv2d_0b_1x7'][:4] == (1, 7, 128, 128)
    assert t['Mixed_6e/Branch_2/Conv2d_0d_7x1'][:4] == (7, 1, 192, 192)
    assert t['Mixed_7a/Branch_1/Conv2d_1a_3x3'] == (3, 3, 192, 192, 2, 'VALID', 8, 8, True)
    assert t['Mixed_7b/Branch_0/Conv2d_0a_1x1'][2] == 1280
    assert t['Mixed_7b/Branch_1/Conv2d_0b_3x1'][:4] == (3, 1, 384, 384)
    assert t['Mixed_7c/Branch_1/Conv2d_0c_3x1'][:4] == (3, 1, 384, 384)
    assert t['Mixed_7c/Branch_2/Conv2d_0a_1x1'][2:4] == (2048, 448)
    assert t['Logits/Conv2d_1c_1x1'] == (1, 1, 2048, 20, 1, 'VALID', 1, 1, False)
    s = M.variable_shapes(20)
    assert s['InceptionV3/Logits/Conv2d_1c_1x1/biases'] == (20,)
    assert s['InceptionV3/Mixed_7c/Branch_3/Conv2d_0b_1x1/BatchNorm/moving_variance'] == (192,)
    assert 'InceptionV3/Conv2d_1a_3x3/biases' not in s
    # slim InceptionV3 base (21 802 784 with the BN statistics) + a 2048 x 20 logits layer with bias
    assert sum(int(np.prod(v)) for v in s.values()) == 21802784 + 2048 * 20 + 20
    assert abs(M.multiply_adds(20) / 5.71e9 - 1) < 0.01


def test_fold_batch_norm():
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception.model import fold_batch_norm
    rng = np.random.default_rng(1)
    w, beta, mean, var = rng.standard_normal((3, 3, 4, 5)), rng.standard_normal(5), rng.standard_normal(5), rng.random(5) + .1
    x = rng.standard_normal((3, 3, 4))
    fw, fb = fold_batch_norm(w, beta, mean, var)
    ref = ((x[..., None] * w).sum((0, 1, 2)) - mean) / np.sqrt(var + 0.001) + beta
    np.testing.assert_allclose((x[..., None] * fw).sum((0, 1, 2)) + fb, ref, rtol=1e-5, atol=1e-5)


def _reference_is(preds, splits):
    scores = []
    for i in range(splits):
        part = preds[i * preds.shape[0] // splits:(i + 1) * preds.shape[0] // splits, :]
        kl = part * (np.log(part) - np.log(np.expand_dims(np.mean(part, 0), 0)))
        scores.append(np.exp(np.mean(np.sum(kl, 1))))
    return np.mean(scores), np.std(scores)


def test_inception_score_formula():
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.inception_score import get_inception_from_predictions, softmax32
    logits = np.random.default_rng(2).standard_normal((103, 20)).astype(np.float32) * 3
    p = softmax32(logits)
    assert p.dtype == np.float32 and np.allclose(p.sum(1), 1, atol=1e-6)
    m, s = get_inception_from_predictions(p, 10, verbose=False)
    rm, rs = _reference_is(p.astype(np.float64), 10)
    assert m == pytest.approx(rm, rel=1e-12) and s == pytest.approx(rs, rel=1e-9, abs=1e-12)
    assert get_inception_from_predictions(np.full((20, 4), .25), 10, verbose=False) == (pytest.approx(1.0), pytest.approx(0.0))


def _reference_fd(mu1, sigma1, mu2, sigma2, eps=1e-6):
    from scipy import linalg
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def test_frechet_distance_formula_and_eps_retry(monkeypatch):
    import t2i_amd  # noqa: F401
    from scipy import linalg
    from t2i_amd.evaluation.fid import calculate_frechet_distance
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((200, 16)), rng.standard_normal((200, 16)) * 1.5 + .3
    mu1, s1, mu2, s2 = a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False)
    assert calculate_frechet_distance(mu1, s1, mu2, s2) == pytest.approx(_reference_fd(mu1, s1, mu2, s2), rel=1e-10)
    assert abs(calculate_frechet_distance(mu1, s1, mu1, s1)) < 1e-8
    # the first sqrtm is not finite: retried with eps on the diagonals (the reference's path), with its warning
    real = linalg.sqrtm
    calls = []

    def flaky(m, disp=True):
        calls.append(disp)
        if len(calls) == 1:
            return np.full_like(m, np.nan), 1.0
        return real(m, disp=disp) if disp is not True else real(m)
    monkeypatch.setattr(linalg, 'sqrtm', flaky)
    with pytest.warns(UserWarning, match='adding 1e-06'):
        got = calculate_frechet_distance(mu1, s1, mu2, s2)
    monkeypatch.setattr(linalg, 'sqrtm', real)
    off = np.eye(16) * 1e-6
    want = mu1 - mu2
    want = want.dot(want) + np.trace(s1) + np.trace(s2) - 2 * np.trace(real((s1 + off).dot(s2 + off)).real)
    assert len(calls) == 2 and got == pytest.approx(want, rel=1e-10)
    with pytest.raises(ValueError):
        calculate_frechet_distance(mu1, s1, mu2[:3], s2[:3, :3])


def test_activation_statistics_file_round_trip(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.fid import load_activation_statistics, save_activation_statistics
    mu, sigma = np.arange(3.), np.eye(3)
    path = str(tmp_path / 'fid' / 'stats.npz')
    save_activation_statistics(mu, sigma, path)
    m, s = load_activation_statistics(path)
    np.testing.assert_array_equal(m, mu); np.testing.assert_array_equal(s, sigma)
    with pytest.raises(RuntimeError, match='already exists'):
        save_activation_statistics(mu, sigma, path)


def _cfg(tmp_path, eval_flag=False):
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'text-to-image_amd', 'models', 'wgancls', 'cfg', 'flowers.yml')))
    d = str(tmp_path)
    cfg.update(DATASET_DIR=d + '/data/flowers/', CHECKPOINT_DIR=d + '/ckpt/', LOGS_DIR=d + '/logs/', SAMPLE_DIR=d + '/samples/')
    cfg['EVAL']['FLAG'] = eval_flag
    path = d + '/cfg.yml'
    yaml.safe_dump(cfg, open(path, 'w'))
    return path


def test_run_eval_argument_errors(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.wgancls import run
    path = _cfg(tmp_path)
    with pytest.raises(ValueError, match='synthetic'):
        run.main(['--cfg', path, '--eval', 'is', '--synthetic'])
    for bad in (['--eval', 'kid'], ['--eval'], ['--eval', 'is', '--train'], ['--eval', 'fid', '--visualize']):
        with pytest.raises(SystemExit):
            run.main(['--cfg', path] + bad)
    with pytest.raises(ValueError, match='incep-batch'):
        run.main(['--cfg', path, '--eval', 'is', '--incep-batch', '0'])
    with pytest.raises(ValueError, match='incep-batch'):
        run.main(['--cfg', path, '--train', '--incep-batch', '8'])


def test_eval_flag_without_eval_still_raises(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.wgancls import run
    path = _cfg(tmp_path, eval_flag=True)
    with pytest.raises(NotImplementedError, match='EVAL.FLAG'):
        run.main(['--cfg', path])
    with pytest.raises(NotImplementedError, match='--eval'):
        run.main(['--cfg', path, '--train'])
