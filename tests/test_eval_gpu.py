"""The evaluator on the GPU: t2i_resample_bilinear against Pillow's arithmetic (NumPy statement, itself held to Pillow by
test_eval_host.py), t2i_pool2d / t2i_channel_slice_copy / t2i_gram_accumulate against NumPy, InceptionV3 against a float64
torch-CPU oracle with unfolded batch norm on random calibrated weights, and `run.py --eval is|fid` end to end."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def _np_prep(u8_images):
    from t2i_amd.evaluation.resize import resize_u8
    return np.stack([resize_u8(im, 299, 299) for im in u8_images]).astype(np.float32) / 127.5 - 1.


# ---- resize -------------------------------------------------------------------------------------------------------------
def test_resample_uint8_gather_upscale_and_downscale():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    rng = np.random.default_rng(0)
    store = rng.integers(0, 256, (5, 76, 76, 3), dtype=np.uint8)
    rows = np.array([3, 0, 4, 0], np.int32)
    got = K.resample_bilinear(torch.from_numpy(store).to(DEV), 299, 299, rows=torch.from_numpy(rows)).cpu().numpy()
    np.testing.assert_array_equal(got, _np_prep(store[rows]))
    big = rng.integers(0, 256, (2, 500, 667, 3), dtype=np.uint8)           # antialiased downscale, no gather
    got = K.resample_bilinear(torch.from_numpy(big).to(DEV), 299, 299).cpu().numpy()
    np.testing.assert_array_equal(got, _np_prep(big))
    same = rng.integers(0, 256, (1, 299, 299, 3), dtype=np.uint8)
    got = K.resample_bilinear(torch.from_numpy(same).to(DEV), 299, 299).cpu().numpy()
    np.testing.assert_array_equal(got, same.astype(np.float32) / 127.5 - 1.)


def test_resample_fp32_generator_source_denormalises_in_kernel():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.utils.utils import denormalize_images
    rng = np.random.default_rng(1)
    x = np.tanh(rng.standard_normal((6, 64, 64, 3)) * 2).astype(np.float32)
    x[0, 0, 0] = (-1.0, 1.0, 0.0)
    src = torch.from_numpy(x).to(DEV)
    rows = torch.tensor([5, 1, 1, 2], dtype=torch.int32)
    got = K.resample_bilinear(src, 299, 299, rows=rows).cpu().numpy()
    np.testing.assert_array_equal(got, _np_prep(denormalize_images(x[[5, 1, 1, 2]])))
    u8 = K.resample_bilinear(src, 64, 64, out_u8=True).cpu().numpy()          # identity tables: the uint8 store itself
    np.testing.assert_array_equal(u8, denormalize_images(x))


# ---- pooling and concatenation -------------------------------------------------------------------------------------------
def _np_pool(x, k, s, padding, op):
    B, H, W, C = x.shape
    if padding == 'SAME':
        Ho, Wo = -(-H // s), -(-W // s)
        pt, pl = max((Ho - 1) * s + k - H, 0) // 2, max((Wo - 1) * s + k - W, 0) // 2
    else:
        Ho, Wo, pt, pl = (H - k) // s + 1, (W - k) // s + 1, 0, 0
    out = np.zeros((B, Ho, Wo, C), np.float64 if op == 'avg' else x.dtype)
    for oy in range(Ho):
        for ox in range(Wo):
            y0, x0 = oy * s - pt, ox * s - pl
            win = x[:, max(y0, 0):min(y0 + k, H), max(x0, 0):min(x0 + k, W), :]
            out[:, oy, ox] = win.max(axis=(1, 2)) if op == 'max' else win.astype(np.float64).mean(axis=(1, 2))
    return out


@pytest.mark.parametrize('C', [8, 3])
@pytest.mark.parametrize('k,s,padding', [(3, 2, 'VALID'), (3, 1, 'SAME'), (2, 2, 'SAME'), (4, 3, 'SAME'), (8, 2, 'VALID')])
def test_pool2d_matches_numpy(C, k, s, padding):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    x = np.random.default_rng(k * 10 + s).standard_normal((2, 9, 8, C)).astype(np.float32) + 3
    xd = torch.from_numpy(x).to(DEV)
    got = K.pool2d(xd, k, k, s, s, padding, K.POOL_MAX).cpu().numpy()
    np.testing.assert_array_equal(got, _np_pool(x, k, s, padding, 'max'))
    want = _np_pool(x, k, s, padding, 'avg')
    got = K.pool2d(xd, k, k, s, s, padding, K.POOL_AVG).cpu().numpy()
    assert np.abs(got - want).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()
    # into a channel slice of a wider buffer: the other channels are untouched
    ld, c0 = C + 8, 4
    buf = torch.full(tuple(want.shape[:3]) + (ld,), 7.0, device=DEV)
    K.pool2d(xd, k, k, s, s, padding, K.POOL_AVG, out=buf, c0=c0)
    b = buf.cpu().numpy()
    np.testing.assert_array_equal(b[..., c0:c0 + C], got)
    assert (b[..., :c0] == 7).all() and (b[..., c0 + C:] == 7).all()


@pytest.mark.parametrize('C,ld,c0', [(64, 256, 64), (96, 288, 128), (3, 10, 5)])
def test_channel_slice_copy_is_exact(C, ld, c0):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    x = torch.randn(2, 5, 7, C, device=DEV)
    out = torch.full((2, 5, 7, ld), -3.0, device=DEV)
    K.channel_slice_copy(x, out, c0)
    want = torch.full((2, 5, 7, ld), -3.0)
    want[..., c0:c0 + C] = x.cpu()
    assert torch.equal(out.cpu(), want)


# ---- FID statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,offset', [(2048, 0.0), (100, 1000.0)])
def test_gram_accumulate_matches_np_cov(d, offset):
    """Several calls (uneven row counts), activations with a large common mean (the cancellation case): mu and sigma within
    1e-6 of max |sigma| of float64 np.mean / np.cov, and a repeated run bitwise identical."""
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.fid import ActivationStatistics
    rng = np.random.default_rng(d)
    mix = rng.standard_normal((d, d)) / np.sqrt(d)
    X = (np.abs(rng.standard_normal((203, d)) @ mix) + offset + rng.random(d)).astype(np.float32)
    runs = []
    for _ in range(2):
        st = ActivationStatistics(d, DEV)
        for a, b in ((0, 64), (64, 128), (128, 131), (131, 203)):
            st.add(torch.from_numpy(X[a:b]).to(DEV))
        runs.append(st.finalize() + (st.sum.cpu().numpy(), st.gram.cpu().numpy()))
    mu, sigma = runs[0][:2]
    X64 = X.astype(np.float64)
    ref_s = np.cov(X64, rowvar=False)
    scale = np.abs(ref_s).max()
    assert np.abs(mu - X64.mean(0)).max() <= 1e-6 * max(np.abs(X64.mean(0)).max(), 1.0)
    assert np.abs(sigma - ref_s).max() <= 1e-6 * scale, np.abs(sigma - ref_s).max() / scale
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


# ---- InceptionV3 ---------------------------------------------------------------------------------------------------------
class _Oracle(object):
    """float64 torch-CPU statement of the network (unfolded batch norm; TF SAME padding by explicit pads).  With calibrate=True
    each batch-normed layer's moving statistics are set from the batch first, so every pre-activation is about N(0, 1)."""

    def __init__(self, arrays, calibrate=False):
        self.a, self.calibrate = arrays, calibrate

    def conv(self, x, name, kh, kw, cout, stride=1, padding='SAME', bn=True):
        import torch.nn.functional as F
        base = 'InceptionV3/%s/' % name
        w = torch.from_numpy(np.asarray(self.a[base + 'weights'], np.float64)).permute(3, 2, 0, 1)
        if padding == 'SAME':
            H, W = x.shape[2], x.shape[3]
            ph = max((-(-H // stride) - 1) * stride + kh - H, 0)
            pw = max((-(-W // stride) - 1) * stride + kw - W, 0)
            x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
        z = F.conv2d(x, w, stride=stride)
        if not bn:
            return z + torch.from_numpy(np.asarray(self.a[base + 'biases'], np.float64))[None, :, None, None]
        if self.calibrate:
            self.a[base + 'BatchNorm/moving_mean'] = z.mean((0, 2, 3)).numpy().astype(np.float32)
            self.a[base + 'BatchNorm/moving_variance'] = z.var((0, 2, 3)).numpy().astype(np.float32)
        g = lambda k: torch.from_numpy(np.asarray(self.a[base + 'BatchNorm/' + k], np.float64))[None, :, None, None]  # noqa: E731
        return torch.relu((z - g('moving_mean')) / torch.sqrt(g('moving_variance') + 0.001) + g('beta'))

    def pool(self, x, name, k, stride, padding, op):
        import torch.nn.functional as F
        from t2i_amd import kernels as K
        if op == K.POOL_MAX:
            assert padding == 'VALID'
            return F.max_pool2d(x, k, stride)
        if padding == 'SAME':
            assert k == 3 and stride == 1
            return F.avg_pool2d(x, 3, 1, padding=1, count_include_pad=False)
        return F.avg_pool2d(x, k, stride)

    pool_into = pool

    def concat(self, parts):
        return torch.cat(parts, 1)

    def __call__(self, images):
        from t2i_amd.models.inception.model import _inception_v3
        with torch.no_grad():
            x = torch.from_numpy(np.asarray(images, np.float64)).permute(0, 3, 1, 2)
            logits, pre = _inception_v3(self, x, 20)
        return logits.reshape(len(images), -1).numpy(), pre.reshape(len(images), -1).numpy()


def _random_inception(seed, calib_images):
    from t2i_amd.models.inception.model import variable_shapes
    rng = np.random.default_rng(seed)
    arrays = {}
    for k, shape in variable_shapes(20).items():
        if k.endswith('weights'):
            arrays[k] = (rng.standard_normal(shape) / np.sqrt(np.prod(shape[:3]))).astype(np.float32)
        elif k.endswith('beta') or k.endswith('biases'):
            arrays[k] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        else:
            arrays[k] = np.ones(shape, np.float32)
    arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] *= 2         # a spread of class probabilities, none underflowing to 0
    arrays['InceptionV3/AuxLogits/Conv2d_1b_1x1/weights'] = np.zeros((1, 1, 768, 128), np.float32)    # ignored
    _Oracle(arrays, calibrate=True)(calib_images)
    return arrays


@pytest.fixture(scope='module')
def inception():
    import t2i_amd  # noqa: F401
    rng = np.random.default_rng(7)
    # uniform noise, low-contrast grey and a smooth ramp: moving statistics that keep any image (generated ones included) in
    # range, so no class probability underflows to 0
    grey = (128 + rng.integers(-8, 9, (1, 64, 64, 3))).astype(np.uint8)
    yy, xx = np.mgrid[0:64, 0:64]
    ramp = np.stack([yy * 4, xx * 4, (yy + xx) * 2], -1)[None].astype(np.uint8)
    calib = _np_prep(np.concatenate([rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8), grey, ramp]))
    return _random_inception(8, calib), calib


@pytest.mark.parametrize('B', [2, 3, 4])
def test_inception_forward_matches_float64_oracle(inception, B):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception.model import InceptionV3
    arrays, calib = inception
    images = {2: calib[[0, 3]], 4: calib}.get(B)
    images = images if images is not None else _np_prep(np.random.default_rng(9).integers(0, 256, (3, 80, 70, 3), dtype=np.uint8))
    net = InceptionV3.from_arrays(arrays, 20, DEV)
    logits, pre = net(torch.from_numpy(images).to(DEV))
    ref_l, ref_p = _Oracle(arrays)(images)
    el = np.abs(logits.cpu().numpy() - ref_l).max() / np.abs(ref_l).max()
    ep = np.abs(pre.cpu().numpy() - ref_p).max() / np.abs(ref_p).max()
    print('InceptionV3 B=%d: PreLogits error %.2e, logits error %.2e of max |ref|' % (B, ep, el))
    # measured on MI355X: PreLogits 3.4e-5 / 4.2e-5 / 3.6e-5 and logits 2.5e-5 / 3.0e-5 / 3.4e-5 of max |ref| at B = 2 / 3 / 4
    # (94 fp32 layers, some on the Winograd F(2x2, 3x3) path)
    assert ep <= 1e-4 and el <= 1e-4, (ep, el)


def test_inception_checkpoint_missing_key_is_named(inception, tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.inception.model import load_inception_inference
    arrays = dict(inception[0])
    del arrays['InceptionV3/Mixed_6c/Branch_2/Conv2d_0d_7x1/BatchNorm/beta']
    np.savez(str(tmp_path / 'model-1.npz'), **arrays)
    open(str(tmp_path / 'checkpoint'), 'w').write('model_checkpoint_path: "model-1.npz"\n')
    with pytest.raises(KeyError, match='Mixed_6c/Branch_2/Conv2d_0d_7x1/BatchNorm/beta'):
        load_inception_inference(20, str(tmp_path), DEV)


# ---- run.py --eval end to end --------------------------------------------------------------------------------------------
def test_run_eval_end_to_end(inception, tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    cache_was_on = K.filter_cache_enabled()
    try:
        _run_eval_end_to_end(inception[0], tmp_path)
    finally:           # run.py's training mode switched the transformed-filter cache on: later tests in this process expect it off
        K.filter_cache(cache_was_on)
        K.filter_cache_reset()


def _run_eval_end_to_end(arrays, tmp_path):
    # the generator's images after three steps are far from the calibration images (oracle logits up to ~90): a smaller logits
    # layer keeps every class probability above fp32 underflow, where the reference's formula gives 0 * log 0 = nan
    arrays = dict(arrays)
    arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] = arrays['InceptionV3/Logits/Conv2d_1c_1x1/weights'] * np.float32(0.05)
    from PIL import Image
    from t2i_amd.evaluation.inception_score import get_inception_from_predictions, softmax32
    from t2i_amd.evaluation.resize import to_rgb
    from t2i_amd.models.wgancls import run
    from t2i_amd.utils.utils import denormalize_images
    from test_visualize import _make_cfg
    path = _make_cfg(tmp_path)
    np.random.seed(0); random.seed(0)
    run.main(['--cfg', path, '--train', '--steps', '3', '--graphs', '0'])
    incep_dir = tmp_path / 'incep'
    incep_dir.mkdir()
    np.savez(str(incep_dir / 'model-7.npz'), **arrays)
    open(str(incep_dir / 'checkpoint'), 'w').write('model_checkpoint_path: "model-7.npz"\n')
    real_dir = tmp_path / 'real' / 'jpg'
    real_dir.mkdir(parents=True)
    rng = np.random.default_rng(11)
    for i, shape in enumerate([(80, 100, 3), (64, 64, 3), (70, 90), (120, 77, 3), (66, 66, 3), (90, 60, 3)]):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(str(real_dir / ('image_%d.jpg' % i)), quality=95)
    cfg = yaml.safe_load(open(path))
    cfg['EVAL'].update(INCEP_CHECKPOINT_DIR=str(incep_dir) + '/', SAMPLE_SIZE=8, SIZE=16, INCEP_BATCH_SIZE=4,
                       ACT_STAT_PATH=str(tmp_path / 'fid' / 'stats.npz'), R_IMG_PATH=str(tmp_path / 'real'))
    yaml.safe_dump(cfg, open(path, 'w'))

    from t2i_amd import kernels as K
    K.filter_cache(False)        # as in a process that only evaluates: the training run above switched the cache on
    out = []
    for _ in range(2):
        np.random.seed(3); random.seed(3); torch.manual_seed(3)
        out.append(run.main(['--cfg', path, '--eval', 'is']))
    r = out[0]
    # the oracle chain over the same samples and permutation
    samples = denormalize_images(r['samples'].cpu().numpy())
    logits, _ = _Oracle(arrays)(_np_prep(samples[r['indices']]))
    print('IS %r / %r, oracle logits max |.| %.3g' % (r['mean'], r['std'], np.abs(logits).max()))
    assert np.isfinite(r['mean']) and np.isfinite(r['std']) and r['mean'] >= 1.0 - 1e-9
    assert (r['mean'], r['std']) == (out[1]['mean'], out[1]['std'])
    assert sorted(r['indices']) == list(range(16))
    m, s = get_inception_from_predictions(softmax32(logits), 10, verbose=False)
    assert abs(r['mean'] - m) <= 1e-4 * abs(m) and abs(r['std'] - s) <= 1e-4 * max(abs(s), 1e-3), (r['mean'], m, r['std'], s)

    res = []
    for _ in range(2):
        np.random.seed(4); random.seed(4); torch.manual_seed(4)
        res.append(run.main(['--cfg', path, '--eval', 'fid', '--incep-batch', '2']))
        if len(res) == 1:
            assert os.path.exists(cfg['EVAL']['ACT_STAT_PATH'])
            stamp = os.stat(cfg['EVAL']['ACT_STAT_PATH']).st_mtime_ns
    assert os.stat(cfg['EVAL']['ACT_STAT_PATH']).st_mtime_ns == stamp          # reused, not recomputed
    f = res[0]
    assert np.isfinite(f['fid']) and f['fid'] == res[1]['fid']
    assert np.array_equal(f['mu_gen'], res[1]['mu_gen']) and np.array_equal(f['sigma_gen'], res[1]['sigma_gen'])
    # the real statistics against the oracle over the decoded JPEGs (each resized from its own size)
    files = sorted(os.listdir(str(real_dir)))
    imgs = [to_rgb(np.asarray(Image.open(str(real_dir / n)))) for n in files]
    order = [files.index(n) for n in [os.path.basename(p) for p in _walk_order(str(tmp_path / 'real'))]]
    _, pre = _Oracle(arrays)(_np_prep([imgs[i] for i in order]))
    mu_ref, sig_ref = pre.mean(0), np.cov(pre, rowvar=False)
    assert np.abs(f['mu_real'] - mu_ref).max() <= 1e-4 * np.abs(mu_ref).max()
    assert np.abs(f['sigma_real'] - sig_ref).max() <= 1e-4 * np.abs(sig_ref).max()


def _walk_order(root):
    return [os.path.join(p, n) for p, _, files in os.walk(root) for n in files if 'jpg' in n or 'png' in n]
