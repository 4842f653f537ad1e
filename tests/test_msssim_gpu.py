"""Multi-scale SSIM on the GPU: t2i_ssim_scale against the float64 restatement of tests/msssim_cases.py (scipy.signal for the
moments, scipy.ndimage for the downsample), the five-scale chain under graph capture, MultiScaleSSIM end to end and
GeneratorEval.evaluate_msssim."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import msssim_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

# |delta ssim|, |delta cs| per image.  Each moment is at most 121 terms of magnitude at most 65025 summed in fp64: about 9e-10 of
# absolute error in the worst case, divided by v2 >= 58.5.  (Two fp64 summation orders, separable against direct 2-D, differ by at
# most 1e-12 on these families on the CPU; an fp32-moment kernel misses the bound on `flat` by four orders of magnitude.)
BOUND = 1e-9


@pytest.fixture(scope='module')
def K():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


# ---- one scale -------------------------------------------------------------------------------------------------------------------
SHAPES = [((2, 16, 16, 3), 11),                          # baseline
          ((2, 37, 53, 3), 11),                          # odd sides, partial tiles, a clamped last downsample row and column
          ((3, 48, 80, 2), 11),                          # several tiles both ways
          ((1, 64, 64, 1), 11),                          # single channel
          ((2, 8, 8, 3), 8),                             # even window
          ((2, 4, 6, 4), 4),                             # small even window, four channels
          ((1, 11, 11, 2), 11),                          # a 1 x 1 map
          ((1, 1, 1, 1), 1)]                             # degenerate


@pytest.mark.parametrize('family', MC.FAMILIES)
@pytest.mark.parametrize('shape,S', SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_one_scale_matches_the_restatement(K, shape, S, family):
    a, b = MC.pairs(family, 1, *shape)
    want_ssim, want_cs = MC.scale_reference(family, 1, shape)
    win = K.msssim_window(shape[1], shape[2])
    assert win.shape == (S,)
    da, db = dev(a), dev(b)
    ssim, cs, ah, bh = K.ssim_scale(da, db, win, MC.C1, MC.C2)
    ssim2, cs2, ah2, bh2 = K.ssim_scale(da, db, win, MC.C1, MC.C2)
    ssim3, cs3, none_a, none_b = K.ssim_scale(da, db, win, MC.C1, MC.C2, downsample=False)
    torch.cuda.synchronize()
    e_ssim = np.abs(ssim.cpu().numpy() - want_ssim).max()
    e_cs = np.abs(cs.cpu().numpy() - want_cs).max()
    print('%s %s: max |delta ssim| %.3g, max |delta cs| %.3g (bound %.3g)' % (family, shape, e_ssim, e_cs, BOUND))
    assert ssim.dtype == cs.dtype == torch.float64 and tuple(ssim.shape) == tuple(cs.shape) == (shape[0],)
    assert e_ssim <= BOUND and e_cs <= BOUND
    # the next scale, bit for bit; the clamped last row and column on their own
    for got, x in ((ah, a), (bh, b)):
        want = MC.downsample(x)
        g = got.cpu().numpy()
        assert g.shape == want.shape == (shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2, shape[3]) and g.dtype == np.float32
        assert np.array_equal(g[:, -1], want[:, -1]), 'last row'
        assert np.array_equal(g[:, :, -1], want[:, :, -1]), 'last column'
        assert np.array_equal(g[:, :-1, :-1], want[:, :-1, :-1]), 'interior'
        assert np.array_equal(g.astype(np.float64), MC.downsample_scipy(x))             # integer levels: scipy's means are exact
    # repeats bit for bit, with and without the downsample
    assert torch.equal(ssim, ssim2) and torch.equal(cs, cs2) and torch.equal(ah, ah2) and torch.equal(bh, bh2)
    assert torch.equal(ssim, ssim3) and torch.equal(cs, cs3) and none_a is None and none_b is None


def test_more_workgroups_than_one_launch_takes(K):
    """2^20 + 37 pairs of 1 x 1 x 1 images: one tile each, more than the 2^20 workgroups of a launch, so the first workgroups take
    a second tile and the fold a second pair.  With S = 1 the map is one pixel: cs = 1 and ssim = (2ab + c1) / (a^2 + b^2 + c1)."""
    n = (1 << 20) + 37
    rng = np.random.RandomState(9)
    a = rng.randint(0, 256, size=(n, 1, 1, 1)).astype(np.float32)
    b = rng.randint(0, 256, size=(n, 1, 1, 1)).astype(np.float32)
    ssim, cs, ah, bh = K.ssim_scale(dev(a), dev(b), K.msssim_window(1, 1), MC.C1, MC.C2)
    a64, b64 = a.reshape(n).astype(np.float64), b.reshape(n).astype(np.float64)
    want = (2 * a64 * b64 + MC.C1) / (a64 * a64 + b64 * b64 + MC.C1)
    assert np.abs(ssim.cpu().numpy() - want).max() <= BOUND and np.abs(cs.cpu().numpy() - 1).max() <= BOUND
    assert np.array_equal(ah.cpu().numpy(), a) and np.array_equal(bh.cpu().numpy(), b)


# ---- capture -----------------------------------------------------------------------------------------------------------------------
def _chain(K, a, b):
    """The five scales: a linear chain of launches."""
    ssim, cs = [], []
    for l in range(5):
        s, c, a, b = K.ssim_scale(a, b, K.msssim_window(a.shape[1], a.shape[2]), MC.C1, MC.C2, downsample=l < 4)
        ssim.append(s)
        cs.append(c)
    return torch.stack(ssim), torch.stack(cs)


def test_five_scales_captured_in_a_graph_replay_bit_for_bit(K):
    shape = (3, 37, 53, 3)
    a0, b0 = MC.pairs('near', 2, *shape)
    a1, b1 = MC.pairs('indep', 3, *shape)
    sa, sb = dev(a0), dev(b0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up: the workspace exists before the capture
        _chain(K, sa, sb)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_ssim, g_cs = _chain(K, sa, sb)
    for x, y in ((a0, b0), (a1, b1)):
        sa.copy_(dev(x)); sb.copy_(dev(y))
        graph.replay()
        torch.cuda.synchronize()
        e_ssim, e_cs = _chain(K, dev(x), dev(y))
        assert torch.equal(g_ssim, e_ssim) and torch.equal(g_cs, e_cs)
    want = MC.msssim_reference('indep', 3, shape)
    assert np.abs(g_ssim.cpu().numpy() - want['ssim']).max() <= BOUND and np.abs(g_cs.cpu().numpy() - want['cs']).max() <= BOUND


# ---- MultiScaleSSIM ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['near', 'flat', 'neg'])
@pytest.mark.parametrize('adds,shape', [(2, (4, 32, 32, 3)), (1, (2, 64, 64, 3))], ids=['2x4x32', '1x2x64'])
def test_msssim_end_to_end(K, adds, shape, family):
    """Two adds of four 32 x 32 x 3 pairs (windows 11, 11, 8, 4, 2) and one add of two 64 x 64 x 3 pairs (11, 11, 11, 8, 4)."""
    from t2i_amd.evaluation.msssim import MultiScaleSSIM
    ms = MultiScaleSSIM(shape[1:], 'cuda')
    refs = []
    for seed in range(1, adds + 1):
        a, b = MC.pairs(family, seed, *shape)
        ms.add(dev(a), dev(b), quantized=True)
        refs.append(MC.msssim_reference(family, seed, shape))
    out = ms.finalize()
    want = np.concatenate([r['values'] for r in refs])
    want_cs = np.concatenate([r['cs'] for r in refs], 1).mean(axis=1)
    e_v, e_c = np.abs(out['values'] - want).max(), np.abs(np.array(out['cs_levels']) - want_cs).max()
    print('%s %s x %d: values %s, max |delta| %.3g, cs_levels max |delta| %.3g, clamped %d' % (family, shape, adds, out['values'][:2], e_v, e_c,
                                                                                      out['clamped']))
    assert out['values'].dtype == np.float64 and out['values'].shape == (adds * shape[0],) and len(out['cs_levels']) == 5
    assert e_v <= BOUND and e_c <= BOUND
    assert out['clamped'] == sum(r['clamped'] for r in refs)
    assert out['mean'] == pytest.approx(want.mean(), abs=BOUND) and out['std'] == pytest.approx(want.std(), abs=BOUND)
    assert out['sides'][0] == shape[1:3] and out['sides'][-1] == (shape[1] // 16, shape[2] // 16)
    if family == 'neg':
        assert np.all(out['values'] == 0.0) and out['clamped'] > 0
    else:
        assert out['clamped'] == 0 and np.all(out['values'] > 0.9)


def test_identical_images_score_one_and_quantize_is_numpys(K):
    from t2i_amd.evaluation import msssim
    rng = np.random.RandomState(6)
    x = rng.uniform(-1.1, 1.1, size=(3, 32, 48, 3)).astype(np.float32)
    x[0, 0, :8, 0] = [-1.0, 1.0, 0.0, 1.0 / 255, -1.0 / 255, 0.5 / 127.5 - 1, 0.00392, -0.99608]
    q = msssim.quantize(dev(x))
    want = np.clip(np.round(x * np.float32(127.5) + np.float32(127.5)), 0, 255).astype(np.float32)
    assert np.array_equal(q.cpu().numpy(), want)
    ms = msssim.MultiScaleSSIM((32, 48, 3), 'cuda')
    ms.add(dev(x), dev(x))                                # quantized=False: through quantize()
    ms.add(q, q.clone(), quantized=True)
    out = ms.finalize()
    assert out['values'].shape == (6,) and np.abs(out['values'] - 1).max() <= 1e-12 and out['clamped'] == 0
    assert np.array_equal(out['values'][:3], out['values'][3:])


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('source', ['cond', 'z'])
def test_evaluate_msssim_with_stub_generators(K, source, capsys):
    """A generator that is a function of the caption only scores 1 on 'caption' pairs (it ignores z: the failure this metric is
    for) and below 1 on 'random' pairs; a function of z only scores below 1 on both.  Two runs give the same bits."""
    from t2i_amd.evaluation.evaluator import GeneratorEval
    from t2i_amd.utils.config import AttrDict
    g = torch.Generator().manual_seed(3)
    proj = {'cond': torch.randn(8, 16 * 16 * 3, generator=g).cuda(), 'z': torch.randn(4, 16 * 16 * 3, generator=g).cuda()}

    class Split(object):
        def next_batch(self, bs, k, embeddings=True):
            return None, None, np.random.standard_normal((bs, 8)).astype(np.float32), None, None

    class Data(object):
        pass

    class Model(object):
        device, z_dim, embed_dim = torch.device('cuda'), 4, 8

    class Ev(GeneratorEval):
        def restore(self):
            self.restored = True

        def generate_batch(self, z, cond, is_training):
            assert not is_training
            return torch.tanh((cond if source == 'cond' else z) @ proj[source]).reshape(-1, 16, 16, 3)

    def run(pairs):
        data = Data()
        data.test = Split()
        ev = Ev(None, Model(), data, AttrDict({'EVAL': {'SIZE': 13, 'SAMPLE_SIZE': 4, 'INCEP_BATCH_SIZE': 4}}))
        np.random.seed(5)
        out = ev.evaluate_msssim(pairs=pairs)
        assert ev.restored
        return out

    for pairs, count in (('random', 3 * 4 // 2), ('caption', 3 * 4)):
        a = run(pairs)
        text = capsys.readouterr().out
        b = run(pairs)
        assert a['values'].shape == (count,) and np.array_equal(a['values'], b['values']) and a['cs_levels'] == b['cs_levels']
        assert a['mean'] == b['mean'] and a['std'] == b['std'] and a['clamped'] == b['clamped'] and a['sides'][0] == (16, 16)
        assert 'MS-SSIM (%s) | mean: %.4f std: %.4f clamped: %d' % (pairs, a['mean'], a['std'], a['clamped']) in text
        print(source, pairs, a['values'])
        if source == 'cond' and pairs == 'caption':
            assert np.abs(a['values'] - 1).max() <= 1e-12
        else:
            assert np.all(a['values'] < 1 - 1e-6)
    kept = run('caption')
    assert 'samples' not in kept
