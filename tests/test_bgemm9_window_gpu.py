"""bgemm9_kernel<1, true> (t2i_bgemm.hip): the fused F(2x2,2x2) input gradient of the 4x4 stride-2 layers with the input transform in
its A loader, K-tile outer / nine positions inner, every dy pixel of a tile's 3x3 window fetched once per K-tile (the centre pixel kept
in registers, the four edge pixels parked in thread-private LDS slots).  Each accumulator still sees its k in ascending order and a V
element is still (d[r][c] - d[1][c]) - (d[r][1] - d[1][1]) with absent taps as exact zeros, so the result must equal the three-kernel
path (input transform, 36 batched GEMMs, output transform) BIT FOR BIT; against the float64 direct oracle it is held to the 1e-5 of the
output scale that test_winograd_k4s2_matches_oracle uses.

Shapes: the smallest at which this loader can go wrong.
  B = 2, dy 4x4 -> dx 8x8     Th = Tw = 2: every tile touches a map edge (all window bits), T = 8 rows of a 64-row M tile
  B = 3, dy 6x10 -> dx 12x20  non-square, T = 45: ragged M tile, T no multiple of 4 (the loader addresses dy by pixel)
  channels (Cout = K, Cin = N) (64, 32), (96, 64), (160, 96): 2, 4 (padded from 3) and 6 (padded from 5) K-tiles — the padded one reads
                              zeros — and N below, equal to and ragged over one 64-column tile
  B = 8, dy 8x8, 64 -> 64     T = 128: 4 phases x 2 M tiles = 8 items.  A launch has min(ceil(items / 8), 64) workgroups per XCD, so
                              this gives ONE item per workgroup: any launch below 513 items does.  The smallest launch in which a workgroup
                              walks a second item (the loader switches window, phase and U planes in mid-pipeline) is the last case:
  B = 9, dy 64x64, 64 -> 32   T = 9216: 4 x 144 x 1 = 576 items, 72 per XCD on 64 workgroups: 8 workgroups per XCD walk TWO items."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5          # test_winograd_k4s2_matches_oracle's bound: max|d| / max|ref| against the float64 direct oracle


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


@pytest.fixture(scope='module', autouse=True)
def _small_shapes_on_the_winograd_path(K):
    """The library routes the input gradient here from 128 channels and ~400 work items up; lifted for this module (restored after)."""
    K.tuning_set('winograd_k4s2_minwork', 0)
    K.tuning_set('winograd_k4s2_minitems', 0)
    K.tuning_set('winograd_k4s2_bwd_minc', 32)
    yield
    K.tuning_set('winograd_k4s2_minwork', 160000000)
    K.tuning_set('winograd_k4s2_minitems', 400)
    K.tuning_set('winograd_k4s2_bwd_minc', 128)


def relerr(got, ref):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def run_case(K, capfd, B, Ho, Wo, Cout, Cin, epilogue, items, per_wg):
    """dy [B, Ho, Wo, Cout] -> dx [B, 2 Ho, 2 Wo, Cin]; epilogue False: plain, True: bias + lrelu."""
    from oracle import np_ops as O
    H, W = 2 * Ho, 2 * Wo
    rng = np.random.default_rng(B * 100000 + Ho * 1000 + Cout * 3 + Cin)
    w = (rng.standard_normal((4, 4, Cin, Cout)) / np.sqrt(16 * Cin)).astype(np.float32)
    dy = rng.standard_normal((B, Ho, Wo, Cout)).astype(np.float32)
    bi = rng.standard_normal(Cin).astype(np.float32)
    ref64 = O.conv2d_bwd_data(dy, w, (B, H, W, Cin), (2, 2), 'SAME')
    if epilogue:
        ref64 = O.lrelu(ref64 + bi)
    wd, dyd = torch.from_numpy(w).cuda(), torch.from_numpy(dy).cuda()
    bd = torch.from_numpy(bi).cuda() if epilogue else None
    act = (K.ACT_LRELU, 0.2) if epilogue else ()
    K.tuning_set('wino_fuse', 0)                     # the three-kernel path
    try:
        d, ws = K.conv_desc(B, H, W, Cin, Cout, 4, 4, 2, 2, 'SAME')
        assert K.conv_algo(d, 'bwd_data') == 'winograd_f2x2_2x2'
        ref = K.conv_bwd_data(dyd, wd, bd, d, ws, *act)
        K.tuning_set('wino_fuse', 2)                 # the fused kernel wherever its operand conditions hold ...
        K.tuning_set('wino_fuse_xf', 1)              # ... with the input transform in its loader
        K.tuning_set('debug_plan', 1)
        d2, ws2 = K.conv_desc(B, H, W, Cin, Cout, 4, 4, 2, 2, 'SAME')
        capfd.readouterr()
        got = K.conv_bwd_data(dyd, wd, bd, d2, ws2, *act)
        torch.cuda.synchronize()
        plan = capfd.readouterr().err
    finally:
        K.tuning_set('debug_plan', 0)
        K.tuning_set('wino_fuse', 1)
        K.tuning_set('wino_fuse_xf', 1)
    # this IS the kernel under test, with the item count the docstring states
    tm, tn = (B * (Ho // 2) * (Wo // 2) + 63) // 64, (Cin + 63) // 64
    assert 'fused gemm (loader transform): fused 9-position items, 4 phases x %d x %d tiles, K=%d' % (tm, tn, Cout) in plan, plan
    assert 4 * tm * tn == items and -(-items // (8 * min(-(-items // 8), 64))) == per_wg
    e_ref, e_got = relerr(ref, ref64), relerr(got, ref64)
    print('  B %d dy %dx%d %d -> %d%s: %d items, <= %d per workgroup; vs oracle: fused %.2e, unfused %.2e (bound %.0e); max |fused - unfused| %.1e'
          % (B, Ho, Wo, Cout, Cin, ' +bias+lrelu' if epilogue else '', items, per_wg, e_got, e_ref, TOL, float((got - ref).abs().max())))
    assert torch.equal(got, ref), float((got - ref).abs().max())
    assert e_got <= TOL, e_got


@pytest.mark.parametrize('chan', [(64, 32), (96, 64), (160, 96)])
@pytest.mark.parametrize('geom', [(2, 4, 4), (3, 6, 10)])
def test_window_loader_is_bit_identical(K, capfd, geom, chan):
    B, Ho, Wo = geom
    tm, tn = (B * (Ho // 2) * (Wo // 2) + 63) // 64, (chan[1] + 63) // 64
    run_case(K, capfd, B, Ho, Wo, chan[0], chan[1], False, 4 * tm * tn, 1)


@pytest.mark.parametrize('geom', [(2, 4, 4), (3, 6, 10)])
def test_window_loader_with_bias_and_lrelu(K, capfd, geom):
    """The epilogue (A^T M A + bias + activation) on the accumulators; the input gradient always scatters with sr = 2 (output pixel
    (2 (2 ty + r) + ph, 2 (2 tx + c) + pw)), so every case here covers it."""
    B, Ho, Wo = geom
    run_case(K, capfd, B, Ho, Wo, 96, 64, True, 4, 1)


def test_window_loader_eight_items(K, capfd):
    """B = 8, dy 8x8, 64 -> 64: two M tiles x four phases, one item per workgroup (see the module docstring)."""
    run_case(K, capfd, 8, 8, 8, 64, 64, False, 8, 1)


def test_window_loader_switches_item_in_mid_pipeline(K, capfd):
    """576 items on 512 workgroups: 64 workgroups walk two items, the others one; with bias + lrelu."""
    run_case(K, capfd, 9, 64, 64, 64, 32, True, 576, 2)
