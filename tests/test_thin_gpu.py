"""The direct kernels of csrc/t2i_thin.hip against float64 (tests/thin_cases.py), through the C ABI, on the branches the models' own
shapes do not take: every CI of the thin deconv, one / two / four passes, the CH == 64 fast path and the generic staging loop, LDS
above 48 KiB and up to the 160 KiB of a CU (and the shapes beyond it, which run on the implicit GEMM); tiny_conv with Cin != Cout,
k1 / k2 / k4s2 / VALID and its grid-stride loop; tiny_bwdw off k3 s1; the head kernels' scalar paths, Cout 2..4 and short K; the
stem off square images.

Bounds (tests/test_kernels_gpu.py): 1e-5 of max|ref| for forward, input gradient and transposed conv, 1e-4 for
filter gradients, 1e-5 for the stem's filter gradient (the bound test_stem_filter_gradient holds).  A case that needs more states its
own bound in thin_cases.STATED, at most min(1e-4, 4 x the float32 evaluation's error): tests/test_thin_host.py checks that.
On integer inputs in -3..3 every partial sum is an integer far below 2^24, so the result equals the reference exactly in any
summation order: a single wrong element has no tolerance to hide in.  Every filter gradient is run twice (same bits) and in its
accumulate form (base + reference at the same bound).  pytest -s prints every measured value."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import thin_cases as TC  # noqa: E402
from thin_cases import relerr  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'
THIN_PARTS_DEFAULT = 2


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEVICE).contiguous()


def dev_off(a):
    """the same values as a contiguous view that starts one float into a larger buffer: 4-byte aligned, not 16"""
    a = np.asarray(a, np.float32)
    buf = torch.zeros(a.size + 7, dtype=torch.float32, device=DEVICE)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a.copy()))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@contextlib.contextmanager
def described(K, case):
    """the case's switches set, its descriptor built AFTER them (tuning_set clears the descriptor cache), the switches restored"""
    parts = case.opt('thin_parts')
    try:
        if parts is not None:
            K.tuning_set('thin_parts', parts)
        B, H, W, Ci, Co, KH, KW, s, pad = case.shape
        d, ws = K.conv_desc(B, H, W, Ci, Co, KH, KW, s, s, pad)
        for e in case.entries:
            algo = K.conv_algo(d, e)
            assert (algo == 'direct_small') == (e in case.direct), (case.id, e, algo)
        yield d, ws
    finally:
        if parts is not None:
            K.tuning_set('thin_parts', THIN_PARTS_DEFAULT)


def drive(K, bd, case, d, ws, integer=False):
    """Every entry point of the case against its reference.  Random inputs: the forward with a bias, the filter gradient twice and in
    its accumulate form.  Integer inputs: no bias, no activation, exact."""
    I, R = TC.inputs(case, integer), TC.refs(case, integer)
    x, w, dy = dev(I['x']), dev(I['w']), dev(I['dy'])
    tag = ' int' if integer else ''
    if 'fwd' in case.entries:
        if integer:
            bd.exact('fwd' + tag, K.conv_fwd(x, w, None, d, ws), R['fwd'])
        else:
            bd.check('fwd', relerr(K.conv_fwd(x, w, dev(I['b']), d, ws), R['fwd'] + I['b']), case.tol('fwd'))
    if 'bwd_data' in case.entries:
        dx = K.conv_bwd_data(dy, w, None, d, ws)
        if integer:
            bd.exact('bwd_data' + tag, dx, R['bwd_data'])
        else:
            bd.check('bwd_data', relerr(dx, R['bwd_data']), case.tol('bwd_data'))
    if 'bwd_filter' in case.entries:
        dw = K.conv_bwd_filter(x, dy, d, ws)
        if integer:
            bd.exact('bwd_filter' + tag, dw, R['bwd_filter'])
        else:
            bd.check('bwd_filter', relerr(dw, R['bwd_filter']), case.tol('bwd_filter'))
        bd.same('bwd_filter' + tag + ' twice', torch.equal(dw, K.conv_bwd_filter(x, dy, d, ws)))
        if not integer:
            acc = dev(I['base'])
            K.conv_bwd_filter(x, dy, d, ws, out=acc)
            bd.check('bwd_filter accumulate', relerr(acc, I['base'].astype(np.float64) + R['bwd_filter']), case.tol('bwd_filter'))


# ---- thin deconv ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TC.THIN, **TC.ids(TC.THIN))
def test_thin_deconv(K, case):
    """thin_deconv_k4s2_kernel<CI> as the input gradient of a k4 s2 conv, one to four passes, up to 160 KiB of LDS; the three shapes no
    legal split brings under that run on the implicit GEMM and compute the same thing."""
    bd = TC.Bounds(case)
    with described(K, case) as (d, ws):
        drive(K, bd, case, d, ws)
        drive(K, bd, case, d, ws, integer=True)
    bd.done()


@pytest.mark.parametrize('mode', TC.THIN_MODES)
def test_thin_deconv_modes(K, mode):
    """The transposed-conv form (the generator's out_deconv: deconv_desc, bias over the 3 image channels, activation): bias alone, an
    activation alone, both; and dy, then w, as a view one float into a larger buffer, which the float4 staging cannot read: that call
    falls back to the GEMM and computes the same thing."""
    case = TC.THIN_MODES_CASE
    B, H, W, Ci, Co = case.shape[:5]
    I, R = TC.inputs(case), TC.refs(case)['bwd_data']
    d, ws = K.deconv_desc(B, H // 2, W // 2, Co, Ci, 4, 4, 2, 2, 'SAME')
    assert K.conv_algo(d, 'bwd_data') == 'direct_small'
    bi = I['bi'].astype(np.float64)
    dy, w = (dev_off if mode == 'dy_off' else dev)(I['dy']), (dev_off if mode == 'w_off' else dev)(I['w'])
    bias, act, ref = {'bias': (dev(I['bi']), K.ACT_NONE, R + bi), 'tanh': (None, K.ACT_TANH, np.tanh(R)),
                      'bias_lrelu': (dev(I['bi']), K.ACT_LRELU, TC.act(R + bi, 'lrelu'))}.get(mode, (None, K.ACT_NONE, R))
    bd = TC.Bounds(case)
    bd.check('bwd_data ' + mode, relerr(K.conv_bwd_data(dy, w, bias, d, ws, act, 0.2), ref), case.tol('bwd_data'))
    bd.done()


# ---- tiny conv ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TC.TINY, **TC.ids(TC.TINY))
def test_tiny_conv(K, case):
    """tiny_conv_kernel<false> and <true> (stride 1) with Cin != Cout, Cout = 1, k1 / k2 / k4s2, VALID; the filter gradients of these
    shapes (tiny_bwdw for the 3 -> 3 case, the GEMM otherwise) ride along."""
    bd = TC.Bounds(case)
    with described(K, case) as (d, ws):
        drive(K, bd, case, d, ws)
        drive(K, bd, case, d, ws, integer=True)
        if case.opt('variants'):
            I, R = TC.inputs(case), TC.refs(case)
            x, w, dy = dev(I['x']), dev(I['w']), dev(I['dy'])
            y = K.conv_fwd(x, w, dev(I['b']), d, ws, K.ACT_TANH)
            bd.check('fwd bias tanh', relerr(y, np.tanh(R['fwd'] + I['b'])), case.tol('fwd'))
            dx = K.conv_bwd_data(dy, w, dev(I['bi']), d, ws, K.ACT_LRELU, 0.2)      # the transposed-conv form: bias over Cin
            bd.check('bwd_data bias lrelu', relerr(dx, TC.act(R['bwd_data'] + I['bi'], 'lrelu')), case.tol('bwd_data'))
    bd.done()


def test_tiny_conv_grid_stride_loop(K):
    """1 059 968 output pixels: more than the 4096 x 256 threads of the capped grid, so the last 11 392 pixels are a second trip"""
    case = TC.TINY_LARGE
    B, H, W = case.shape[:3]
    assert B * H * W > 4096 * 256
    bd = TC.Bounds(case)
    with described(K, case) as (d, ws):
        drive(K, bd, case, d, ws)
    bd.done()


@pytest.mark.parametrize('case', TC.TINY_BWDW, **TC.ids(TC.TINY_BWDW))
def test_tiny_filter_gradient(K, case):
    """tiny_bwdw_kernel<3, 3> at k1, k2, 1 x 3, stride 2, odd extents, VALID and under 256 pixels"""
    bd = TC.Bounds(case)
    with described(K, case) as (d, ws):
        drive(K, bd, case, d, ws)
        drive(K, bd, case, d, ws, integer=True)
    bd.done()


# ---- head -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TC.HEAD, **TC.ids(TC.HEAD))
def test_head(K, case):
    """head_fwd / head_bwd_data / head_bwd_filter with Cout 2..4 (the scalar loop, the red[4][4] join), K % 4 != 0, K < 256 and < 64,
    B = 1, and Cout = 1 from a misaligned x or w (the scalar loop instead of the float4 one)."""
    bd = TC.Bounds(case)
    with described(K, case) as (d, ws):
        drive(K, bd, case, d, ws)
        drive(K, bd, case, d, ws, integer=True)
        I, R = TC.inputs(case), TC.refs(case)
        if case.opt('variants'):
            y = K.conv_fwd(dev(I['x']), dev(I['w']), dev(I['b']), d, ws, K.ACT_LRELU, 0.2)
            bd.check('fwd bias lrelu', relerr(y, TC.act(R['fwd'] + I['b'], 'lrelu')), case.tol('fwd'))
        if case.opt('offsets'):
            for name, put_x, put_w in (('x off', dev_off, dev), ('w off', dev, dev_off)):
                x, w, dy = put_x(I['x']), put_w(I['w']), dev(I['dy'])
                bd.check('fwd ' + name, relerr(K.conv_fwd(x, w, dev(I['b']), d, ws), R['fwd'] + I['b']), case.tol('fwd'))
                bd.check('bwd_data ' + name, relerr(K.conv_bwd_data(dy, w, None, d, ws), R['bwd_data']), case.tol('bwd_data'))
                bd.check('bwd_filter ' + name, relerr(K.conv_bwd_filter(x, dy, d, ws), R['bwd_filter']), case.tol('bwd_filter'))
    bd.done()


# ---- stem -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TC.STEM, **TC.ids(TC.STEM))
def test_stem(K, case):
    """stem_k4s2_fwd_kernel and stem_k4s2_bwdf_kernel off square images: H != W, Wo = 40 (a ragged second column block), Ho = 1 and
    Ho = 5 (no multiple of 4), with and without bias, every activation, and a misaligned bias (the call falls back)."""
    bd = TC.Bounds(case)
    with described(K, case) as (d, ws):
        drive(K, bd, case, d, ws)
        drive(K, bd, case, d, ws, integer=True)
        I, R = TC.inputs(case), TC.refs(case)['fwd']
        x, w, b = dev(I['x']), dev(I['w']), dev(I['b'])
        tol = case.tol('fwd')
        bd.check('fwd bias lrelu', relerr(K.conv_fwd(x, w, b, d, ws, K.ACT_LRELU, 0.2), TC.act(R + I['b'], 'lrelu')), tol)
        bd.check('fwd plain', relerr(K.conv_fwd(x, w, None, d, ws), R), tol)
        bd.check('fwd bias tanh', relerr(K.conv_fwd(x, w, b, d, ws, K.ACT_TANH), np.tanh(R + I['b'])), tol)
        if case.opt('bias_off'):
            y = K.conv_fwd(x, w, dev_off(I['b']), d, ws, K.ACT_LRELU, 0.2)
            bd.check('fwd bias off lrelu', relerr(y, TC.act(R + I['b'], 'lrelu')), tol)
    bd.done()


# ---- the pair entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first', ['bwd_data', 'fwd'])
@pytest.mark.parametrize('case', TC.PAIR, **TC.ids(TC.PAIR))
def test_pair_equals_the_two_calls_bit_for_bit(K, case, first):
    """t2i_conv2d_bwd_pair in fp32 storage on the direct kernels: the same bits as t2i_conv2d_bwd_data (or t2i_conv2d_fwd) followed by
    t2i_conv2d_bwd_filter, as its header promises; accumulating and storing."""
    bd = TC.Bounds(case)
    with described(K, case) as (d, ws):
        I, R = TC.inputs(case), TC.refs(case)
        x, w, dy = dev(I['x']), dev(I['w']), dev(I['dy'])
        if first == 'bwd_data':
            code, g, alone = K.PAIR_BWD_DATA, dy, K.conv_bwd_data(dy, w, None, d, ws)
        else:
            code, g, alone = K.PAIR_FWD, x, K.conv_fwd(x, w, None, d, ws)
        bd.check(first, relerr(alone, R[first]), case.tol(first))
        for accumulate in (True, False):
            sep, both = dev(I['base']), dev(I['base'])
            K.conv_bwd_filter(x, dy, d, ws, out=sep, accumulate=accumulate)
            out1 = K.conv_bwd_pair(code, g, w, x, dy, d, ws, both, accumulate=accumulate)
            name = 'accumulate' if accumulate else 'store'
            bd.same('%s %s' % (first, name), torch.equal(out1, alone))
            bd.same('bwd_filter ' + name, torch.equal(both, sep))
            want = R['bwd_filter'] + (I['base'].astype(np.float64) if accumulate else 0.0)
            bd.check('bwd_filter ' + name, relerr(both, want), case.tol('bwd_filter'))
    bd.done()
