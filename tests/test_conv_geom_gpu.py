"""The three convolution entry points against float64 (tests/conv_geom_cases.py), through the C ABI, over the geometry space the
descriptor admits and the models use: non-square kernels, 5 x 5, stride 2 and 3 VALID with unequal, empty and one-tap stride phases,
rectangular strides, kernels larger than the map, asymmetric padding, conv2d_transpose VALID, the pixel walk, the last kernel on the
bf16 tap-mask path and the first one off it, and both sides of every term of the Winograd eligibility rules; each on the scalar, the
vector and the tap-uniform address path of the fp32 GEMM and, with 64-multiple channels, on the bf16-operand kernels.

Integer inputs in -2..2: every intermediate of every path is exactly representable (conv_geom_cases derives the bound,
tests/test_conv_geom_host.py asserts it per case), so the result must EQUAL the float64 reference, whatever the tile, split-K grouping or
accumulation order, in fp32 and in bf16 math; with bf16 storage y and dx equal its RNE bf16 rounding.  Gaussian inputs: the project's
own bounds (tests/test_kernels_gpu.py): 1e-5 of max|ref| forward, 1e-4 for the gradients; for bf16 math the
oracle runs on the RNE-rounded operands.  pytest -s prints every measured value; profiles/conv_geom_parity.txt keeps one such run."""
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

import conv_geom_cases as GC  # noqa: E402
from conv_geom_cases import relerr  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = 'cuda'
FORCED_WS = 256 << 20          # forced splits can exceed the planner's own workspace estimate (test_every_tile_and_split_config)


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEVICE).to(dtype).contiguous()


@contextlib.contextmanager
def described(K, case, math, forced=None):
    """the case's switches (and the forced tile / split, with the direct kernels off) set, its descriptor built AFTER them (tuning_set
    clears the descriptor cache), the routing the case names asserted, the switches restored"""
    switches = dict(case.switches)
    switches.update(forced or {})
    try:
        for k, v in switches.items():
            K.tuning_set(k, v)
        B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
        mcode = K.MATH_BF16 if math == 'bf16' else K.MATH_F32
        if case.opt('deconv'):
            h, w = case.opt('deconv')
            d, ws = K.deconv_desc(B, h, w, Co, Ci, KH, KW, SH, SW, pad, math=mcode)
        else:
            d, ws = K.conv_desc(B, H, W, Ci, Co, KH, KW, SH, SW, pad, math=mcode)
        assert d.math == mcode and (d.H, d.W, d.Ho, d.Wo) == (H, W) + GC.geometry(case)[:2]
        if not forced:
            for e, algo in case.algos(math).items():
                assert K.conv_algo(d, e) == algo, (case.id, math, e, K.conv_algo(d, e))
        yield d, (FORCED_WS if forced else ws)
    finally:
        for k in switches:
            K.tuning_set(k, GC.SWITCH_DEFAULTS[k])


def drive_integer(K, bd, case, d, ws, tag, stored=False):
    """every entry point on the integer inputs, equality only.  stored: the activation tensors are handed in with the dtype the
    wrappers allocate such a tensor with (bf16 storage: bf16 with 64-multiple channels); an output that comes back as bf16 must equal
    the RNE rounding of the exact result, the filter gradient the exact result in fp32."""
    I, R = GC.inputs(case, True), GC.refs(case, True)
    store = (lambda a: K._act_dtype(a.shape)) if stored else (lambda a: torch.float32)      # noqa: E731
    x, dy, w = dev(I['x'], store(I['x'])), dev(I['dy'], store(I['dy'])), dev(I['w'])
    b, bi = I['b'].astype(np.float64), I['bi'].astype(np.float64)
    kind = lambda t: 'bf16' if t.dtype == torch.bfloat16 else np.float32      # noqa: E731
    if 'fwd' in case.entries:
        for name, bias, act, ref in (('fwd', None, K.ACT_NONE, R['fwd']), ('fwd bias relu', dev(I['b']), K.ACT_RELU, GC.act(R['fwd'] + b, 'relu')),
                                     ('fwd bias lrelu', dev(I['b']), K.ACT_LRELU, GC.act(R['fwd'] + b, 'lrelu'))):
            y = K.conv_fwd(x, w, bias, d, ws, act, GC.LRELU_ALPHA)
            bd.exact('%s %s' % (tag, name), y, ref, kind(y))
    if 'bwd_data' in case.entries:
        for name, bias, act, ref in (('bwd_data', None, K.ACT_NONE, R['bwd_data']),
                                     ('bwd_data bias relu', dev(I['bi']), K.ACT_RELU, GC.act(R['bwd_data'] + bi, 'relu'))):
            dx = K.conv_bwd_data(dy, w, bias, d, ws, act, GC.LRELU_ALPHA)
            bd.exact('%s %s' % (tag, name), dx, ref, kind(dx))
        if case.opt('deconv'):                               # the transposed conv through the oracle's own entry: bias, no activation
            dx = K.conv_bwd_data(dy, w, dev(I['bi']), d, ws)
            bd.exact(tag + ' transpose bias', dx, GC.transpose_ref(case, True), kind(dx))
    if 'bwd_filter' in case.entries:
        dw = K.conv_bwd_filter(x, dy, d, ws)
        assert dw.dtype == torch.float32
        bd.exact(tag + ' bwd_filter', dw, R['bwd_filter'])
        acc = dev(I['base'])
        K.conv_bwd_filter(x, dy, d, ws, out=acc)
        bd.exact(tag + ' bwd_filter accumulate', acc, R['bwd_filter'] + I['base'].astype(np.float64))


def drive_gaussian(K, bd, case, d, ws, math):
    """the same entry points on the Gaussian inputs against the float64 oracle (bf16 math: on the RNE-rounded operands)"""
    I, R = GC.inputs(case), GC.refs(case, False, math == 'bf16')
    x, dy, w = dev(I['x']), dev(I['dy']), dev(I['w'])
    b, bi = I['b'].astype(np.float64), I['bi'].astype(np.float64)
    if 'fwd' in case.entries:
        tol = case.tol('fwd')
        bd.check('fwd %s' % math, relerr(K.conv_fwd(x, w, None, d, ws), R['fwd']), tol)
        bd.check('fwd bias relu %s' % math, relerr(K.conv_fwd(x, w, dev(I['b']), d, ws, K.ACT_RELU), GC.act(R['fwd'] + b, 'relu')), tol)
        y = K.conv_fwd(x, w, dev(I['b']), d, ws, K.ACT_LRELU, GC.LRELU_ALPHA)
        bd.check('fwd bias lrelu %s' % math, relerr(y, GC.act(R['fwd'] + b, 'lrelu')), tol)
    if 'bwd_data' in case.entries:
        tol = case.tol('bwd_data')
        bd.check('bwd_data %s' % math, relerr(K.conv_bwd_data(dy, w, None, d, ws), R['bwd_data']), tol)
        dx = K.conv_bwd_data(dy, w, dev(I['bi']), d, ws, K.ACT_RELU)
        bd.check('bwd_data bias relu %s' % math, relerr(dx, GC.act(R['bwd_data'] + bi, 'relu')), tol)
    if 'bwd_filter' in case.entries:
        tol = case.tol('bwd_filter')
        bd.check('bwd_filter %s' % math, relerr(K.conv_bwd_filter(x, dy, d, ws), R['bwd_filter']), tol)
        acc = dev(I['base'])
        K.conv_bwd_filter(x, dy, d, ws, out=acc)
        bd.check('bwd_filter accumulate %s' % math, relerr(acc, I['base'].astype(np.float64) + R['bwd_filter']), tol)


def maths(case):
    return ('f32', 'bf16') if case.algo_h else ('f32',)


@pytest.mark.parametrize('case', GC.ALL, **GC.ids(GC.ALL))
def test_integer_inputs_equal_the_oracle(K, case):
    """fwd (plain, bias + relu, bias + lrelu 0.25), bwd_data (plain, bias + relu), bwd_filter (plain, accumulate into integers): bit
    equality with the float64 reference, in fp32 math and, where the channels admit it, in bf16 math."""
    bd = GC.Bounds(case)
    for math in maths(case):
        with described(K, case, math) as (d, ws):
            drive_integer(K, bd, case, d, ws, math)
    bd.done()


PHASE_CASES = [c for c in GC.GEOMETRY if c.tag in GC.PHASE_TAGS]


@pytest.mark.parametrize('case', PHASE_CASES, **GC.ids(PHASE_CASES))
def test_phase_rows_under_every_forced_tile_and_split(K, case):
    """the stride-phase rows again under force_tile in {22, 11} x force_splitk in {1, 3} with the direct kernels off: unequal and empty
    phases in every K-slab of a split, on the largest and the smallest tile"""
    bd = GC.Bounds(case)
    for math in maths(case):
        for tile in (22, 11):
            for splitk in (1, 3):
                with described(K, case, math, dict(force_tile=tile, force_splitk=splitk, no_thin=1)) as (d, ws):
                    drive_integer(K, bd, case, d, ws, '%s t%d s%d' % (math, tile, splitk))
    bd.done()


OTHER_ROWS = [c for c in GC.GEOMETRY + GC.WALK if c.tag not in GC.PHASE_TAGS]


@pytest.mark.parametrize('case', OTHER_ROWS, **GC.ids(OTHER_ROWS))
def test_other_rows_under_the_largest_and_the_smallest_forced_plan(K, case):
    """the rows without unequal phases (non-square kernels, 5 x 5, kernels larger than the map, asymmetric padding, the transposed
    conv, the pixel walk) on the 128 x 128 tile split three ways and on the 64 x 64 tile unsplit: border taps in every K-slab"""
    bd = GC.Bounds(case)
    for math in maths(case):
        for tile, splitk in ((22, 3), (11, 1)):
            with described(K, case, math, dict(force_tile=tile, force_splitk=splitk, no_thin=1)) as (d, ws):
                drive_integer(K, bd, case, d, ws, '%s t%d s%d' % (math, tile, splitk))
    bd.done()


BF16_CASES =[c for c in GC.ALL if c.algo_h]


@pytest.mark.parametrize('case', BF16_CASES, **GC.ids(BF16_CASES))
def test_bf16_storage_rounds_the_exact_result(K, case):
    """the bf16-operand cases with bf16 tensors in and out (K.set_storage('bf16')): y and dx are the RNE bf16 rounding of the exact
    result wherever the wrapper allocates them as bf16 (64-multiple channels), dw is the exact result in fp32"""
    B, H, W, Ci, Co = case.shape[:5]
    Ho, Wo = GC.geometry(case)[:2]
    bd = GC.Bounds(case)
    K.set_math('bf16')
    K.set_storage('bf16')
    try:
        assert (K._act_dtype((B, Ho, Wo, Co)) is torch.bfloat16) == (Co % 64 == 0 and (B * Ho * Wo * Co) % 8 == 0)
        assert (K._act_dtype((B, H, W, Ci)) is torch.bfloat16) == (Ci % 64 == 0 and (B * H * W * Ci) % 8 == 0)
        with described(K, case, 'bf16') as (d, ws):
            drive_integer(K, bd, case, d, ws, 'stored', stored=True)
    finally:
        K.set_storage('f32')
        K.set_math('f32')
    bd.done()


@pytest.mark.parametrize('case', GC.ALL, **GC.ids(GC.ALL))
def test_gaussian_inputs_meet_the_project_bounds(K, case):
    bd = GC.Bounds(case)
    for math in maths(case):
        with described(K, case, math) as (d, ws):
            drive_gaussian(K, bd, case, d, ws, math)
    bd.done()


def test_unsupported_geometry_is_refused(K):
    """a stride above 4 (more than 16 phases) is unsupported by design: every entry point refuses it with an error, none computes"""
    d, ws = K.conv_desc(1, 10, 10, 8, 8, 3, 3, 5, 5, 'SAME')
    x, w, dy = torch.ones(1, 10, 10, 8, device=DEVICE), torch.ones(3, 3, 8, 8, device=DEVICE), torch.ones(1, 2, 2, 8, device=DEVICE)
    for call in (lambda: K.conv_fwd(x, w, None, d, ws), lambda: K.conv_bwd_data(dy, w, None, d, ws), lambda: K.conv_bwd_filter(x, dy, d, ws)):
        with pytest.raises(RuntimeError, match='stride > 4'):
            call()


@pytest.mark.parametrize('pair', GC.WINO_PAIRS, ids=['%s-%s-%s' % p for p in GC.WINO_PAIRS])
def test_routing_pairs_are_both_exact(K, pair):
    """A just-eligible and a just-ineligible Winograd or bf16-path case of the same kernel geometry are both exact on integer inputs;
    where the two sides are the same shape under another switch, the fast path and its fallback agree bit for bit."""
    fam, inside, outside = pair
    a, b = GC.by_tag(fam, inside), GC.by_tag('k16' if fam == 'k15' else fam, outside)
    math = 'bf16' if fam in ('k15', 'hf') else 'f32'        # the arithmetic whose routing the pair is about
    out = {}
    for case in (a, b):
        bd = GC.Bounds(case)
        I, R = GC.inputs(case, True), GC.refs(case, True)
        with described(K, case, math) as (d, ws):
            got = (K.conv_fwd(dev(I['x']), dev(I['w']), None, d, ws), K.conv_bwd_data(dev(I['dy']), dev(I['w']), None, d, ws),
                   K.conv_bwd_filter(dev(I['x']), dev(I['dy']), d, ws))
        for e, t in zip(GC.ENTRIES, got):
            bd.exact('%s %s' % (math, e), t, R[e])
        bd.done()
        out[case.id] = got
    if a.shape == b.shape:
        # (the inputs are seeded from the case id, so the two sides ran on different data: run the fallback on the fast side's)
        I = GC.inputs(a, True)
        with described(K, b, math) as (d, ws):
            again = (K.conv_fwd(dev(I['x']), dev(I['w']), None, d, ws), K.conv_bwd_data(dev(I['dy']), dev(I['w']), None, d, ws),
                     K.conv_bwd_filter(dev(I['x']), dev(I['dy']), d, ws))
        for e, t, u in zip(GC.ENTRIES, out[a.id], again):
            assert torch.equal(t, u), (pair, e)
