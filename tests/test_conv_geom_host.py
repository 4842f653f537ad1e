"""The cases of tests/conv_geom_cases.py without a GPU: their float64 references against float64 torch convolutions (so that
tests/test_conv_geom_gpu.py does not rest on one implementation), their sensitivity to the indexing errors they are there to catch, the
exactness condition of the integer inputs, the census of the models' own layer geometries, and the routing of every case through
t2i_conv2d_algo, which is host logic."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_geom_cases as GC  # noqa: E402

RTOL = 1e-12


@pytest.fixture(scope='module')
def K():
    lib = os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')
    if not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels
    return kernels


def test_case_ids_are_unique_and_every_table_is_listed():
    seen = [c.id for c in GC.ALL]
    assert len(set(seen)) == len(seen), sorted(i for i in seen if seen.count(i) > 1)
    assert {name: len(t) for name, t in GC.TABLES.items()} == GC.TABLE_LENGTHS
    assert sum(GC.TABLE_LENGTHS.values()) == len(GC.ALL)
    for c in GC.ALL:
        assert set(c.entries) <= set(GC.ENTRIES) and len(c.algo) == 3 and (c.algo_h is None or len(c.algo_h) == 3), c.id
        assert set(c.algo + (c.algo_h or '')) <= set(GC.ALGO_WORDS), c.id
        assert set(k for k, _ in c.sw) <= set(GC.SWITCH_DEFAULTS) | {'deconv'}, c.id


def test_every_geometry_row_has_every_channel_class():
    """each geometry row once per channel class, the class's channel counts on the address path it names"""
    rows = {}
    for c in GC.GEOMETRY:
        rows.setdefault(c.shape[:3] + c.shape[5:] + (c.tag,), []).append(c)
    assert len(rows) == len(GC.GEOMETRY_ROWS) == 23
    for row, cases in rows.items():
        assert [c.cls for c in cases] == list(GC.CLASSES), row
    for c in GC.GEOMETRY + GC.H_FILTER + GC.WALK + GC.K15:
        Ci, Co = c.shape[3:5]
        want = {'v0': Ci % 4 != 0 and Co % 4 != 0, 'v1': Ci % 4 == 0 and Co % 4 == 0 and Ci % 32 != 0 and Co % 32 != 0,
                'v2': Ci % 32 == 0 and Co % 32 == 0, 'h': Ci % 64 == 0}[c.cls]
        assert want, c.id
        assert c.algo_h is not None or c.cls != 'h', c.id
    for c in GC.GEOMETRY:
        assert (c.algo_h is not None) == (c.cls == 'h'), c.id
    for c in GC.ALL:                                        # the bf16 word: the rule restated, also where a table states it
        assert c.algo_h == (GC.h_word(c.shape) if 'H' in GC.h_word(c.shape) else None), c.id
    tags = set(c.tag for c in GC.GEOMETRY)
    assert tags == {'k1x7', 'k7x1', 'k1x3', 'k3x1', 'k5', 'k3s2v', 'k3s2s', 'k1s2', 'k2s3', 'k3s3', 's2x1', 's1x2', 'big_k', 'k4s1', 'deconv_v'}
    assert set(GC.PHASE_TAGS) <= tags and all(c.phases for c in GC.GEOMETRY if c.tag in GC.PHASE_TAGS)
    assert sorted(GC.geometry(c)[1] for c in GC.WALK) == [1, 2, 2, 3, 16, 32] and all(c.shape[1] != c.shape[2] for c in GC.WALK)


def test_phase_rows_have_the_phases_they_name():
    """unequal phases 4C / 2C / 2C / C for k3 s2, on both parities of the phase origin; empty phases for k < s; one tap each for k3 s3"""
    taps = lambda tag, hw: sorted(p[4] * p[5] for p in GC.phase_table(next(c for c in GC.GEOMETRY if c.tag == tag and c.shape[1:3] == hw)))  # noqa: E731
    assert taps('k3s2v', (7, 9)) == taps('k3s2s', (8, 8)) == taps('k3s2s', (7, 7)) == [1, 2, 2, 4]
    origin = lambda hw: [p[2] for p in GC.phase_table(next(c for c in GC.GEOMETRY if c.tag == 'k3s2s' and c.shape[1:3] == hw))][::2]  # noqa: E731
    assert origin((8, 8)) == [0, 1] and origin((7, 7)) == [1, 0]
    assert taps('k1s2', (8, 6)) == [0, 0, 0, 1] and taps('k2s3', (10, 10)) == [0, 0, 0, 0, 0, 1, 1, 1, 1] and taps('k3s3', (10, 10)) == [1] * 9
    assert taps('s2x1', (8, 12)) == [3, 6]
    # VALID geometries that leave trailing input rows / columns unused: dx is exactly 0 there
    for tag, hw, rows, cols in (('k3s2v', (8, 10), 1, 1), ('k2s3', (10, 10), 2, 2), ('k3s3', (10, 10), 1, 1)):
        for c in (c for c in GC.GEOMETRY if c.tag == tag and c.shape[1:3] == hw):
            dx = GC.refs(c, True)['bwd_data']
            assert not dx[:, -rows:].any() and not dx[:, :, -cols:].any() and dx[:, :-rows, :-cols].any(), c.id


@pytest.mark.parametrize('case', GC.ALL, **GC.ids(GC.ALL))
def test_references_agree_with_float64_torch(case):
    """max-norm agreement of the tap loops with conv2d + autograd on the explicitly padded input, on the random and on the integer
    inputs; on the integer inputs the adjoint identities <y, dy> == <x, dx> == <w, dw> hold exactly"""
    for integer in (False, True):
        mine, theirs = GC.refs(case, integer), GC.torch_refs(case, integer)
        for e in case.entries:
            assert GC.relerr(mine[e], theirs[e]) <= RTOL, (case.id, e, integer)
    I, R = GC.inputs(case, True), GC.refs(case, True)
    dots = [float((R['fwd'] * I['dy']).sum()), float((R['bwd_data'] * I['x']).sum()), float((R['bwd_filter'] * I['w']).sum())]
    assert dots[0] == dots[1] == dots[2], (case.id, dots)
    if case.opt('deconv'):
        for integer in (False, True):
            I = GC.inputs(case, integer)
            assert I['dy'].shape[1:3] == case.opt('deconv')
            assert np.array_equal(GC.transpose_ref(case, integer), GC.refs(case, integer)['bwd_data'] + I['bi'].astype(np.float64))


@pytest.mark.parametrize('case', GC.ALL, **GC.ids(GC.ALL))
def test_integer_inputs_are_exact_in_float32(case):
    """The exactness condition: the derived bound on every intermediate the kernel can form is below 2^24 in units of the path's grid
    (1 for the direct GEMMs, 1/4 for the Winograd forms; derivation in conv_geom_cases), the references are integers within it, the
    inputs are bf16 numbers, and torch float32 on the CPU reproduces the float64 result bit for bit."""
    I, R = GC.inputs(case, True), GC.refs(case, True)
    for k in ('x', 'w', 'dy', 'b', 'bi', 'base'):
        assert np.array_equal(I[k], np.rint(I[k])) and np.abs(I[k]).max() <= 2 and np.array_equal(GC.rne_bf16(I[k]), I[k]), (case.id, k)
    assert all(np.array_equal(GC.refs(case, True, bf16=True)[e], R[e]) for e in case.entries)
    f32 = GC.torch_refs(case, True, 'float32')
    for e in case.entries:
        assert GC.direct_bound(case, e) < 2 ** 24, (case.id, e)
        for word in (case.algo, case.algo_h or ''):
            if word and word[GC.ENTRIES.index(e)] in '32':
                assert GC.winograd_bound(case, e) < 2 ** 24, (case.id, e)
        assert np.array_equal(R[e], np.rint(R[e])) and np.abs(R[e]).max() + 2 <= GC.direct_bound(case, e), (case.id, e)
        assert f32[e].dtype == np.float32 and np.array_equal(f32[e].astype(np.float64), R[e]), (case.id, e)


@pytest.mark.parametrize('case', GC.ALL, **GC.ids(GC.ALL))
def test_cases_tell_the_indexing_errors_from_the_truth(case):
    """A dropped border tap, exchanged filter axes (KH / KW; Cin / Cout), exchanged H / W, exchanged SH / SW and unmasked stride phases
    each move the integer reference, and the Gaussian reference by at least 100 x the bound the GPU test applies, on every entry point
    the case drives.  Where the corruption is provably the identity (conv_geom_cases.identity) that is asserted instead; where it
    changes a tensor's size it is no quiet error and there is nothing to tell apart."""
    for corrupt in GC.CORRUPTIONS:
        if GC.identity(case, corrupt):
            if corrupt == 'io':
                w = GC.inputs(case)['w']
                assert np.array_equal(GC.exchange_io(w), w), case.id
            elif corrupt == 'phase':
                assert np.array_equal(GC.corrupted(case, corrupt, True)['bwd_data'], GC.refs(case, True)['bwd_data']), case.id
            continue
        if not GC.applies(case, corrupt):
            continue
        entries = ('bwd_data',) if corrupt == 'phase' else case.entries
        for integer in (True, False):
            true, wrong = GC.refs(case, integer), GC.corrupted(case, corrupt, integer)
            for e in entries:
                moved = GC.relerr(wrong[e], true[e])
                assert moved > 0 if integer else moved >= 100 * case.tol(e), (case.id, corrupt, e, integer, moved)


def test_every_corruption_is_seen_by_some_case_of_every_family():
    for fam in ('geom', 'walk', 'wino3', 'wino2', 'census'):
        cases = [c for c in GC.ALL if c.family == fam]
        for corrupt in GC.CORRUPTIONS:
            if corrupt == 'shsw' and fam != 'geom':
                continue            # SH != SW exists in the geometry rows only
            if corrupt == 'phase' and fam in ('walk', 'wino3', 'wino2'):
                continue            # stride 1, or k4 s2 (four phases of four taps each): nothing to mask
            assert any(GC.applies(c, corrupt) for c in cases), (fam, corrupt)
    for tag in GC.PHASE_TAGS:
        if tag != 'k3s3':
            assert all(GC.applies(c, 'phase') for c in GC.GEOMETRY if c.tag == tag), tag
    assert all(GC.applies(c, 'shsw') for c in GC.GEOMETRY if c.tag in ('s2x1', 's1x2'))
    assert all(GC.applies(c, 'khkw') for c in GC.GEOMETRY if c.tag in ('k1x7', 'k7x1', 'k1x3', 'k3x1'))


# ---- census ---------------------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """an ops object for models/inception/model.py _inception_v3 that records every convolution with the map it runs on"""

    def __init__(self, K):
        self.K, self.convs = K, []

    def conv(self, x, name, kh, kw, cout, stride=1, padding='SAME', bn=True):
        B, H, W, cin = x
        self.convs.append((name, (H, W, cin, cout, kh, kw, stride, stride, padding)))
        return (B, self.K.pool_out_size(H, kh, stride, padding), self.K.pool_out_size(W, kw, stride, padding), cout)

    def pool(self, x, name, k, stride, padding, op):
        B, H, W, C = x
        return (B, self.K.pool_out_size(H, k, stride, padding), self.K.pool_out_size(W, k, stride, padding), C)

    pool_into = pool

    def concat(self, parts):
        assert len(set(p[:3] for p in parts)) == 1, parts
        return parts[0][:3] + (sum(p[3] for p in parts),)


def test_census_every_model_geometry_has_a_case(K):
    """The key (KH, KW, stride, padding, H odd, W odd, Cin % 32 == 0, Cout % 32 == 0) of every InceptionV3 layer at a 299 x 299 input,
    and of every GAN layer tests/test_host.py and FULL of tests/test_kernels_gpu.py list, is the key of some case."""
    from t2i_amd.models.inception import model as M
    rec = _Recorder(K)
    M._inception_v3(rec, (1, M.IMAGE_SIZE, M.IMAGE_SIZE, 3), 20)
    table = M.layer_table(20)
    assert [n for n, _ in rec.convs] == list(table) and len(rec.convs) == 95
    for name, g in rec.convs:                                # the recorder and the model's own trace agree
        kh, kw, cin, cout, stride, padding, Ho, Wo, _ = table[name]
        assert g[2:] == (cin, cout, kh, kw, stride, stride, padding), name
    maps = sorted(set(g[0] for _, g in rec.convs))
    assert maps == [1, 8, 17, 35, 73, 147, 149, 299]
    have = set(c.key for c in GC.ALL)
    missing = sorted(set((GC.census_key(g), name) for name, g in rec.convs if GC.census_key(g) not in have))
    assert not missing, missing
    gan = [(H, W, Ci, Co, k, k, s, s, pad) for H, W, Ci, Co, k, s, pad in GC.GAN_LAYERS]
    missing = [g for g in gan if GC.census_key(g) not in have]
    assert not missing, missing


# ---- routing --------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switched(K, switches):
    try:
        for k, v in switches.items():
            K.tuning_set(k, v)
        yield
    finally:
        for k in switches:
            K.tuning_set(k, GC.SWITCH_DEFAULTS[k])


def _desc(K, case, math):
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    mcode = K.MATH_BF16 if math == 'bf16' else K.MATH_F32
    if case.opt('deconv'):
        h, w = case.opt('deconv')
        return K.deconv_desc(B, h, w, Co, Ci, KH, KW, SH, SW, pad, math=mcode)[0]
    return K.conv_desc(B, H, W, Ci, Co, KH, KW, SH, SW, pad, math=mcode)[0]


@pytest.mark.parametrize('case', GC.ALL, **GC.ids(GC.ALL))
def test_cases_reach_the_kernels_they_name(K, case):
    with switched(K, case.switches):
        for math in ('f32', 'bf16') if case.algo_h else ('f32',):
            d = _desc(K, case, math)                  # after the switches: tuning_set drops the cached descriptors
            assert (d.H, d.W, d.Cin, d.Cout) == case.shape[1:5] and (d.Ho, d.Wo, d.pad_t, d.pad_l) == GC.geometry(case), case.id
            for e, algo in case.algos(math).items():
                assert K.conv_algo(d, e) == algo, (case.id, math, e, K.conv_algo(d, e))
    if case.tag in GC.PHASE_TAGS:                     # ... and under the forced tiles of the GPU test, with the direct kernels off
        with switched(K, dict(force_tile=11, force_splitk=3, no_thin=1)):
            for math in ('f32', 'bf16') if case.algo_h else ('f32',):
                d = _desc(K, case, math)
                forced = dict(case.algos(math))
                if math == 'bf16':
                    forced['bwd_filter'] = 'implicit_gemm_bf16_operands' if GC.geometry(case)[1] % 4 == 0 else 'implicit_gemm'
                assert {e: K.conv_algo(d, e) for e in case.entries} == forced, case.id


def test_unsupported_geometry_is_refused(K):
    """validate_desc admits SH != SW and strides up to 4; a stride of 5 is refused (tests/test_conv_geom_gpu.py: by every entry point)"""
    assert K.conv_algo(K.conv_desc(1, 10, 10, 8, 8, 3, 3, 4, 1, 'SAME')[0], 'bwd_data') == 'implicit_gemm'
    for SH, SW in ((5, 1), (1, 5), (5, 5)):
        with pytest.raises(ValueError):
            K.conv_algo(K.conv_desc(1, 10, 10, 8, 8, 3, 3, SH, SW, 'SAME')[0], 'fwd')
    with pytest.raises(ValueError):                          # a VALID kernel larger than the map has no output
        K.conv_desc(1, 2, 2, 8, 8, 3, 3, 1, 1, 'VALID')


def test_routing_pairs_share_their_geometry():
    """a just-eligible and a just-ineligible case of a pair have the same kernel, stride and padding and take different algorithms"""
    for fam, inside, outside in GC.WINO_PAIRS:
        a, b = GC.by_tag(fam, inside), GC.by_tag('k16' if fam == 'k15' else fam, outside)
        assert a.shape[5:] == b.shape[5:] or fam == 'k15', (fam, inside, outside)
        assert (a.algo, a.algo_h) != (b.algo, b.algo_h), (fam, inside, outside)


def test_stated_bounds_rest_on_the_float32_yardstick():
    """A bound a case states for itself is at most min(1e-4, 4 x the error of torch's float32 evaluation on the CPU)."""
    by_id = {c.id: c for c in GC.ALL}
    for cid, stated in GC.STATED.items():
        for check, bound in stated.items():
            entry = next(e for e in GC.ENTRIES if check.startswith(e))
            assert bound <= min(1e-4, 4 * GC.f32_yardstick(by_id[cid], entry)), (cid, check, bound)
