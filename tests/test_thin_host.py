"""The cases of tests/thin_cases.py without a GPU: their float64 references against float64 torch convolutions (so that
tests/test_thin_gpu.py does not rest on one implementation), their sensitivity to the three indexing errors they are there to catch,
and the routing of every case (and of the models' own edge layers) through t2i_conv2d_algo, which is host logic."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import thin_cases as TC  # noqa: E402

RTOL = 1e-12
LDS_PER_CU = 160 * 1024


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
    seen = [c.id for c in TC.ALL]
    assert len(set(seen)) == len(seen), sorted(i for i in seen if seen.count(i) > 1)
    assert len(TC.THIN) == 11 and len(TC.TINY) == 6 and len(TC.TINY_BWDW) == 5 and len(TC.HEAD) == 5 and len(TC.STEM) == 8 and len(TC.PAIR) == 3
    for c in TC.ALL:
        assert set(c.direct) <= set(c.entries) <= set(TC.ENTRIES), c.id


@pytest.mark.parametrize('case', TC.ALL, **TC.ids(TC.ALL))
def test_references_agree_with_float64_torch(case):
    """max-norm agreement of the tap loops with conv2d + autograd on the explicitly padded input, on the random and on the integer inputs"""
    for integer in (False, True):
        mine, theirs = TC.refs(case, integer), TC.torch_refs(case, integer)
        for e in case.entries:
            assert TC.relerr(mine[e], theirs[e]) <= RTOL, (case.id, e, integer)
            if integer:
                assert np.array_equal(mine[e], np.rint(mine[e])) and np.abs(mine[e]).max() < 2 ** 24, (case.id, e)


@pytest.mark.parametrize('case', TC.ALL, **TC.ids(TC.ALL))
def test_cases_tell_the_indexing_errors_from_the_truth(case):
    """A dropped border tap, exchanged filter axes and exchanged H / W each move the reference by at least 100 x the bound the GPU test
    applies, on every entry point the case drives.  Exchanged filter axes do not exist where Cin or Cout is 1 (the two orders address
    the same memory), exchanged H / W not where H == W: there the corruption is checked to be the identity instead."""
    true = TC.refs(case)
    for corrupt in TC.CORRUPTIONS:
        if not TC.applies(case, corrupt):
            if corrupt == 'io':
                w = TC.inputs(case)['w']
                assert np.array_equal(TC.exchange_io(w), w), case.id
            continue
        wrong = TC.corrupted(case, corrupt)
        for e in case.entries:
            moved = TC.relerr(wrong[e], true[e])
            assert moved >= 100 * case.tol(e), (case.id, corrupt, e, moved)


def test_every_corruption_is_seen_by_some_case_of_every_family():
    for fam in ('thin', 'tiny', 'bwdw', 'head', 'stem'):
        cases = [c for c in TC.ALL if c.family == fam]
        for corrupt in TC.CORRUPTIONS:
            if fam == 'head' and corrupt == 'hw':
                continue            # the head reduces a square map to one pixel: H and W meet only in the product K = H W Cin
            assert any(TC.applies(c, corrupt) for c in cases), (fam, corrupt)


# ---- routing --------------------------------------------------------------------------------------------------------------------------
def _desc(K, shape):
    B, H, W, Ci, Co, KH, KW, s, pad = shape
    return K.conv_desc(B, H, W, Ci, Co, KH, KW, s, s, pad)[0]


@pytest.mark.parametrize('case', TC.ALL, **TC.ids(TC.ALL))
def test_cases_reach_the_kernels_they_name(K, case):
    parts = case.opt('thin_parts')
    try:
        if parts is not None:
            K.tuning_set('thin_parts', parts)
        d = _desc(K, case.shape)                     # after the switch: tuning_set drops the cached descriptors
        for e in case.entries:
            algo = K.conv_algo(d, e)
            assert (algo == 'direct_small') == (e in case.direct), (case.id, e, algo)
    finally:
        if parts is not None:
            K.tuning_set('thin_parts', 2)


@pytest.mark.parametrize('shape,entries', TC.MODEL_SHAPES)
def test_model_edge_layers_stay_on_the_direct_kernels(K, shape, entries):
    d = _desc(K, shape)
    for e in entries:
        assert K.conv_algo(d, e) == 'direct_small', (shape, e)


def _lds(Cin, CH):
    return (100 * (CH + 4) + 16 * Cin * CH) * 4


def _passes(Cin, Cout, start):
    """the rule of thin_deconv_passes (csrc/t2i_thin.hip), restated: halve the tuning value until the split is legal, double it while
    the patch does not fit a CU and the doubled split is legal; 0 where that ends over the limit"""
    legal = lambda p: p == 1 or (Cout % (4 * p) == 0 and Cout // p >= 32)
    p = max(start, 1)
    while not legal(p):
        p >>= 1
    while _lds(Cin, Cout // p) > LDS_PER_CU:
        if not legal(2 * p):
            return 0
        p *= 2
    return p


def test_thin_deconv_eligibility_follows_the_lds_arithmetic(K):
    """Every (Cin, Cout, thin_parts) the descriptor admits: direct exactly where a legal split fits the 160 KiB of a CU; the models'
    widths keep the passes they had; per Cin, the first Cout = 4 (mod 8) over the limit (356, 308, 276, 252)."""
    assert _lds(4, 256) == 169536 and _lds(3, 256) == 153152 and _lds(3, 508) == 302336
    assert [_passes(3, 64, 2), _passes(3, 128, 2), _passes(4, 64, 2), _passes(3, 64, 1), _passes(4, 128, 4)] == [2, 2, 2, 1, 4]
    assert _passes(4, 512, 2) == 4 and _passes(3, 512, 2) == 2 and _passes(3, 512, 1) == 2 and _passes(4, 512, 1) == 4
    for Cin, Cout, direct in TC.THIN_LDS_EDGES:
        assert (_passes(Cin, Cout, 2) > 0) == direct, (Cin, Cout)
    over = {Cin: min(Co for Co in range(20, 513, 8) if _passes(Cin, Co, 2) == 0) for Cin in (1, 2, 3, 4)}
    assert over == {1: 356, 2: 308, 3: 276, 4: 252}
    assert sorted(Co for Co in range(16, 513, 8) if _passes(4, Co, 2) == 0) == [504]        # multiples of 8 that cannot be split again
    for parts in (1, 2, 4):
        try:
            K.tuning_set('thin_parts', parts)
            for Cin in (1, 2, 3, 4):
                for Cout in range(16, 513, 4):
                    algo = K.conv_algo(_desc(K, TC._k4s2(1, 16, 16, Cin, Cout)), 'bwd_data')
                    want = _passes(Cin, Cout, parts) > 0
                    assert (algo == 'direct_small') == want, (parts, Cin, Cout, algo)
        finally:
            K.tuning_set('thin_parts', 2)


def test_stated_bounds_rest_on_the_float32_yardstick():
    """A bound a case states for itself is at most min(1e-4, 4 x the error of torch's float32 evaluation on the CPU)."""
    by_id = {c.id: c for c in TC.ALL}
    for cid, stated in TC.STATED.items():
        for check, bound in stated.items():
            entry = next(e for e in TC.ENTRIES if check.startswith(e))
            assert bound <= min(1e-4, 4 * TC.f32_yardstick(by_id[cid], entry)), (cid, check, bound)
