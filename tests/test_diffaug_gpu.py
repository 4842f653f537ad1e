"""The differentiable augmentation on the GPU (csrc/t2i_augment.hip) against its float64 restatement
(tests/diffaug_cases.py, differentiated by autograd): second-order parity on the gradient-penalty chain, the exactness cases, the adjoint
identity, independence of the batch and repeatability bit for bit, and the refusals, none of which launches.

Bounds (tests/test_norm_second_order_gpu.py's): forward <= 1e-5, first- and second-order gradients <= 1e-4, max-norm relative."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import diffaug_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = dict(ids=lambda s: 'x'.join(str(v) for v in s) if isinstance(s, tuple) else s.replace(',', '+'))
FWD_TOL, GRAD_TOL = 1e-5, 1e-4


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import ops
    return ops


@pytest.fixture(scope='module')
def K(ops):
    from t2i_amd import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def _reference(shape, policy):
    """(y, gx, d loss / dx, d loss / dw) of the float64 restatement: computed once per case and never written to"""
    x, w = DC.inputs(shape)
    P = DC.table(shape, torch.float64)
    return DC.second_order(lambda t: DC.ref_T(t, P, policy), x.double(), w.double())


@pytest.mark.parametrize('policy', DC.POLICIES, **IDS)
@pytest.mark.parametrize('shape', DC.SHAPES, **IDS)
def test_second_order_parity_with_float64(ops, shape, policy):
    x, w = DC.inputs(shape)
    P = DC.table(shape).cuda()
    got = DC.second_order(lambda t: ops.diff_augment(t, P, policy), x.cuda(), w.cuda())
    torch.cuda.synchronize()
    errs = [DC.relerr(g, r) for g, r in zip(got, _reference(shape, policy))]
    print('diff_augment %s %s: y %.2e  gx %.2e  d/dx %.2e  d/dw %.2e' % ((shape, policy) + tuple(errs)))
    assert float(got[1].abs().max()) > 0 and float(got[2].abs().max()) > 0
    assert errs[0] <= FWD_TOL and max(errs[1:]) <= GRAD_TOL, errs


def test_a_sample_of_64x64_has_more_than_one_partial(K):
    from t2i_amd import _lib
    ws = _lib.lib.t2i_diff_augment_workspace_bytes
    assert int(ws(2, 64, 64, 3, K.DIFFAUG_COLOR)) // (2 * 4) > 1
    assert int(ws(1, 256, 256, 3, K.DIFFAUG_COLOR)) // 4 > 1 and int(ws(2, 4, 4, 3, K.DIFFAUG_COLOR)) // (2 * 4) == 1


@pytest.mark.parametrize('shape', [(2, 4, 4, 3), (3, 5, 7, 3), (2, 8, 8, 4), (2, 64, 64, 3), (2, 6, 5, 5)], **IDS)
def test_identity_rows_return_the_input_bit_for_bit(ops, K, shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    P = DC.identity_table(shape[0]).cuda()
    for policy in DC.POLICIES:
        assert torch.equal(ops.diff_augment(x, P, policy), x), policy
        mask = ops.diff_augment_policy(policy)
        assert torch.equal(K.diff_augment_fwd(x, P, mask, offset=False), x), policy
        assert torch.equal(K.diff_augment_adj(x, P, mask), x), policy


@pytest.mark.parametrize('shape', [(3, 5, 7, 3), (2, 8, 8, 4), (2, 64, 64, 3), (2, 6, 5, 5)], **IDS)
def test_exact_values_of_the_colour_transform(ops, shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(2)).cuda()
    B = shape[0]
    P = DC.identity_table(B)
    P[:, 0] = torch.linspace(-0.4, 0.3, B)
    # s = 0: every pixel's channels are equal (its channel mean, then one contrast blend for all of them)
    Ps = P.clone()
    Ps[:, 1], Ps[:, 2] = 0.0, 1.3
    y = ops.diff_augment(x, Ps.cuda(), 'color')
    assert torch.equal(y, y[..., :1].expand_as(y)) and float(y.std()) > 0
    # c = 0: a constant image, the sample's mean plus b
    Pc = P.clone()
    Pc[:, 1], Pc[:, 2] = 0.7, 0.0
    y = ops.diff_augment(x, Pc.cuda(), 'color')
    want = x.double().mean((1, 2, 3)).cpu() + P[:, 0].double()
    assert torch.equal(y, y[:, :1, :1, :1].expand_as(y))
    err = float((y[:, 0, 0, 0].double().cpu() - want).abs().max())
    print('c = 0 at %s: |constant - (float64 mean + b)| = %.2e' % (shape, err))
    assert err <= 1e-5


@pytest.mark.parametrize('shape', [(2, 4, 4, 3), (3, 5, 7, 3), (2, 8, 8, 4), (2, 64, 64, 3)], **IDS)
def test_a_rectangle_over_the_whole_image_gives_exact_zeros(ops, K, shape):
    B, H, W, _ = shape
    x = DC.inputs(shape)[0].cuda()
    P = DC.table(shape)
    P[:, 5], P[:, 6], P[:, 7], P[:, 8] = 0, H, 0, W
    P = P.cuda()
    for policy in ('cutout', DC.ALL):
        mask = ops.diff_augment_policy(policy)
        assert not bool(ops.diff_augment(x, P, policy).any()), policy
        assert not bool(K.diff_augment_adj(x, P, mask).any()), policy


@pytest.mark.parametrize('policy', DC.POLICIES, **IDS)
@pytest.mark.parametrize('shape', DC.SHAPES, **IDS)
def test_the_adjoint_identity(K, ops, shape, policy):
    """<A u, g> = <u, A^T g> with A = the forward without the offset, both sides summed in float64.  u and g are positive (U(0.5, 1.5)),
    so neither inner product is a small difference of large terms and 1e-5 of its value is a bound on the kernels' own rounding."""
    gen = torch.Generator().manual_seed(11 + sum(shape))
    u = (torch.rand(shape, generator=gen) + 0.5).cuda()
    g = (torch.rand(shape, generator=gen) + 0.5).cuda()
    P = DC.table(shape).cuda()
    mask = ops.diff_augment_policy(policy)
    lhs = float((K.diff_augment_fwd(u, P, mask, offset=False).double() * g.double()).sum())
    rhs = float((u.double() * K.diff_augment_adj(g, P, mask).double()).sum())
    print('adjoint identity %s %s: %.12g against %.12g' % (shape, policy, lhs, rhs))
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


@pytest.mark.parametrize('shape', [(3, 5, 7, 3), (2, 8, 8, 4), (2, 64, 64, 3)], **IDS)
def test_a_sample_does_not_depend_on_its_batch_and_calls_repeat(ops, shape):
    """cat of three batches with cat of their tables = the three calls, bit for bit, for y, gx and the second-order gradients (the
    odd sample size 5 * 7 * 3 also puts the second and third batch at addresses that are not 16-byte aligned); and a repeated call
    is bit-equal"""
    P = DC.table(shape)
    parts = []
    for k in range(3):
        x, w = DC.inputs(shape, seed=k)
        parts.append((x.cuda(), w.cuda(), P.roll(k, 0).contiguous().cuda()))
    one = [DC.second_order(lambda t, Pk=Pk: ops.diff_augment(t, Pk, DC.ALL), x, w) for x, w, Pk in parts]
    X, Wt, Pc = (torch.cat([p[i] for p in parts], 0) for i in range(3))
    whole = DC.second_order(lambda t: ops.diff_augment(t, Pc, DC.ALL), X, Wt)
    again = DC.second_order(lambda t: ops.diff_augment(t, Pc, DC.ALL), X, Wt)
    for i, name in enumerate(('y', 'gx', 'd/dx', 'd/dw')):
        assert torch.equal(whole[i], torch.cat([o[i] for o in one], 0)), name
        assert torch.equal(whole[i], again[i]), name


def test_refusals_on_device_tensors_launch_nothing(ops, K, monkeypatch):
    calls = []
    real = K.diff_augment_fwd
    monkeypatch.setattr(K, 'diff_augment_fwd', lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    from t2i_amd import stacked as ST
    x, P = torch.zeros(2, 4, 4, 3, device='cuda'), DC.identity_table(2).cuda()
    bad_calls = [
        (ValueError, lambda: ops.diff_augment(x.bfloat16(), P)),
        (NotImplementedError, lambda: ops.diff_augment(ST.Stacked(x, x.clone()), P)),
        (ValueError, lambda: ops.diff_augment(x[0], P)),
        (ValueError, lambda: ops.diff_augment(torch.zeros(2, 3, 4, 4, device='cuda').permute(0, 2, 3, 1), P)),
        (ValueError, lambda: ops.diff_augment(x, P, 'color,flip')),
        (ValueError, lambda: ops.diff_augment(x, P, '')),
        (ValueError, lambda: ops.diff_augment(x, DC.identity_table(3).cuda())),
        (ValueError, lambda: ops.diff_augment(x, P[:, :8])),
        (ValueError, lambda: ops.diff_augment(x, P.double())),
        (ValueError, lambda: ops.diff_augment(x, P.cpu())),
        (ValueError, lambda: ops.diff_augment(x, torch.zeros(9, 2, device='cuda').t())),
    ]
    for exc, call in bad_calls:
        with pytest.raises(exc, match='diff_augment'):
            call()
    assert calls == []
    assert torch.equal(ops.diff_augment(x, P), x) and calls == [1]          # the wrapper does count an accepted call
