"""kernels.nearest_images (t2i_nearest_images) against a float64 NumPy brute force over the same uint8 store and crop tables.
The brute force normalises with the kernel's own fp32 arithmetic (u8 * fl32(2/255) - 1 without fused multiply-add, the value
crop_flip_normalize is pinned to), then takes the squared distance in float64 and the lowest index of the minimum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _real(u8):
    return (u8.astype(np.float32) * np.float32(2. / 255) - np.float32(1.)).astype(np.float64)


def _crops_of(src, n, row0, col0, flip, out):
    """src[n] cropped at (row0[k], col0[k]) and flipped where flip[k], for the index arrays n / row0 / col0 / flip."""
    rows = row0[:, None] + np.arange(out)[None, :]
    cols = np.where(flip[:, None] != 0, col0[:, None] + out - 1 - np.arange(out)[None, :], col0[:, None] + np.arange(out)[None, :])
    return src[n[:, None, None], rows[:, :, None], cols[:, None, :], :]


def _brute(src, queries, tables, lo=-1.0, hi=1.0):
    """-> (idx [Q], sorted distances [Q, N]) in float64."""
    N, S = src.shape[0], src.shape[1]
    Q, out = queries.shape[0], queries.shape[1]
    fake = np.minimum(np.maximum(queries, np.float32(lo)), np.float32(hi)).astype(np.float64)
    idx, srt = np.zeros(Q, np.int64), np.zeros((Q, N))
    for q in range(Q):
        if tables is None:
            real = _real(src)
        else:
            real = _real(_crops_of(src, np.arange(N), tables[0][q], tables[1][q], tables[2][q], out))
        d2 = ((fake[q][None] - real) ** 2).sum(axis=(1, 2, 3))
        idx[q] = int(np.argmin(d2))                     # np.argmin: first occurrence of the minimum
        srt[q] = np.sort(d2)
    return idx, srt


def _case(N, S, out, Q, seed, tables=True):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (N, S, S, 3), dtype=np.uint8)
    queries = rng.uniform(-1.05, 1.05, (Q, out, out, 3)).astype(np.float32)
    tabs = None
    if tables:
        tabs = (rng.integers(0, S - out + 1, (Q, N)).astype(np.int32), rng.integers(0, S - out + 1, (Q, N)).astype(np.int32),
                rng.integers(0, 2, (Q, N)).astype(np.int32))
    return src, queries, tabs


def _run(src, queries, tabs, **kw):
    from t2i_amd import kernels as K
    dev = torch.device('cuda')
    t = [torch.from_numpy(a).to(dev) for a in tabs] if tabs is not None else [None] * 3
    idx, d2 = K.nearest_images(torch.from_numpy(src).to(dev), torch.from_numpy(queries).to(dev), *t, **kw)
    return idx.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize('N,S,out,Q,tables', [(1, 64, 64, 1, False), (37, 76, 64, 8, True), (300, 76, 64, 64, True),
                                              (1025, 76, 64, 3, True)])
def test_nearest_matches_float64_brute_force(N, S, out, Q, tables):
    import t2i_amd  # noqa: F401
    src, queries, tabs = _case(N, S, out, Q, seed=N + Q, tables=tables)
    want, srt = _brute(src, queries, tabs)
    if N > 1:      # well posed: best and second best apart by more than the tolerance
        assert np.all((srt[:, 1] - srt[:, 0]) > 1e-9 * srt[:, 0])
    idx, d2 = _run(src, queries, tabs)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_allclose(d2, srt[:, 0], rtol=1e-12, atol=0)


def test_nearest_ties_take_the_lowest_index():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    src, _, tabs = _case(24, 76, 64, 2, seed=7)
    k = 11
    for j in (k - 3, k + 5):
        src[j] = src[k]
        for t in tabs:
            t[:, j] = t[:, k]
    dev = torch.device('cuda')
    t = [torch.from_numpy(a).to(dev) for a in tabs]
    ids = torch.full((2,), k, dtype=torch.int32, device=dev)
    # each query: its own crop of image k, slightly perturbed, so the three copies are the three nearest and tie exactly
    crops = torch.stack([K.crop_flip_normalize(torch.from_numpy(src).to(dev), ids[q:q + 1], t[0][q, k:k + 1], t[1][q, k:k + 1],
                                               t[2][q, k:k + 1], 64)[0] for q in range(2)])
    queries = (crops.cpu().numpy() + np.random.default_rng(1).uniform(-0.01, 0.01, crops.shape)).astype(np.float32)
    idx, d2 = _run(src, queries, tabs)
    want, srt = _brute(src, queries, tabs)
    assert list(idx) == [k - 3, k - 3] and list(want) == [k - 3, k - 3]
    assert np.all(srt[:, 0] == srt[:, 2]) and np.all(srt[:, 3] > srt[:, 0])
    np.testing.assert_allclose(d2, srt[:, 0], rtol=1e-12, atol=0)


def test_nearest_exact_zero_for_a_stored_crop():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    src, _, tabs = _case(50, 76, 64, 3, seed=11)
    dev = torch.device('cuda')
    t = [torch.from_numpy(a).to(dev) for a in tabs]
    js = [4, 0, 49]
    queries = torch.stack([K.crop_flip_normalize(torch.from_numpy(src).to(dev), torch.tensor([j], dtype=torch.int32, device=dev),
                                                 t[0][q, j:j + 1], t[1][q, j:j + 1], t[2][q, j:j + 1], 64)[0] for q, j in enumerate(js)])
    idx, d2 = _run(src, queries.cpu().numpy(), tabs)
    assert list(idx) == js
    assert np.all(d2 == 0.0)


def test_nearest_clips_the_queries():
    import t2i_amd  # noqa: F401
    src, queries, tabs = _case(64, 76, 64, 4, seed=13)
    big = queries * np.float32(3.0)
    want, srt = _brute(src, np.clip(big, -1.0, 1.0), tabs)
    idx, d2 = _run(src, big, tabs)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_allclose(d2, srt[:, 0], rtol=1e-12, atol=0)
    # other bounds go through as given
    want2, srt2 = _brute(src, big, tabs, lo=-0.5, hi=0.75)
    idx2, d22 = _run(src, big, tabs, lo=-0.5, hi=0.75)
    np.testing.assert_array_equal(idx2, want2)
    np.testing.assert_allclose(d22, srt2[:, 0], rtol=1e-12, atol=0)


def test_nearest_is_deterministic():
    import t2i_amd  # noqa: F401
    src, queries, tabs = _case(300, 76, 64, 64, seed=17)
    a = _run(src, queries, tabs)
    b = _run(src, queries, tabs)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes()
