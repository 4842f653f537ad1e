"""The load-size image stores on the GPU: t2i_pillow_tables against evaluation/resize.py's tables, kernels.preprocess_images and
the two commands against the host statement (preprocess/utils.py, which tests/test_preprocess_host.py holds to Pillow) — all by
equality."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import preprocess_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)

MAX_SIDE = 16384                          # T2I_PREPROCESS_MAX_SIDE
PAIRS = [(667, 600), (500, 360), (90, 360), (5, 600), (601, 600), (599, 600), (7, 600), (1000, 600), (1200, 360), (37, 360), (600, 600),
         (1, 5), (1, 1), (2, 3), (4096, 1024), (MAX_SIDE, 600), (MAX_SIDE, 7)]


@pytest.mark.parametrize('filter', ['bicubic', 'bilinear'])
def test_device_tables_equal_the_host_tables(filter):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.evaluation import resize as R
    host = {'bicubic': R.bicubic_tables, 'bilinear': R.bilinear_tables}[filter]
    for out in sorted({o for _, o in PAIRS}):
        ins = [i for i, o in PAIRS if o == out]
        bounds, coeffs = K.pillow_tables(torch.tensor(ins, dtype=torch.int32, device=DEV), out, filter)
        bounds, coeffs = bounds.cpu().numpy(), coeffs.cpu().numpy()
        for n, i in enumerate(ins):
            hb, hk = host(i, out)
            assert np.array_equal(bounds[n], hb), (filter, i, out)
            assert np.array_equal(coeffs[n, :, :hk.shape[1]], hk), (filter, i, out)
            assert not coeffs[n, :, hk.shape[1]:].any(), (filter, i, out)
    # an axis that needs more taps than kmax, or is outside the supported sides, gets empty rows; its neighbours are untouched
    sizes = torch.tensor([600, 1200, 0, MAX_SIDE + 1, 300], dtype=torch.int32, device=DEV)
    kmax = host(600, 600)[1].shape[1]
    bounds, coeffs = (t.cpu().numpy() for t in K.pillow_tables(sizes, 600, filter, kmax=kmax))
    for n in (1, 2, 3):
        assert not bounds[n].any() and not coeffs[n].any()
    for n, i in ((0, 600), (4, 300)):
        assert np.array_equal(bounds[n], host(i, 600)[0]) and np.array_equal(coeffs[n], host(i, 600)[1])


def _mixed_batch():
    """-> (images, boxes): the eight shapes, 1- / 3- / 4-channel storage, crops at every border, constant, full range, a twin."""
    images, boxes = [], []
    for k, (h, w, _) in enumerate(PC.RAGGED):
        images.append(PC.image(k, h, w, (3, 1, 4, 3)[k % 4]))
        boxes.append(None)
    big = PC.image(50, 120, 150, 3)
    for box in ((0, 70, 0, 90), (0, 120, 60, 150), (50, 120, 0, 150), (33, 120, 41, 150), (0, 120, 0, 150), (10, 110, 20, 21), (60, 61, 0, 150)):
        images.append(big)                                                        # (each stored again: a crop is an offset into ITS copy)
        boxes.append(box)
    images.append(PC.image(51, 64, 80, 4)); boxes.append((5, 60, 7, 77))         # a crop of 4-channel storage
    images.append(PC.image(52, 64, 80, 1)); boxes.append((0, 64, 40, 80))        # a crop of grey storage
    images.append(np.full((40, 50, 3), 93, np.uint8)); boxes.append(None)        # constant: black
    images.append(PC.image(53, 45, 55, 3, lo=0, hi=255)); boxes.append(None)     # already 0 .. 255: the table is the identity
    twin = PC.image(54, 70, 90, 3)
    images.insert(2, twin); boxes.insert(2, None)
    images.append(twin.copy()); boxes.append(None)                                # the same content at another offset
    return images, boxes


def test_preprocess_images_equals_the_host_statement_on_a_mixed_batch():
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    images, boxes = _mixed_batch()
    S = 360
    packed, rows = PC.pack(images, boxes)
    dp = torch.from_numpy(packed).to(DEV)
    got = K.preprocess_images(dp, rows, S)
    again = K.preprocess_images(dp, rows, S)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(images), S, S, 3)
    assert torch.equal(got, again)                                                 # bitwise repeatable
    got = got.cpu().numpy()
    want = PC.host_statement(packed, rows, S)
    for n in range(len(images)):
        assert np.array_equal(got[n], want[n]), (n, rows[n])
    assert np.array_equal(got[2], got[-1]) and got[2].any()                       # the twins
    assert not got[-3].any()                                                       # the constant image
    # an image alone (a batch of one, its own workspace layout) gives the same bytes, at the size RAGGED lists it with
    for n in (0, 1):
        p1, r1 = PC.pack([images[n]], None)
        s = PC.RAGGED[n][2]
        y1 = K.preprocess_images(torch.from_numpy(p1).to(DEV), r1, s).cpu().numpy()
        assert np.array_equal(y1, PC.host_statement(p1, r1, s)), PC.RAGGED[n]


@pytest.mark.parametrize('case', [c for c in PC.RAGGED if c[2] == 600], ids=lambda c: '%dx%d-%d' % c)
def test_preprocess_images_at_600(case):
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    h, w, S = case
    packed, rows = PC.pack([PC.image(h + w, h, w, 3)], None)
    got = K.preprocess_images(torch.from_numpy(packed).to(DEV), rows, S).cpu().numpy()
    assert np.array_equal(got, PC.host_statement(packed, rows, S))


def test_many_tiny_images_and_one_tall_one():
    """More images than a grid's y / z extent holds (65 535), the last ones distinct; a tall image among them costs the others nothing."""
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib, kernels as K
    n_fill, S = 65535, 2
    tail = [PC.image(60 + k, 2 + k % 3 * 3, 5 + k, 3) for k in range(9)] + [PC.image(70, 40, 2, 1)]
    filler = np.array([[[9, 9, 9]]], np.uint8)                                     # 1 x 1: constant, so black
    packed_t, rows_t = PC.pack(tail, None)
    packed = np.concatenate([np.tile(filler.reshape(-1), n_fill), packed_t])
    rows = [(3 * i, 1, 1, 3, 0, 1, 0, 1) for i in range(n_fill)] + [(o + 3 * n_fill,) + tuple(r) for (o, *r) in rows_t]
    total_rows = n_fill + sum(t.shape[0] for t in tail)
    # the intermediate follows the batch's rows (S * 3 bytes each), not N x the tallest image
    q = _lib.lib.t2i_preprocess_images_workspace_bytes
    assert q(len(rows), total_rows, 40, S) - q(len(rows), total_rows - 256, 40, S) == 256 * S * 3
    got = K.preprocess_images(torch.from_numpy(packed).to(DEV), rows, S).cpu().numpy()
    assert got.shape == (n_fill + len(tail), S, S, 3) and not got[:n_fill].any()
    assert np.array_equal(got[n_fill:], PC.host_statement(packed_t, rows_t, S)) and got[n_fill:].any()


def test_bad_arguments_are_refused_on_the_device_too():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib, kernels as K
    packed, rows = PC.pack([PC.image(1, 20, 30, 3)], None)
    dp = torch.from_numpy(packed).to(DEV)
    for bad in ([(0, 20, 30, 2, 0, 20, 0, 30)], [(0, 20, 30, 3, 0, 21, 0, 30)], [(1, 20, 30, 3, 0, 20, 0, 30)], [(0, 20, 30, 3, 5, 5, 0, 30)]):
        with pytest.raises(_lib.T2IError, match='t2i_preprocess_images'):
            K.preprocess_images(dp, bad, 8)
    assert np.array_equal(K.preprocess_images(dp, rows, 8).cpu().numpy(), PC.host_statement(packed, rows, 8))


# ---- the commands, device path ----------------------------------------------------------------------------------------------------
def _load(path):
    import joblib
    return np.asarray(joblib.load(path))


def test_flowers_command_end_to_end_with_a_chunk_boundary(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.resize import resize_u8_bicubic
    from t2i_amd.preprocess import image_store as IS, preprocess_flowers as PF
    # two images of about 1 MB each: --chunk-mb 1 splits the train split into several kernel calls
    root = PC.flowers_tree(str(tmp_path / 'flowers'), [(500, 667, 3), (40, 60, 3), (64, 48, 1), (520, 700, 3), (57, 31, 3), (90, 120, 3)],
                           [(48, 48, 3), (25, 70, 1)])
    paths = PF.image_paths(root, PF.load_filenames(os.path.join(root, 'train')))
    _, stats = IS.build_store(paths, None, 96, DEV, chunk_bytes=1 << 20, workers=4)
    assert stats['chunks'] >= 3
    written = PF.main(['--dir', root, '--load-size', '96', '--stage-sizes', '4', '76', '--chunk-mb', '1', '--workers', '4'])
    assert len(written) == 6
    for split in ('train', 'test'):
        store = _load(IS.store_path(root, split, 96))
        assert np.array_equal(store, PC.expected_flowers(root, split, 96))
        for s in (4, 76):
            assert np.array_equal(_load(IS.store_path(root, split, s)), np.stack([resize_u8_bicubic(im, s, s) for im in store]))


def test_birds_command_end_to_end(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.evaluation.resize import resize_u8_bicubic
    from t2i_amd.preprocess import image_store as IS, preprocess_birds as PB
    root = PC.birds_tree(str(tmp_path / 'birds'),
                         [(60, 80, 3, '12.0 5.0 40.0 30.0'), (50, 50, 3, '0.0 0.0 50.0 50.0'), (45, 70, 1, '30.0 10.0 39.0 33.0'),
                          (80, 40, 3, '5.0 50.0 20.0 28.0'), (375, 500, 3, '60.0 27.0 325.0 304.0')],
                         [(64, 64, 3, '20.0 20.0 10.0 10.0'), (30, 90, 3, '60.0 2.0 29.0 27.0')])
    written = PB.main(['--dir', root, '--load-size', '96', '--stage-sizes', '4', '76'])
    assert len(written) == 6
    for split in ('train', 'test'):
        store = _load(IS.store_path(root, split, 96))
        assert np.array_equal(store, PC.expected_birds(root, split, 96))
        for s in (4, 76):
            assert np.array_equal(_load(IS.store_path(root, split, s)), np.stack([resize_u8_bicubic(im, s, s) for im in store]))
