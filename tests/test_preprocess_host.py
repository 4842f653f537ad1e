"""The load-size image stores, host side: preprocess/utils.py (the host statement of the reference's get_image) against Pillow
itself, crop_box known answers, the C ABI's argument checks without a GPU, and the two commands' plumbing with the device call
replaced by the host statement."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import preprocess_cases as PC  # noqa: E402


def _pillow(img, S):
    return np.array(Image.fromarray(PC.scipy_bytescale(img)).resize((S, S), Image.BICUBIC))


# ---- the host statement against Pillow --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', PC.RAGGED, ids=lambda c: '%dx%d-%d' % c)
def test_transform_matches_pillow(case):
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess import utils as U
    h, w, S = case
    img = PC.image(h * 31 + w, h, w)
    assert img.min() > 0 and img.max() < 255                      # the stretch matters
    got = U.transform(img.astype(np.float64), S, False, None)
    assert got.dtype == np.uint8 and got.shape == (S, S, 3)
    assert np.array_equal(got, _pillow(img.astype(np.float64), S))
    assert not np.array_equal(got, np.array(Image.fromarray(img).resize((S, S), Image.BICUBIC)))   # (and is not a plain resize)


def test_grey_rgba_constant_and_full_range():
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess import utils as U
    grey = PC.image(3, 41, 57, 1)
    rgb = np.stack([grey] * 3, axis=2)
    assert np.array_equal(U.colorize(grey), rgb)
    assert np.array_equal(U.transform(grey, 64, False, None), _pillow(rgb, 64))
    rgba = PC.image(4, 30, 44, 4)
    rgba[:, :, 3] = np.where(rgba[:, :, 3] > 100, 0, 255)        # an alpha channel with a wider range than the colours: never read
    assert np.array_equal(U.colorize(rgba), rgba[:, :, :3])
    assert np.array_equal(U.transform(rgba, 50, False, None), _pillow(rgba[:, :, :3], 50))
    const = np.full((20, 30, 3), 77, np.uint8)
    assert not U.transform(const, 16, False, None).any()          # cscale = 1: (v - cmin) * 255 = 0 everywhere
    full = PC.image(5, 25, 35, lo=0, hi=255)
    assert np.array_equal(U.transform(full, 40, False, None), np.array(Image.fromarray(full).resize((40, 40), Image.BICUBIC)))
    with pytest.raises(ValueError, match='0 .. 255'):
        U.transform(np.full((10, 10, 3), 0.5), 8, False, None)


@pytest.mark.parametrize('cmin,cmax', [(0, 255), (37, 201), (77, 77), (0, 0), (255, 255), (0, 1), (3, 250), (100, 101), (1, 254)])
def test_bytescale_lut_is_the_float64_formula(cmin, cmax):
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess.utils import bytescale_lut
    lut = bytescale_lut(cmin, cmax)
    assert lut.dtype == np.uint8 and lut.shape == (256,)
    vals = np.arange(cmin, cmax + 1, dtype=np.float64)
    assert np.array_equal(lut[cmin:cmax + 1], PC.scipy_bytescale(vals))
    if cmin == cmax:
        assert lut[cmin] == 0


def test_crop_box_known_answers():
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess import utils as U
    # inside: centre (222, 179), R = int(325 * 0.75) = 243 -> rows 0:422 of 500 (top cut), columns 0:465 of 500 (left cut)
    assert U.crop_box((500, 500, 3), [60, 27, 325, 304]) == (0, 422, 0, 465)
    assert U.crop_box((500, 500, 3), [60.0, 27.0, 325.0, 304.0]) == (0, 422, 0, 465)       # CUB writes floats
    # well inside a big image: centre (500, 400), R = 75
    assert U.crop_box((1000, 1000), [450, 350, 100, 100]) == (325, 475, 425, 575)
    # leaves on the right and at the bottom: centre (90, 95), R = int(40 * 0.75) = 30, image 100 x 100
    assert U.crop_box((100, 100, 3), [70, 80, 40, 30]) == (65, 100, 60, 100)
    # leaves on all four sides: R = 150 around (50, 100)
    assert U.crop_box((100, 100, 3), [0, 0, 100, 200]) == (0, 100, 0, 100)
    # odd 2 * x + w: (2 * 10 + 7) / 2 = 13.5 -> 13; (2 * 20 + 5) / 2 = 22.5 -> 22; R = int(5.25) = 5
    assert U.crop_box((100, 100, 3), [10, 20, 7, 5]) == (17, 27, 8, 18)
    img = np.arange(100 * 100 * 3).reshape(100, 100, 3)
    assert np.array_equal(U.custom_crop(img, [10, 20, 7, 5]), img[17:27, 8:18])
    # refused, by name
    with pytest.raises(ValueError, match='bird.jpg.*empty'):
        U.check_crop((100, 100), U.crop_box((100, 100), [300, 300, 20, 20]), 'bird.jpg')
    with pytest.raises(ValueError, match='empty'):
        U.transform(np.zeros((100, 100, 3)), 16, True, [300, 300, 20, 20])
    for shape in ((3, 20, 3), (20, 4, 3), (4, 4, 3)):
        with pytest.raises(ValueError, match='3 or 4 pixels'):
            U.transform(np.zeros(shape), 16, False, None, name='x.jpg')
    with pytest.raises(ValueError, match='3 or 4 pixels'):
        U.transform(np.zeros((50, 50, 3)), 16, True, [10, 10, 3, 2])          # centre (11, 11), R = int(2.25) = 2 -> 4 x 4


def test_load_bbox_reads_cub_floats(tmp_path):
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess import preprocess_birds as PB
    d = tmp_path / 'CUB_200_2011'
    d.mkdir()
    (d / 'images.txt').write_text('1 001.A/A_0001.jpg\n2 002.B/B_0002.jpg\n')
    (d / 'bounding_boxes.txt').write_text('1 60.0 27.0 325.0 304.0\n2 139.0 30.0 153.0 264.0\n')
    assert PB.load_bbox(str(tmp_path)) == {'001.A/A_0001': [60, 27, 325, 304], '002.B/B_0002': [139, 30, 153, 264]}
    (d / 'bounding_boxes.txt').write_text('1 60.0 27.0 325.0 304.0\n')
    with pytest.raises(ValueError, match='lines'):
        PB.load_bbox(str(tmp_path))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_bad_arguments_without_a_gpu():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib, kernels
    L = _lib.lib
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    assert L.t2i_version() == 13 and _lib.ABI_VERSION == 13
    for name in ('t2i_pillow_tables', 't2i_preprocess_images', 't2i_preprocess_images_workspace_bytes'):
        assert name in _lib.SIGNATURES and re.search(r'\b%s\s*\(' % name, header) and hasattr(L, name), name
    assert callable(kernels.preprocess_images) and callable(kernels.pillow_tables)
    assert ctypes.sizeof(_lib.ImageDesc) == 40
    max_side = int(re.search(r'#define\s+T2I_PREPROCESS_MAX_SIDE\s+(\d+)', header).group(1))
    max_out = int(re.search(r'#define\s+T2I_PREPROCESS_MAX_OUT\s+(\d+)', header).group(1))
    assert max_side >= 4096 and max_out >= 1024

    q = L.t2i_preprocess_images_workspace_bytes                     # (N, sum of crop heights, largest crop side, S)
    assert q(2, 58, 40, 16) > 58 * 16 * 3 and q(2, 58, 40, 16) % 256 == 0
    assert q(2, 58, 40, 16) - q(2, 57, 40, 16) in (0, 256)          # the intermediate holds exactly the batch's rows
    assert q(64, 64 * 4096, 4096, 1024) > 0 and q(1, max_side, max_side, max_out) > 0
    for bad in ((0, 58, 40, 16), (2, 0, 40, 16), (2, 58, 0, 16), (2, 58, 40, 0), (2, 58, max_side + 1, 16), (2, 58, 40, max_out + 1),
                (2, 1 << 31, 40, 16), ((1 << 24) + 1, 1 << 25, 40, 16)):
        assert q(*bad) == 0, bad

    fake = ctypes.c_void_p(0x10000)          # never dereferenced: every call below is refused before anything is launched
    good = [(0, 40, 30, 3, 0, 40, 0, 30), (3600, 20, 10, 1, 2, 20, 1, 9)]      # crops of 40 x 30 and 18 x 8
    nbytes = 3600 + 200
    need = q(2, 40 + 18, 40, 16)

    def call(rows=good, packed=fake, nb=nbytes, desc=True, N=None, S=16, y=fake, ws=fake, wsn=need):
        d = kernels.image_descs(rows)
        return L.t2i_preprocess_images(packed, nb, ctypes.cast(d, ctypes.c_void_p) if desc else None, len(rows) if N is None else N, S, y,
                                       ws, wsn, None)
    invalid = {
        'packed NULL': dict(packed=None), 'desc NULL': dict(desc=False), 'y NULL': dict(y=None), 'N = 0': dict(N=0), 'N < 0': dict(N=-1),
        'S = 0': dict(S=0), 'S < 0': dict(S=-5), 'S above the limit': dict(S=max_out + 1),
        '2 channels': dict(rows=[(0, 40, 30, 2, 0, 40, 0, 30)]), '5 channels': dict(rows=[good[0], (3600, 5, 5, 5, 0, 5, 0, 5)]),
        'zero height': dict(rows=[(0, 0, 30, 3, 0, 0, 0, 30)]), 'side above the limit': dict(rows=[(0, max_side + 1, 1, 1, 0, 1, 0, 1)], nb=1 << 20),
        'crop below': dict(rows=[(0, 40, 30, 3, 0, 41, 0, 30)]), 'crop right': dict(rows=[(0, 40, 30, 3, 0, 40, 0, 31)]),
        'crop above': dict(rows=[(0, 40, 30, 3, -1, 40, 0, 30)]), 'crop left': dict(rows=[(0, 40, 30, 3, 0, 40, -1, 30)]),
        'empty rows': dict(rows=[(0, 40, 30, 3, 7, 7, 0, 30)]), 'empty columns': dict(rows=[(0, 40, 30, 3, 0, 40, 9, 9)]),
        'reversed': dict(rows=[(0, 40, 30, 3, 9, 2, 0, 30)]),
        'past the buffer': dict(nb=3600 + 199), 'offset past the buffer': dict(rows=[(1 << 40, 4, 4, 1, 0, 4, 0, 4)]),
        'negative offset': dict(rows=[(-4, 40, 30, 3, 0, 40, 0, 30)]),
    }
    for what, kw in invalid.items():
        assert call(**kw) == -1, what                                  # T2I_ERR_INVALID
        assert b't2i_preprocess_images' in L.t2i_last_error(), what
    assert b'image 1' in (call(rows=[good[0], (3600, 5, 5, 5, 0, 5, 0, 5)]), L.t2i_last_error())[1]
    for what, kw in {'ws NULL': dict(ws=None), 'ws misaligned': dict(ws=ctypes.c_void_p(0x10004)), 'ws short': dict(wsn=need - 1),
                     'ws empty': dict(wsn=0)}.items():
        assert call(**kw) == -2, what                                  # T2I_ERR_WORKSPACE
        assert b'workspace' in L.t2i_last_error(), what

    def tables(filter=1, sizes=fake, N=3, out=16, b=fake, c=fake, kmax=5):
        return L.t2i_pillow_tables(filter, sizes, N, out, b, c, kmax, None)
    for what, kw in {'filter': dict(filter=2), 'sizes NULL': dict(sizes=None), 'bounds NULL': dict(b=None), 'coeffs NULL': dict(c=None),
                     'N': dict(N=0), 'out': dict(out=0), 'out above the limit': dict(out=max_out + 1), 'kmax': dict(kmax=0)}.items():
        assert tables(**kw) == -1, what
        assert b't2i_pillow_tables' in L.t2i_last_error(), what

    import torch
    with pytest.raises(ValueError, match='preprocess_images'):
        kernels.preprocess_images(torch.zeros(10, dtype=torch.float32), good, 16)
    with pytest.raises(ValueError, match='image_descs'):
        kernels.preprocess_images(torch.zeros(10, dtype=torch.uint8), [(0, 1, 1)], 16)
    with pytest.raises(RuntimeError, match='no CPU path'):
        kernels.preprocess_images(torch.zeros(4000, dtype=torch.uint8), good, 16)


# ---- the commands, with the device call replaced by the host statement ------------------------------------------------------
FLOWERS = ([(40, 60, 3), (33, 50, 3), (64, 48, 1), (20, 90, 3), (57, 31, 3)], [(48, 48, 3), (25, 70, 1), (70, 25, 3)])
BIRDS = ([(60, 80, 3, '12.0 5.0 40.0 30.0'), (50, 50, 3, '0.0 0.0 50.0 50.0'), (45, 70, 1, '30.0 10.0 39.0 33.0'), (80, 40, 3, '5.0 50.0 20.0 28.0')],
         [(64, 64, 3, '20.0 20.0 10.0 10.0'), (30, 90, 3, '60.0 2.0 29.0 27.0')])


@pytest.fixture
def host_device(monkeypatch):
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess import image_store as IS, stage_images as SI
    calls = {'chunks': 0}

    def chunk(packed, rows, size, device):
        calls['chunks'] += 1
        return PC.host_chunk(packed, rows, size, device)
    monkeypatch.setattr(IS, 'open_device', lambda: 'host')
    monkeypatch.setattr(IS, 'transform_chunk', chunk)
    monkeypatch.setattr(SI, 'resize_store', PC.host_resize_store)
    return calls


def _load(path):
    import joblib
    return np.asarray(joblib.load(path))


def test_flowers_command_writes_ordered_stores_and_keeps_existing(tmp_path, host_device):
    from t2i_amd.evaluation.resize import resize_u8_bicubic
    from t2i_amd.preprocess import image_store as IS, preprocess_flowers as PF
    root = PC.flowers_tree(str(tmp_path / 'flowers'), *FLOWERS)
    written = PF.main(['--dir', root, '--load-size', '32', '--stage-sizes', '4', '16', '--workers', '3'])
    assert len(written) == 6
    for split, n in (('train', 5), ('test', 3)):
        store = _load(IS.store_path(root, split, 32))
        assert store.dtype == np.uint8 and store.shape == (n, 32, 32, 3)
        assert np.array_equal(store, PC.expected_flowers(root, split, 32))
        assert len({store[i].tobytes() for i in range(n)}) == n                    # distinct images: the order is observable
        for s in (4, 16):
            assert np.array_equal(_load(IS.store_path(root, split, s)), np.stack([resize_u8_bicubic(im, s, s) for im in store]))
    # a second run keeps everything; a removed stage store is derived from the kept load-size store, without decoding
    before = host_device['chunks']
    assert PF.main(['--dir', root, '--load-size', '32', '--stage-sizes', '4', '16']) == {}
    os.remove(IS.store_path(root, 'test', 4))
    assert list(PF.main(['--dir', root, '--load-size', '32', '--stage-sizes', '4', '16'])) == [IS.store_path(root, 'test', 4)]
    assert host_device['chunks'] == before
    assert len(PF.main(['--dir', root, '--load-size', '32', '--stage-sizes', '4', '16', '--force'])) == 6
    assert host_device['chunks'] > before
    # chunk boundaries and decode order do not change the store
    paths = PF.image_paths(root, PF.load_filenames(os.path.join(root, 'train')))
    whole, st1 = IS.build_store(paths, None, 32, 'host', chunk_bytes=1 << 30, workers=1)
    split_up, st2 = IS.build_store(paths, None, 32, 'host', chunk_bytes=7000, workers=16)
    assert st1['chunks'] == 1 and st2['chunks'] >= 3 and np.array_equal(whole, split_up)
    assert np.array_equal(whole, _load(IS.store_path(root, 'train', 32)))


def test_birds_command_crops_by_box_and_joins_by_name(tmp_path, host_device):
    from t2i_amd.preprocess import image_store as IS, preprocess_birds as PB
    root = PC.birds_tree(str(tmp_path / 'birds'), *BIRDS)
    written = PB.main(['--dir', root, '--load-size', '24', '--stage-sizes', '8'])
    assert len(written) == 4
    for split, n in (('train', 4), ('test', 2)):
        store = _load(IS.store_path(root, split, 24))
        assert store.dtype == np.uint8 and store.shape == (n, 24, 24, 3)
        assert np.array_equal(store, PC.expected_birds(root, split, 24))
        assert _load(IS.store_path(root, split, 8)).shape == (n, 8, 8, 3)


def test_commands_check_everything_before_any_work(tmp_path, monkeypatch):
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess import image_store as IS, preprocess_birds as PB, preprocess_flowers as PF

    def touched(*a, **k):
        raise AssertionError('work started')
    monkeypatch.setattr(IS, 'open_device', touched)
    monkeypatch.setattr(IS, 'decode', touched)
    with pytest.raises(FileNotFoundError, match='does not exist'):
        PF.main(['--dir', str(tmp_path / 'none')])
    froot = PC.flowers_tree(str(tmp_path / 'flowers'), *FLOWERS)
    os.remove(os.path.join(froot, 'jpg', 'image_00007.jpg'))                      # a test-split image: found before train is touched
    with pytest.raises(FileNotFoundError, match='image_00007.jpg'):
        PF.main(['--dir', froot, '--load-size', '32'])
    os.remove(os.path.join(froot, 'test', 'filenames.pickle'))
    with pytest.raises(FileNotFoundError, match='filenames.pickle'):
        PF.main(['--dir', froot, '--load-size', '32'])
    for argv in (['--dir', froot, '--chunk-mb', '0'], ['--dir', froot, '--workers', '0'], []):
        with pytest.raises(SystemExit):
            PF.main(argv)
    with pytest.raises(ValueError, match='upscale'):
        PF.main(['--dir', froot, '--load-size', '32', '--stage-sizes', '64'])
    broot = PC.birds_tree(str(tmp_path / 'birds'), *BIRDS)
    boxes = os.path.join(broot, 'CUB_200_2011', 'bounding_boxes.txt')
    names = os.path.join(broot, 'CUB_200_2011', 'images.txt')
    keep_b, keep_n = open(boxes).read(), open(names).read()
    open(boxes, 'w').writelines(keep_b.splitlines(True)[:-1])
    open(names, 'w').writelines(keep_n.splitlines(True)[:-1])                     # the last listed image (a train key) has no box
    with pytest.raises(KeyError, match='no bounding box'):
        PB.main(['--dir', broot, '--load-size', '24'])
    open(boxes, 'w').write(keep_b)
    open(names, 'w').write(keep_n)
    shutil.rmtree(os.path.join(broot, 'CUB_200_2011', 'images', '002.Species_2'))
    with pytest.raises(FileNotFoundError, match='Species_2'):
        PB.main(['--dir', broot, '--load-size', '24'])
    assert not [f for f in os.listdir(os.path.join(broot, 'train')) if f.endswith('images.pickle')]


def test_missing_gpu_is_a_runtime_error(tmp_path, monkeypatch):
    import torch
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess import preprocess_flowers as PF
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    root = PC.flowers_tree(str(tmp_path / 'flowers'), *FLOWERS)
    with pytest.raises(RuntimeError, match='no ROCm device'):
        PF.main(['--dir', root, '--load-size', '32'])


def test_written_store_is_read_by_textdataset(tmp_path, host_device):
    import pickle
    import t2i_amd  # noqa: F401
    from t2i_amd.preprocess import preprocess_flowers as PF
    from t2i_amd.preprocess.dataset import TextDataset
    root = PC.flowers_tree(str(tmp_path / 'flowers'), *FLOWERS)
    PF.main(['--dir', root, '--load-size', '76'])                                # FINAL_SIZE_TO_ORIG[64]
    for split, n in (('train', 5), ('test', 3)):
        with open(os.path.join(root, split, TextDataset.EMBEDDINGS), 'wb') as f:
            pickle.dump(np.zeros((n, 2, 8), np.float32), f)
        with open(os.path.join(root, split, TextDataset.CLASSES), 'wb') as f:
            pickle.dump(list(range(1, n + 1)), f)
    ds = TextDataset(root, 64, device='cpu')
    train = ds.get_data(os.path.join(root, 'train'))
    assert train.num_examples == 5 and tuple(train.images.shape) == (5, 76, 76, 3)
    assert np.array_equal(train.images.numpy(), PC.expected_flowers(root, 'train', 76))
    assert list(train.filenames) == ['jpg/image_%05d' % k for k in range(1, 6)]
