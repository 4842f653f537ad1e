"""Shared by tests/test_preprocess_host.py and tests/test_preprocess_gpu.py: the ragged shapes, synthetic images, tiny dataset
trees written with Pillow, and the host statement applied to a packed batch."""
import os
import pickle

import numpy as np

# (height, width, S): the two datasets' typical downscales, two upscales, near-identity, extreme aspect ratios, identity
RAGGED = [(500, 667, 600), (333, 500, 360), (90, 120, 360), (5, 5, 600), (601, 599, 600), (7, 1000, 600), (1200, 37, 360),
          (600, 600, 600)]


def image(seed, h, w, c=3, lo=37, hi=201):
    """uint8 [h, w, c] (c == 1: [h, w]) with values in [lo, hi], both attained: smooth ramps plus noise, so that the stretch and
    both filter lobes matter."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(yy / 7.0 + seed)[..., None] + np.cos(xx / 5.0)[..., None] * np.array([1.0, 0.6, -0.8, 0.3])[:c]) * 0.25 + 0.5
    v = np.clip(base + rng.normal(0, 0.2, (h, w, c)), 0, 1)
    img = (lo + v * (hi - lo)).astype(np.uint8)
    flat = img.reshape(-1)
    flat[rng.integers(0, flat.size)] = lo
    flat[(rng.integers(0, flat.size) + 1) % flat.size] = hi if flat.size > 1 else lo
    return img[:, :, 0] if c == 1 else img


def scipy_bytescale(data):
    """scipy.misc.bytescale (scipy <= 1.2) of a float64 array with the default arguments."""
    data = np.asarray(data, np.float64)
    cmin, cmax = data.min(), data.max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1
    bytedata = (data - cmin) * (255.0 / cscale)
    return (bytedata.clip(0, 255) + 0.5).astype(np.uint8)


def pack(images, boxes=None):
    """[uint8 image] (+ [(y1, y2, x1, x2)] or None) -> (uint8 [bytes], descriptor rows), as preprocess/image_store.pack."""
    from t2i_amd.preprocess import image_store as IS
    boxes = boxes or [None] * len(images)
    return IS.pack([(im, b if b is not None else (0, im.shape[0], 0, im.shape[1])) for im, b in zip(images, boxes)])


def host_statement(packed, rows, size):
    """preprocess/utils.py transform of every described image -> uint8 [N, size, size, 3]."""
    from t2i_amd.preprocess import utils as U
    out = []
    for off, h, w, c, y1, y2, x1, x2 in rows:
        img = packed[off:off + h * w * c].reshape((h, w) if c == 1 else (h, w, c))
        out.append(U.transform(U.colorize(img)[y1:y2, x1:x2], size, False, None))
    return np.stack(out)


def host_chunk(packed, rows, size, device):
    """Stands in for image_store.transform_chunk."""
    out = host_statement(packed, rows, size)
    return lambda: out


def host_resize_store(images, sizes, device, chunk_bytes=0):
    """Stands in for stage_images.resize_store."""
    from t2i_amd.evaluation.resize import resize_u8_bicubic
    return {s: np.stack([resize_u8_bicubic(im, s, s) for im in images]) for s in sizes}


def _save_jpeg(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(img).save(path, quality=92)


def flowers_tree(root, shapes_train, shapes_test):
    """shapes: [(h, w, channels)] -> the directory; keys jpg/image_%05d, filenames.pickle written with joblib."""
    import joblib
    k = 0
    for split, shapes in (('train', shapes_train), ('test', shapes_test)):
        names = []
        for h, w, c in shapes:
            k += 1
            key = 'jpg/image_%05d' % k
            _save_jpeg(os.path.join(root, key + '.jpg'), image(k, h, w, c, lo=20 + k, hi=180 + k))
            names.append(key)
        os.makedirs(os.path.join(root, split), exist_ok=True)
        joblib.dump(names, os.path.join(root, split, 'filenames.pickle'))
    return root


def birds_tree(root, items_train, items_test):
    """items: [(h, w, channels, 'x y w h' as CUB writes a box)] -> the directory; filenames.pickle written with pickle.  images.txt
    lists the test images first, so the join is by name, not by split order."""
    k, listing = 0, []
    for split, items in (('train', items_train), ('test', items_test)):
        names = []
        for h, w, c, box in items:
            k += 1
            key = '%03d.Species_%d/Species_%d_%04d' % (k % 3 + 1, k % 3 + 1, k % 3 + 1, k)
            _save_jpeg(os.path.join(root, 'CUB_200_2011', 'images', key + '.jpg'), image(100 + k, h, w, c, lo=10 + k, hi=150 + 3 * k))
            names.append(key)
            listing.append((key + '.jpg', box))
        os.makedirs(os.path.join(root, split), exist_ok=True)
        with open(os.path.join(root, split, 'filenames.pickle'), 'wb') as f:
            pickle.dump(names, f)
    listing = listing[len(items_train):] + listing[:len(items_train)]
    with open(os.path.join(root, 'CUB_200_2011', 'images.txt'), 'w') as f:
        f.writelines('%d %s\n' % (i + 1, name) for i, (name, _) in enumerate(listing))
    with open(os.path.join(root, 'CUB_200_2011', 'bounding_boxes.txt'), 'w') as f:
        f.writelines('%d %s\n' % (i + 1, box) for i, (_, box) in enumerate(listing))
    return root


def expected_flowers(root, split, size):
    import joblib
    from t2i_amd.preprocess import utils as U
    names = joblib.load(os.path.join(root, split, 'filenames.pickle'))
    return np.stack([U.get_image('%s/%s.jpg' % (root, key), size) for key in names])


def expected_birds(root, split, size):
    from t2i_amd.preprocess import preprocess_birds as PB, utils as U
    with open(os.path.join(root, split, 'filenames.pickle'), 'rb') as f:
        names = pickle.load(f)
    boxes = PB.load_bbox(root)
    return np.stack([U.get_image('%s/CUB_200_2011/images/%s.jpg' % (root, key), size, is_crop=True, bbox=boxes[key]) for key in names])
