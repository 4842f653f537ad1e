#!/usr/bin/env python
"""The load-size image stores on one GPU, synthetic images (no dataset needed).  One JSON line with, for a flowers-shaped batch
(height 500, widths 500 .. 1000, -> 600) and a birds-shaped one (square crops of 150 .. 500 pixels out of larger images, -> 360),
images per second of
  kernel        kernels.preprocess_images alone, the packed batch resident on the device (device time, median of --repeats);
  device_path   upload of the packed batch + the kernel call + download of the store (wall clock);
  pillow        the same bytescale + Image.resize(BICUBIC) by NumPy and Pillow on the host, one thread — the reference's serial loop
                after its decode;
and, for the flowers shape, `command`: preprocess_flowers on a generated tree of --files JPEGs (wall clock, pickling included),
with the share of that time the main thread spent waiting for the decoder threads."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.preprocess import image_store as IS, preprocess_flowers as PF  # noqa: E402
from t2i_amd.preprocess.utils import bytescale_lut  # noqa: E402


def synthetic(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 110 + 70 * np.sin(yy / 23.0)[..., None] * np.cos(xx / 17.0)[..., None] * np.array([1.0, 0.7, -0.5])
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 5, 250).astype(np.uint8)


def flowers_batch(rng, n):
    return [(synthetic(rng, 500, int(w)), None) for w in rng.integers(500, 1001, n)]


def birds_batch(rng, n):
    out = []
    for side in rng.integers(150, 501, n):
        h, w = int(side) + int(rng.integers(0, 120)), int(side) + int(rng.integers(0, 200))
        y1, x1 = int(rng.integers(0, h - side + 1)), int(rng.integers(0, w - side + 1))
        out.append((synthetic(rng, h, w), (y1, y1 + int(side), x1, x1 + int(side))))
    return out


def pillow_one(img, box, size):
    if box is not None:
        img = img[box[0]:box[1], box[2]:box[3]]
    u8 = bytescale_lut(img.min(), img.max())[img]
    return np.asarray(Image.fromarray(u8).resize((size, size), Image.BICUBIC))


def measure(name, batch, size, dev, repeats):
    decoded = [(im, b if b is not None else (0, im.shape[0], 0, im.shape[1])) for im, b in batch]
    packed, rows = IS.pack(decoded)
    n = len(batch)
    dp = torch.from_numpy(packed).to(dev)
    y = K.preprocess_images(dp, rows, size)                      # workspace warm
    check = y[:2].cpu().numpy()
    for i in range(2):
        assert np.array_equal(check[i], pillow_one(batch[i][0], batch[i][1], size)), 'device and Pillow disagree'
    descs = K.image_descs(rows)
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        K.preprocess_images(dp, descs, size)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    t_kernel = float(np.median(times))
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        K.preprocess_images(torch.from_numpy(packed).to(dev), descs, size).cpu()
        walls.append(time.perf_counter() - t0)
    t_path = float(np.median(walls))
    m = min(n, 32)
    t0 = time.perf_counter()
    for im, b in batch[:m]:
        pillow_one(im, b, size)
    t_pil = (time.perf_counter() - t0) / m
    return {'shape': name, 'images': n, 'size': size, 'packed_MB': round(packed.nbytes / 1e6, 1),
            'kernel_images_per_s': round(n / t_kernel, 1), 'kernel_ms': round(t_kernel * 1e3, 3),
            'device_path_images_per_s': round(n / t_path, 1), 'pillow_images_per_s': round(1.0 / t_pil, 1)}


def command(rng, files, dev_workers):
    root = tempfile.mkdtemp(prefix='bench_preprocess_')
    try:
        import joblib
        names = []
        os.makedirs(os.path.join(root, 'jpg'))
        for k in range(files):
            key = 'jpg/image_%05d' % (k + 1)
            Image.fromarray(synthetic(rng, 500, int(rng.integers(500, 1001)))).save(os.path.join(root, key + '.jpg'), quality=90)
            names.append(key)
        for split, part in (('train', names[:-8]), ('test', names[-8:])):
            os.makedirs(os.path.join(root, split))
            joblib.dump(part, os.path.join(root, split, 'filenames.pickle'))
        paths = PF.image_paths(root, names)
        t0 = time.perf_counter()
        _, stats = IS.build_store(paths, None, 600, torch.device('cuda'), workers=dev_workers)
        t_store = time.perf_counter() - t0
        t0 = time.perf_counter()
        PF.main(['--dir', root, '--workers', str(dev_workers), '--force'])
        t_cmd = time.perf_counter() - t0
        t0 = time.perf_counter()
        for p in paths[:32]:
            IS.decode(p)
        t_dec = (time.perf_counter() - t0) / 32
        return {'files': files, 'workers': dev_workers, 'command_images_per_s': round(files / t_cmd, 1), 'command_s': round(t_cmd, 2),
                'store_images_per_s': round(files / t_store, 1), 'decode_wait_share': round(stats['decode_wait_s'] / t_store, 3),
                'device_wait_share': round(stats['device_wait_s'] / t_store, 3),
                'decode_one_thread_images_per_s': round(1.0 / t_dec, 1)}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=192, help='images per synthetic batch')
    ap.add_argument('--files', type=int, default=256, help='JPEGs in the generated tree of the whole-command figure')
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_preprocess.py needs a GPU')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    out = {'bench': 'preprocess', 'form': 'one thread per output byte, intermediate in global memory',
           'flowers': measure('flowers', flowers_batch(rng, args.images), 600, dev, args.repeats),
           'birds': measure('birds', birds_batch(rng, args.images), 360, dev, args.repeats),
           'command': command(rng, args.files, args.workers)}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
