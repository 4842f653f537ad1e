"""Stage-size image stores for PGGAN: `<s>images.pickle` of every split, derived from `<source>images.pickle` on the GPU.

    python -m t2i_amd.preprocess.stage_images --dir DATASET_DIR [--source 600] [--sizes 4 8 16 38 76 152 304] [--force]

The reference's preprocess_flowers.py / preprocess_birds.py write each size s by `scipy.misc.imresize(img, [s, s], 'bicubic')`
of the uint8 600 x 600 image, which is Pillow's `Image.resize((s, s), BICUBIC)` on that image unchanged (bytescale returns a
uint8 array as it is).  SciPy no longer has imresize, and the reference ships IMG_SIZES = [600] only; this command derives the
other stores of FINAL_SIZE_TO_ORIG from the 600 one with the same arithmetic, bit for bit: kernels.resample_u8 (Pillow's
bicubic tables applied by t2i_resample_bilinear).

For `train/` and `test/`: the source store is read with joblib, uploaded in chunks of at most --chunk-mb MiB (the kernel's
workspace is bounded by the chunk as well), each chunk is resized to every requested size, and each store is written with
joblib.dump as the reference does.  Existing stores are kept unless --force; a size above the source is refused.  Every
argument and file check runs before any device work."""
import argparse
import os
import sys
import time

import numpy as np

SPLITS = ('train', 'test')
DEFAULT_SIZES = (4, 8, 16, 38, 76, 152, 304)


def store_path(dataset_dir, split, size):
    return os.path.join(dataset_dir, split, '%dimages.pickle' % size)


def plan(dataset_dir, source=600, sizes=DEFAULT_SIZES, force=False):
    """-> [(split, [sizes to write])] for the splits that need work.  Raises on a bad size or a missing source store."""
    sizes = [int(s) for s in sizes]
    bad = [s for s in sizes if s <= 0]
    if bad:
        raise ValueError('stage_images: sizes must be positive, got %s' % bad)
    up = [s for s in sizes if s > source]
    if up:
        raise ValueError('stage_images: refusing to upscale the %d store to %s' % (source, up))
    out = []
    for split in SPLITS:
        todo = [s for s in dict.fromkeys(sizes) if s != source and (force or not os.path.exists(store_path(dataset_dir, split, s)))]
        if not todo:
            continue
        src = store_path(dataset_dir, split, source)
        if not os.path.isfile(src):
            raise FileNotFoundError('stage_images: %s does not exist (the reference preprocessing writes %dimages.pickle into '
                                    'train/ and test/)' % (src, source))
        out.append((split, todo))
    return out


def resize_store(images, sizes, device, chunk_bytes=256 << 20):
    """uint8 [N, S, S, 3] host store -> {size: uint8 [N, size, size, 3]} on the host, through the device in chunks."""
    import torch
    from .. import kernels as K
    images = np.ascontiguousarray(images, np.uint8)
    if images.ndim != 4 or images.shape[3] != 3 or images.shape[1] != images.shape[2]:
        raise ValueError('stage_images: expected a uint8 [N, S, S, 3] store, got %s' % (images.shape,))
    n = images.shape[0]
    per = max(1, int(chunk_bytes // max(images[0].nbytes, 1)))
    out = {s: np.empty((n, s, s, 3), np.uint8) for s in sizes}
    for i in range(0, n, per):
        src = torch.from_numpy(images[i:i + per]).to(device)
        for s in sizes:
            out[s][i:i + src.shape[0]] = K.resample_u8(src, s, s, 'bicubic').cpu().numpy()
        del src
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m t2i_amd.preprocess.stage_images', description=__doc__.split('\n\n')[0])
    ap.add_argument('--dir', required=True, help='DATASET_DIR with train/ and test/')
    ap.add_argument('--source', type=int, default=600, help='size of the store to derive from [600]')
    ap.add_argument('--sizes', type=int, nargs='+', default=list(DEFAULT_SIZES), help='sizes to write [4 8 16 38 76 152 304]')
    ap.add_argument('--force', action='store_true', help='rewrite stores that already exist')
    ap.add_argument('--chunk-mb', type=int, default=256, help='source MiB uploaded per chunk [256]')
    args = ap.parse_args(argv)
    if args.chunk_mb <= 0:
        ap.error('--chunk-mb must be positive')
    if not os.path.isdir(args.dir):
        raise FileNotFoundError('stage_images: DATASET_DIR %r does not exist' % args.dir)
    work = plan(args.dir, args.source, args.sizes, args.force)
    for split in SPLITS:
        if split not in dict(work):
            print('%s: every store exists (--force rewrites them)' % split)
    if not work:
        return {}
    import joblib
    import torch
    import t2i_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise RuntimeError('stage_images resizes on the GPU and no ROCm device is visible')
    dev = torch.device('cuda')
    written = {}
    for split, sizes in work:
        t0 = time.time()
        src = store_path(args.dir, split, args.source)
        images = np.asarray(joblib.load(src))
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[1:] != (args.source, args.source, 3):
            raise ValueError('stage_images: %s holds %s %s, expected uint8 [N, %d, %d, 3]' % (
                src, images.dtype, images.shape, args.source, args.source))
        stores = resize_store(images, sizes, dev, args.chunk_mb << 20)
        for s in sizes:
            path = store_path(args.dir, split, s)
            joblib.dump(stores[s], path)
            written[path] = stores[s].shape
            print('save to: ', path, stores[s].shape)
        print('%s: %d images, %d stores in %.1f s' % (split, images.shape[0], len(sizes), time.time() - t0))
        sys.stdout.flush()
    return written


if __name__ == '__main__':
    main()
