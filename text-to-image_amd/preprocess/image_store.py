"""What preprocess_flowers.py and preprocess_birds.py share: from a list of image files (and, for birds, boxes) to the
`<size>images.pickle` stores of one split.

Decoding stays on the host (Pillow, in a thread pool: the decoder releases the GIL); everything after it — colorize, crop,
scipy's bytescale, Pillow's bicubic resize — is one kernels.preprocess_images call per chunk of decoded bytes.  While chunk k is
on the device the pool decodes chunk k + 1: a chunk's result is only fetched when the next chunk has been packed.  Results land
at their index, so the store's order is the file list's order whatever order decoding finishes in."""
import collections
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import utils as U

MAX_WORKERS = 16


def store_path(dataset_dir, split, size):
    return os.path.join(dataset_dir, split, '%dimages.pickle' % size)


def open_device():
    import torch
    import t2i_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise RuntimeError('the image stores are resized on the GPU and no ROCm device is visible (there is no CPU path)')
    return torch.device('cuda')


def decode(path, bbox=None):
    """-> (uint8 image as stored [H, W] / [H, W, 3] / [H, W, 4], (y1, y2, x1, x2)): the crop is checked here, by file name."""
    img = U.imread_u8(path)
    box = U.crop_box(img.shape, bbox) if bbox is not None else (0, img.shape[0], 0, img.shape[1])
    return img, U.check_crop(img.shape, box, path)


def pack(decoded):
    """[(image, box)] -> (uint8 [bytes], N descriptor rows of kernels.preprocess_images)."""
    rows, off = [], 0
    for img, (y1, y2, x1, x2) in decoded:
        rows.append((off, img.shape[0], img.shape[1], 1 if img.ndim == 2 else img.shape[2], y1, y2, x1, x2))
        off += img.size
    packed = np.empty(off, np.uint8)
    for (o, *_), (img, _) in zip(rows, decoded):
        packed[o:o + img.size] = img.reshape(-1)
    return packed, rows


def transform_chunk(packed, rows, size, device):
    """Starts the device work of one chunk and returns fetch() -> uint8 [n, size, size, 3] on the host."""
    import torch
    from .. import kernels as K
    try:
        y = K.preprocess_images(torch.from_numpy(packed).to(device), rows, size)
    except torch.cuda.OutOfMemoryError as e:
        raise RuntimeError('the device ran out of memory on a chunk of %d images (%d MiB decoded; the filter tables are sized by the '
                           "chunk's largest image side): use a smaller --chunk-mb" % (len(rows), packed.nbytes >> 20)) from e
    return lambda: y.cpu().numpy()


def build_store(paths, boxes, size, device, chunk_bytes=256 << 20, workers=8):
    """paths [N] (and boxes [N] of [x, y, w, h], or None) -> (uint8 [N, size, size, 3], timings dict)."""
    n = len(paths)
    workers = max(1, min(int(workers), MAX_WORKERS))
    out = np.empty((n, size, size, 3), np.uint8)
    stats = {'images': n, 'chunks': 0, 'decode_cpu_s': 0.0, 'decode_wait_s': 0.0, 'device_wait_s': 0.0}

    def job(i):
        t0 = time.perf_counter()
        r = decode(paths[i], None if boxes is None else boxes[i])
        return r, time.perf_counter() - t0

    pending = None                          # (fetch, first index, count) of the chunk that is on the device

    def flush():
        nonlocal pending
        if pending is not None:
            t0 = time.perf_counter()
            fetch, lo, cnt = pending
            out[lo:lo + cnt] = fetch()
            stats['device_wait_s'] += time.perf_counter() - t0
            pending = None

    with ThreadPoolExecutor(workers) as pool:
        window = collections.deque()        # decode jobs in flight, in file order; bounded so that decoded images do not pile up
        nxt = 0
        chunk, chunk_lo, chunk_size = [], 0, 0
        for i in range(n):
            while nxt < n and len(window) < 4 * workers:
                window.append(pool.submit(job, nxt))
                nxt += 1
            t0 = time.perf_counter()
            (img, box), dt = window.popleft().result()
            stats['decode_wait_s'] += time.perf_counter() - t0
            stats['decode_cpu_s'] += dt
            if chunk and chunk_size + img.size > chunk_bytes:
                packed, rows = pack(chunk)
                flush()
                pending = (transform_chunk(packed, rows, size, device), chunk_lo, len(chunk))
                stats['chunks'] += 1
                chunk, chunk_lo, chunk_size = [], i, 0
            chunk.append((img, box))
            chunk_size += img.size
        if chunk:
            packed, rows = pack(chunk)
            flush()
            pending = (transform_chunk(packed, rows, size, device), chunk_lo, len(chunk))
            stats['chunks'] += 1
        flush()
    return out, stats


def check_sizes(what, load_size, stage_sizes):
    stage_sizes = [int(s) for s in stage_sizes]
    if load_size <= 0 or any(s <= 0 for s in stage_sizes):
        raise ValueError('%s: sizes must be positive, got --load-size %d --stage-sizes %s' % (what, load_size, stage_sizes))
    up = [s for s in stage_sizes if s > load_size]
    if up:
        raise ValueError('%s: refusing to upscale the %d store to %s' % (what, load_size, up))
    return [s for s in dict.fromkeys(stage_sizes) if s != load_size]


def check_files(what, paths):
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError('%s: %d of %d image files do not exist, the first: %s' % (what, len(missing), len(paths), missing[0]))


def write_split(what, dataset_dir, split, paths, boxes, load_size, stage_sizes, force, chunk_bytes, workers, device):
    """Writes the split's load-size store (from the image files) and stage-size stores (from the load-size store) that do not
    exist yet, or all of them with force.  `device` is a zero-argument callable, called once there is work.  -> {path: shape}"""
    import joblib
    from . import stage_images as SI
    written = {}
    load_path = store_path(dataset_dir, split, load_size)
    todo = [s for s in stage_sizes if force or not os.path.exists(store_path(dataset_dir, split, s))]
    make_load = force or not os.path.exists(load_path)
    if not make_load and not todo:
        print('%s: every store exists (--force rewrites them)' % split)
        return written
    t0 = time.time()
    if make_load:
        print('%s: %d images -> %d x %d' % (split, len(paths), load_size, load_size))
        images, stats = build_store(paths, boxes, load_size, device(), chunk_bytes, workers)
        joblib.dump(images, load_path)
        written[load_path] = images.shape
        print('wrote %s %s' % (load_path, images.shape))
        print('%s: decode %.1f s of CPU in %d threads, waited %.1f s for decoding and %.1f s for the device, %d chunks' % (
            split, stats['decode_cpu_s'], max(1, min(int(workers), MAX_WORKERS)), stats['decode_wait_s'], stats['device_wait_s'],
            stats['chunks']))
    else:
        images = np.asarray(joblib.load(load_path))
        if images.dtype != np.uint8 or images.shape != (len(paths), load_size, load_size, 3):
            raise ValueError('%s: %s holds %s %s, expected uint8 %s (--force rebuilds it)' % (
                what, load_path, images.dtype, images.shape, (len(paths), load_size, load_size, 3)))
    if todo:
        stores = SI.resize_store(images, todo, device(), chunk_bytes)
        for s in todo:
            path = store_path(dataset_dir, split, s)
            joblib.dump(stores[s], path)
            written[path] = stores[s].shape
            print('wrote %s %s' % (path, stores[s].shape))
    print('%s: %d images in %.1f s' % (split, len(paths), time.time() - t0))
    return written


def add_arguments(ap, load_size):
    ap.add_argument('--dir', required=True, help='dataset directory with train/ and test/')
    ap.add_argument('--load-size', type=int, default=load_size, help='side of the store made from the image files [%d]' % load_size)
    ap.add_argument('--stage-sizes', type=int, nargs='*', default=[], help='also derive these stores from the load-size one (stage_images)')
    ap.add_argument('--force', action='store_true', help='rewrite stores that already exist')
    ap.add_argument('--chunk-mb', type=int, default=256, help='decoded MiB uploaded per kernel call [256]')
    ap.add_argument('--workers', type=int, default=8, help='decoder threads [8], at most %d' % MAX_WORKERS)


def check_arguments(ap, args):
    if args.chunk_mb <= 0:
        ap.error('--chunk-mb must be positive')
    if args.workers <= 0:
        ap.error('--workers must be positive')
    if not os.path.isdir(args.dir):
        raise FileNotFoundError('%s: dataset directory %r does not exist' % (ap.prog, args.dir))


class LazyDevice(object):
    """open_device() on first use: a run that finds every store in place never touches the GPU."""

    def __init__(self):
        self.dev = None

    def __call__(self):
        if self.dev is None:
            self.dev = open_device()
        return self.dev
