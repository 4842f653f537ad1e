#!/usr/bin/env python
"""PGGAN stage-7 scoring and the stage-size image stores on one GPU.  One JSON line:
  images_per_s    a whole scoring step per batch of eval_pggan.py (B = 64, the reference's): the full-width stage-7 generator
                  (random weights, conditioning noise on) -> clip -> t2i_resample_bilinear 256 -> 299 from the fp32 store ->
                  InceptionV3 forward (random He-scaled weights, 20 classes), over --iters batches;
  split_ms        the same step's device time per batch in three parts: generator (with the clip), resize, Inception;
  stores          preprocess/stage_images.resize_store on a synthetic uint8 600 x 600 store of --images images (8 189: the
                  flowers train + test splits): upload in 256 MiB chunks, the seven bicubic resizes 600 -> 4 ... 304, download.
                  Wall-clock seconds, pickling excluded."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.models.inception import model as M  # noqa: E402
from t2i_amd.models.pggan.eval_pggan import generate  # noqa: E402
from t2i_amd.models.pggan.pggan import PGGAN  # noqa: E402
from t2i_amd.preprocess.stage_images import DEFAULT_SIZES, resize_store  # noqa: E402
from bench_inception import random_weights, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64, help='eval_pggan.py batch (the reference: 64)')
    ap.add_argument('--stage', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--images', type=int, default=8189, help='images in the synthetic 600 store (flowers: 7034 + 1155)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pggan_eval.py needs a GPU')
    dev = torch.device('cuda', 0)
    B = args.batch
    m = PGGAN(B, None, None, None, None, None, None, args.stage, False, build_model=False, device=dev)
    with K.dry_run(), torch.no_grad():
        m.generator(torch.empty(B, m.z_dim, device=dev), torch.empty(B, m.embed_dim, device=dev), stages=args.stage, t=False)
    net = M.InceptionV3.from_arrays(random_weights(20), 20, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn((B, m.z_dim), generator=g, device=dev)
    cond = torch.randn((B, m.embed_dim), generator=g, device=dev)

    def gen():
        return generate(m, z, cond)

    img = gen()
    x = K.resample_bilinear(img, M.IMAGE_SIZE, M.IMAGE_SIZE)

    def step():
        xx = K.resample_bilinear(gen(), M.IMAGE_SIZE, M.IMAGE_SIZE)
        with torch.no_grad():
            net(xx)

    def fwd():
        with torch.no_grad():
            net(x)
    t_step = timed(step, args.iters)
    t_gen = timed(gen, args.iters)
    t_resize = timed(lambda: K.resample_bilinear(img, M.IMAGE_SIZE, M.IMAGE_SIZE, out=x), args.iters)
    t_incep = timed(fwd, args.iters)
    del m, net, img, x
    torch.cuda.empty_cache()

    # a flowers-sized 600 store: 64 random images repeated (filling 8 GB with fresh random bytes would dominate the run)
    rng = np.random.default_rng(0)
    tile = rng.integers(0, 256, (64, 600, 600, 3), dtype=np.uint8)
    store = np.empty((args.images, 600, 600, 3), np.uint8)
    for i in range(0, args.images, 64):
        store[i:i + 64] = tile[:min(64, args.images - i)]
    resize_store(store[:64], DEFAULT_SIZES, dev)                  # tables and workspace warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    resize_store(store, DEFAULT_SIZES, dev)
    torch.cuda.synchronize()
    t_stores = time.perf_counter() - t0
    print(json.dumps({'bench': 'pggan_stage%d_scoring' % args.stage, 'batch': B, 'images_per_s': round(B / t_step, 1),
                      'step_ms': round(t_step * 1e3, 3),
                      'split_ms': {'generator': round(t_gen * 1e3, 3), 'resize': round(t_resize * 1e3, 3),
                                   'inception': round(t_incep * 1e3, 3)},
                      'stores': {'images': args.images, 'sizes': list(DEFAULT_SIZES), 'seconds': round(t_stores, 2),
                                 'source_GB': round(store.nbytes / 1e9, 2)}}), flush=True)


if __name__ == '__main__':
    main()
