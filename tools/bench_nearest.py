#!/usr/bin/env python
"""t2i_nearest_images (the visualiser's closest-neighbour search) at flowers shape: a seeded uint8 store of N = 7034 train
images at S = 76, 64x64 queries, one random crop table entry per (query, image).  For Q = 1, 8, 64: 10 warm-up calls, then
the mean of >= 200 back-to-back calls timed with device events on the launch stream.  One JSON line per Q:
  us_per_call, hbm_bytes = N*S*S*3 (store) + 3*4*Q*N (crop tables) + Q*out*out*3*4 (queries), fp64_fma = Q*N*out*out*3,
  hbm_bound_share = (hbm_bytes / 6.29 TB/s, the measured copy bandwidth of MI355X_MICROARCH.md) / us_per_call.
Then the CPU time of ONE query done the way the reference does it (float64 NumPy over all N crops) for comparison."""
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

HBM_MEASURED = 6.29e12   # B/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=7034)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--qs', default='1,8,64')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_nearest.py needs a GPU')
    N, S, out = args.n, 76, 64
    rng = np.random.default_rng(0)
    dev = torch.device('cuda')
    src_h = rng.integers(0, 256, (N, S, S, 3), dtype=np.uint8)
    src = torch.from_numpy(src_h).to(dev)
    for Q in [int(q) for q in args.qs.split(',')]:
        queries = torch.from_numpy(rng.uniform(-1, 1, (Q, out, out, 3)).astype(np.float32)).to(dev)
        tabs = [torch.from_numpy(rng.integers(0, hi, (Q, N)).astype(np.int32)).to(dev) for hi in (S - out + 1, S - out + 1, 2)]
        fn = lambda: K.nearest_images(src, queries, *tabs)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        us = s.elapsed_time(e) / args.iters * 1e3
        nbytes = N * S * S * 3 + 3 * 4 * Q * N + Q * out * out * 3 * 4
        print(json.dumps({'kernel': 't2i_nearest_images', 'N': N, 'S': S, 'out': out, 'Q': Q, 'iters': args.iters,
                          'us_per_call': round(us, 2), 'hbm_bytes': nbytes, 'fp64_fma': Q * N * out * out * 3,
                          'hbm_bound_us': round(nbytes / HBM_MEASURED * 1e6, 2),
                          'hbm_bound_share': round(nbytes / HBM_MEASURED * 1e6 / us, 3)}), flush=True)
    # the reference's way, one query: float64 distance to every crop of the store (crop gather included)
    q = rng.uniform(-1, 1, (out, out, 3)).astype(np.float32).astype(np.float64)
    r0, c0 = rng.integers(0, S - out + 1, N), rng.integers(0, S - out + 1, N)
    t0 = time.perf_counter()
    best, bi = np.inf, -1
    for n in range(N):
        real = src_h[n, r0[n]:r0[n] + out, c0[n]:c0[n] + out].astype(np.float32) * np.float32(2. / 255) - np.float32(1.)
        d = np.linalg.norm(q - real.astype(np.float64))
        if d < best:
            best, bi = d, n
    print(json.dumps({'cpu_numpy_one_query_s': round(time.perf_counter() - t0, 3), 'N': N}), flush=True)


if __name__ == '__main__':
    main()
