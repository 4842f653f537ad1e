#!/usr/bin/env python
"""The sliced Wasserstein distance's three costs (csrc/t2i_swd.hip, evaluation/swd.py), each next to the same step written with
tensor-library calls in the same process — one JSON line per step:

  pyramid    t2i_laplacian_pyramid of 64 images of 256 x 256 x 3, 5 levels, against conv2d (depthwise 5 x 5, stride 2, reflect padding)
             and a zero-insert followed by conv2d with 4 F on the NCHW copy of the batch (the transposition is not timed);
  sort       t2i_segmented_sort_f32 of [256, 2^20] against torch.sort(dim=1).  Both sort a fresh copy of the same random data each
             time (a sorted input would be a different problem for a library sort); the copy is timed on its own and reported, not
             subtracted.  The line carries the pass structure of the bitonic sort: launches, and bytes moved per pass;
  finalize   SlicedWasserstein.finalize() with the descriptor stores of 8192 images of 256 x 256 x 3 (random descriptors: the cost
             does not depend on the values), against per level torch mean / std, a materialised standardised matrix, torch.matmul,
             torch.sort and an abs-mean.

Timing as tools/bench_ops.py: warm-up calls, then REPS rounds of ITERS back-to-back calls between device events, the HIP and the
tensor-library rounds alternating; the median round is reported and the spread (fastest and slowest round) next to it.

    python tools/bench_swd.py [--reps 5] [--only pyramid|sort|finalize] [--images 8192]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.evaluation import swd  # noqa: E402


def _round(fn, iters):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def compare(step, shape, hip, lib, reps, iters, warmup, **extra):
    for _ in range(warmup):
        hip(); lib()
    torch.cuda.synchronize()
    th, tl = [], []
    for _ in range(reps):
        th.append(_round(hip, iters))
        tl.append(_round(lib, iters))
    h, l = statistics.median(th), statistics.median(tl)
    line = {'step': step, 'shape': list(shape), 'hip_ms': round(h * 1e3, 3), 'hip_spread_ms': [round(min(th) * 1e3, 3), round(max(th) * 1e3, 3)],
            'torch_ms': round(l * 1e3, 3), 'torch_spread_ms': [round(min(tl) * 1e3, 3), round(max(tl) * 1e3, 3)],
            'hip_over_torch': round(h / l, 3), 'reps': reps, 'iters': iters}
    line.update(extra)
    print(json.dumps(line), flush=True)


def torch_pyramid(x_nchw, levels, f):
    """The same pyramid by the tensor library: reflect padding is scipy's 'mirror'."""
    C = x_nchw.shape[1]
    g = [x_nchw]
    for _ in range(levels - 1):
        g.append(torch.nn.functional.conv2d(torch.nn.functional.pad(g[-1], (2, 2, 2, 2), mode='reflect'), f, stride=2, groups=C))
    out = []
    for i in range(levels - 1):
        z = torch.zeros_like(g[i])
        z[:, :, ::2, ::2] = g[i + 1]
        out.append(g[i] - torch.nn.functional.conv2d(torch.nn.functional.pad(z, (2, 2, 2, 2), mode='reflect'), 4.0 * f, groups=C))
    return out + [g[-1]]


def sort_passes(n, chunk):
    """(LDS launches, global passes) of the bitonic sort of one segment of n floats."""
    if n <= chunk:
        return 1, 0
    lds, glob, k = 1, 0, 2 * chunk
    while k <= n:
        j = k // 2
        while j >= chunk:
            r = 0
            jj = j
            while jj >= chunk and r < 3:
                r += 1
                jj //= 2
            glob += 1
            j >>= r
        lds += 1
        k *= 2
    return lds, glob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', default='')
    ap.add_argument('--images', type=int, default=8192, help='finalize: images per side [8192]')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_swd.py measures on the GPU; there is nothing to measure without one'
    torch.manual_seed(0)

    if a.only in 'pyramid':
        B, S, C, L = 64, 256, 3, 5
        x = torch.rand((B, S, S, C), device='cuda') * 2 - 1
        xn = x.permute(0, 3, 1, 2).contiguous()
        k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device='cuda') / 16
        f = (k[:, None] * k[None, :]).expand(C, 1, 5, 5).contiguous()
        got, want = K.laplacian_pyramid(x, L), torch_pyramid(xn, L, f)
        err = max(float((g.permute(0, 3, 1, 2) - w).abs().max()) for g, w in zip(got, want))
        n = x.numel()
        compare('pyramid', (B, S, S, C), lambda: K.laplacian_pyramid(x, L), lambda: torch_pyramid(xn, L, f), a.reps, 20, 5,
                levels=L, max_abs_diff=err, hip_launches=2 * (L - 1),
                hip_bytes_floor=int(4 * n * (1 + 1 / 4 + 1 / 16 + 1 / 64) * 2 + 4 * n * (1 + 1 / 4 + 1 / 16 + 1 / 64 + 1 / 256)))

    if a.only in 'sort':
        segs, n = 256, 1 << 20
        src = torch.randn((segs, n), device='cuda')
        buf = torch.empty_like(src)

        def hip():
            buf.copy_(src)
            K.segmented_sort(buf)

        def lib():
            buf.copy_(src)
            torch.sort(buf, dim=1)
        hip()
        same = bool(torch.equal(buf, torch.sort(src, dim=1)[0]))
        tc = statistics.median(_round(lambda: buf.copy_(src), 5) for _ in range(a.reps))
        lds, glob = sort_passes(n, K.SORT_CHUNK)
        compare('sort', (segs, n), hip, lib, a.reps, 3, 2, equal_to_torch_sort=same, copy_ms_included_in_both=round(tc * 1e3, 3),
                chunk=K.SORT_CHUNK, lds_launches=lds, global_passes=glob, bytes_per_pass=2 * 4 * segs * n,
                bytes_moved=(lds + glob) * 2 * 4 * segs * n)

    if a.only in 'finalize':
        n_img, side, C = a.images, 256, 3
        sw = swd.SlicedWasserstein((side, side, C), n_img, 'cuda', seed=0)
        for st in sw.real + sw.gen:
            st.normal_()
        for st in sw.gen:
            st.mul_(1.1).add_(0.05)
        sw.count = n_img
        rows, D, S, R = n_img * sw.nhoods, 49 * C, sw.dirs, sw.repeats
        result = {}

        def hip():
            sw.rng = np.random.RandomState(1)
            result['hip'] = sw.finalize()

        def lib():
            rng = np.random.RandomState(1)
            levels = []
            for i in range(sw.levels):
                std = []
                for X in (sw.real[i], sw.gen[i]):
                    v = X.view(rows, C, 49)
                    m = v.mean(dim=(0, 2), keepdim=True, dtype=torch.float64)
                    s = (v.double() - m).square_().mean(dim=(0, 2), keepdim=True).sqrt_()
                    std.append(((v - m.float()) / s.float()).view(rows, D))
                dists = []
                for _ in range(R):
                    d = torch.from_numpy(swd.draw_directions(rng, D, S)).cuda()
                    pa = torch.sort(torch.matmul(d.t(), std[0].t()), dim=1)[0]          # [S, rows]: a slice is one contiguous run
                    pb = torch.sort(torch.matmul(d.t(), std[1].t()), dim=1)[0]
                    dists.append((pa - pb).abs_().mean(dtype=torch.float64))
                levels.append(float(torch.stack(dists).mean().cpu()) * 1e3)
                del std
            result['torch'] = levels
        hip(); lib()
        compare('finalize', (n_img, side, side, C), hip, lib, min(a.reps, 3), 1, 0, rows_per_level=rows, levels_hip=result['hip']['levels'],
                levels_torch=result['torch'])


if __name__ == '__main__':
    main()
