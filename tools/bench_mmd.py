#!/usr/bin/env python
"""The costs of the Kernel Inception distance (csrc/t2i_mmd.hip, evaluation/mmd.py), each next to the same step written with
tensor-library calls in the same process — one JSON line per step, at S = 100 subsets of m = 1000 rows of D = 2048 from two sets of
8192 rows:

  sums      one K.poly_mmd_sums call (the fused gather + products + kernel + sums, then the fold: 2 launches) against, per subset:
            a gather of the m rows of each set, three float64 GEMMs (x x^T, y y^T, x y^T), (. / D + 1) ** 3 and the sums (the
            symmetric ones as (sum - trace) / 2) — what StyleGAN2-ADA and torch-fidelity do, said with a tensor library.
  finalize  a whole KernelDistance.finalize() — the finiteness checks, the host tables and their upload, the call and the host
            estimates — against the same chain with the rival sums.

The rival's float64 copies of the features are made outside the timed region.  Its float32 form is listed beside it as information,
with its distance from the float64 form.  `hip_tflops` is the algorithmic 2 * 3 S m^2 D of the three full products over the whole
call's time (the kernel skips the tiles below the diagonal: about two thirds of that is executed).  Timing as tools/bench_prdc.py:
warm-up calls, then REPS rounds of ITERS back-to-back calls between device events, the HIP and the tensor-library rounds
alternating; the median round is reported and the spread (fastest and slowest round) next to it.

    python tools/bench_mmd.py [--reps 3] [--only sums|finalize] [--rows 8192] [--subsets 100] [--size 1000]
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
from t2i_amd.evaluation import mmd  # noqa: E402


def _round(fn, iters):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def compare(step, shape, fns, reps, iters, warmup, flops, **extra):
    """fns: name -> callable; the rounds of all of them alternate."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t[name].append(_round(fn, iters))
    line = {'step': step, 'shape': list(shape)}
    for name, v in t.items():
        line[name + '_ms'] = round(statistics.median(v) * 1e3, 3)
        line[name + '_spread_ms'] = [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]
    line['hip_over_torch_f64'] = round(statistics.median(t['hip']) / statistics.median(t['torch_f64']), 3)
    line['hip_tflops'] = round(flops / statistics.median(t['hip']) * 1e-12, 2)
    line.update(reps=reps, iters=iters, **extra)
    print(json.dumps(line), flush=True)


def torch_sums(x, y, ix, iy):
    """-> [S, 3] in the dtype of x: per subset a gather, three GEMMs, the kernel and the sums.  ix, iy: device int64 [S, m]."""
    D = x.shape[1]
    out = torch.empty((ix.shape[0], 3), dtype=x.dtype, device=x.device)
    for s in range(ix.shape[0]):
        a, b = x[ix[s]], y[iy[s]]
        kxx, kyy, kxy = (a @ a.t() / D + 1) ** 3, (b @ b.t() / D + 1) ** 3, (a @ b.t() / D + 1) ** 3
        out[s, 0] = (kxx.sum() - kxx.diagonal().sum()) / 2
        out[s, 1] = (kyy.sum() - kyy.diagonal().sum()) / 2
        out[s, 2] = kxy.sum()
    return out


def torch_finalize(kd, x, y):
    """KernelDistance.finalize() with the rival sums (x, y: the features in the rival's dtype)."""
    for rows in (kd.real, kd.gen):
        assert bool(torch.isfinite(rows.rows()).all())
    ix, iy, m = kd.tables()
    sums = torch_sums(x, y, torch.from_numpy(ix).to(x.device).long(), torch.from_numpy(iy).to(x.device).long())
    est = mmd.estimates(sums.double().cpu().numpy(), m)
    return dict(kid=float(np.mean(est)), kid_std=float(np.std(est)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--only', default='')
    ap.add_argument('--rows', type=int, default=8192)
    ap.add_argument('--subsets', type=int, default=100)
    ap.add_argument('--size', type=int, default=1000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mmd.py measures on the GPU; there is nothing to measure without one'
    torch.manual_seed(0)
    n, S, m, D = args.rows, args.subsets, args.size, 2048
    W = torch.randn(64, D, device='cuda') / 8.0
    real = (torch.randn(n, 64, device='cuda') @ W + 0.05 * torch.randn(n, D, device='cuda')).contiguous()
    gen = ((0.8 * torch.randn(n, 64, device='cuda') + 0.3) @ W + 0.05 * torch.randn(n, D, device='cuda')).contiguous()
    real64, gen64 = real.double(), gen.double()
    kd = mmd.KernelDistance(D, 'cuda', num_subsets=S, max_subset_size=m)
    kd.add_real(real)
    kd.add_gen(gen)
    ix_h, iy_h, m = kd.tables()
    ix, iy = torch.from_numpy(ix_h).cuda(), torch.from_numpy(iy_h).cuda()
    ixl, iyl = ix.long(), iy.long()
    flops = 2.0 * 3 * S * m * m * D

    if args.only in 'sums':
        hip = K.poly_mmd_sums(real, gen, ix, iy)
        ref = torch_sums(real64, gen64, ixl, iyl)
        f32 = torch_sums(real, gen, ixl, iyl).double()
        w = 2.0 / (m * (m - 1)), 2.0 / (m * m)

        def kid(sm):
            return float((sm[:, 0] * w[0] + sm[:, 1] * w[0] - sm[:, 2] * w[1]).mean())
        compare('sums', (n, n, D, S, m), {
            'hip': lambda: K.poly_mmd_sums(real, gen, ix, iy, check_indices=False),
            'torch_f64': lambda: torch_sums(real64, gen64, ixl, iyl),
            'torch_f32': lambda: torch_sums(real, gen, ixl, iyl)}, args.reps, 2, 1, flops,
            max_rel_diff_sums_vs_torch_f64=float(((hip - ref).abs() / ref.abs()).max()),
            max_rel_diff_sums_torch_f32_vs_f64=float(((f32 - ref).abs() / ref.abs()).max()),
            kid_hip=kid(hip), kid_torch_f64=kid(ref), kid_torch_f32=kid(f32), hip_launches=2, hip_work_items=K.poly_mmd_items(S, m))

    if args.only in 'finalize':
        got = kd.finalize()
        want = torch_finalize(kd, real64, gen64)
        f32 = torch_finalize(kd, real, gen)
        compare('finalize', (n, n, D, S, m), {
            'hip': kd.finalize,
            'torch_f64': lambda: torch_finalize(kd, real64, gen64),
            'torch_f32': lambda: torch_finalize(kd, real, gen)}, args.reps, 1, 1, flops,
            hip=dict(kid=got['kid'], kid_std=got['kid_std']), torch_f64=want, torch_f32=f32, hip_launches=2)


if __name__ == '__main__':
    main()
