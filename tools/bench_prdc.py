#!/usr/bin/env python
"""The costs of precision / recall / density / coverage (csrc/t2i_knn.hip, evaluation/prdc.py), each next to the same step written
with tensor-library calls in the same process — one JSON line per step and size, at M = N = 8192 and 32768 rows of D = 2048, k = 5:

  knn       one K.knn_dist2(X, X, 5, exclude_self) call (two norm launches, the fused product + selection, the fold) against: over
            row chunks that fit memory, |q|^2 + |r|^2 - 2 Q R^T in float64 (one GEMM per chunk, the cheapest way to say it with a
            tensor library; torch.cdist in float64 takes the same route), the diagonal set to +inf, clamp, topk(5, largest=False).
  ball      one K.ball_counts(G, R, r2) call against the same chunked distance, then (d <= r2).sum(1) and d.min(1).
  finalize  a whole ManifoldMetrics.finalize() — four passes, the finiteness checks and the host ratios — against the chain of the
            same rival steps.

The rival's float64 copies of the features are made outside the timed region.  Its float32 form is listed beside it as information,
with the number of decisions (d2 <= r2, elementwise over the M x N pairs) on which it disagrees with the float64 form; the HIP
kernel's counts are compared with the float64 form's in the same way (`hip_count_rows_differing`).  `hip_tflops` is the product's
algorithmic 2 M N D over the whole call's time, nothing else.  Timing as tools/bench_swd.py: warm-up calls, then REPS rounds of ITERS
back-to-back calls between device events, the HIP and the tensor-library rounds alternating; the median round is reported and the
spread (fastest and slowest round) next to it.

    python tools/bench_prdc.py [--reps 3] [--only knn|ball|finalize] [--sizes 8192,32768]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.evaluation import prdc  # noqa: E402

CHUNK = 4096                                              # query rows per rival GEMM: 4096 x 32768 float64 distances are 1 GiB


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


def chunks(q, r, qn, rn):
    """Yields (row offset, clamped Gram-form distances [c, N]) in the dtype of q."""
    for s in range(0, q.shape[0], CHUNK):
        d = torch.addmm(qn[s:s + CHUNK, None] + rn[None, :], q[s:s + CHUNK], r.t(), alpha=-2.0)
        yield s, d.clamp_(min=0.0)


def torch_knn(x, xn, k):
    out = []
    for s, d in chunks(x, x, xn, xn):
        i = torch.arange(d.shape[0], device=d.device)
        d[i, i + s] = float('inf')
        out.append(torch.topk(d, k, dim=1, largest=False, sorted=True)[0])
    return torch.cat(out)


def torch_ball(q, r, qn, rn, r2):
    cnt, dmin = [], []
    for _, d in chunks(q, r, qn, rn):
        cnt.append((d <= r2[None, :]).sum(1))
        dmin.append(d.min(1)[0])
    return torch.cat(cnt), torch.cat(dmin)


def torch_finalize(real, gen, rn, gn, k):
    r2_real = torch_knn(real, rn, k)[:, k - 1]
    r2_gen = torch_knn(gen, gn, k)[:, k - 1]
    cnt_gen, _ = torch_ball(gen, real, gn, rn, r2_real)
    cnt_real, dmin_real = torch_ball(real, gen, rn, gn, r2_gen)
    return prdc.ratios(cnt_gen.cpu().numpy(), cnt_real.cpu().numpy(), (dmin_real <= r2_real).cpu().numpy(), k)


def decisions_differing(q, r, r2, q64, r64, r2_64):
    """Elementwise over the M x N pairs: how often (d2 <= r2) in the arithmetic of q differs from float64."""
    n = 0
    qn, rn, qn64, rn64 = (q * q).sum(1), (r * r).sum(1), (q64 * q64).sum(1), (r64 * r64).sum(1)
    for (_, d), (_, d64) in zip(chunks(q, r, qn, rn), chunks(q64, r64, qn64, rn64)):
        n += int(((d <= r2[None, :]) != (d64 <= r2_64[None, :])).sum())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--only', default='')
    ap.add_argument('--sizes', default='8192,32768')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_prdc.py measures on the GPU; there is nothing to measure without one'
    torch.manual_seed(0)
    D, k = 2048, 5
    for n in (int(v) for v in args.sizes.split(',')):
        iters = 3 if n <= 8192 else 1
        W = torch.randn(64, D, device='cuda') / 8.0
        real = (torch.randn(n, 64, device='cuda') @ W + 0.05 * torch.randn(n, D, device='cuda')).contiguous()
        gen = ((0.8 * torch.randn(n, 64, device='cuda') + 0.3) @ W + 0.05 * torch.randn(n, D, device='cuda')).contiguous()
        real64, gen64 = real.double(), gen.double()
        norms = {torch.float64: ((real64 * real64).sum(1), (gen64 * gen64).sum(1)), torch.float32: ((real * real).sum(1), (gen * gen).sum(1))}
        flops = 2.0 * n * n * D

        r2_hip = K.knn_dist2(real, real, k, exclude_self=True)[:, k - 1].contiguous()
        r2_64 = torch_knn(real64, norms[torch.float64][0], k)[:, k - 1].contiguous()
        r2_32 = torch_knn(real, norms[torch.float32][0], k)[:, k - 1].contiguous()

        if args.only in 'knn':
            compare('knn', (n, n, D, k), {
                'hip': lambda: K.knn_dist2(real, real, k, exclude_self=True),
                'torch_f64': lambda: torch_knn(real64, norms[torch.float64][0], k),
                'torch_f32': lambda: torch_knn(real, norms[torch.float32][0], k)}, args.reps, iters, 1, flops,
                max_rel_diff_radius_vs_torch_f64=float(((r2_hip - r2_64).abs() / r2_64).max()),
                max_rel_diff_radius_torch_f32_vs_f64=float(((r2_32.double() - r2_64).abs() / r2_64).max()), hip_launches=4)

        if args.only in 'ball':
            cnt, dmin = K.ball_counts(gen, real, r2_hip)
            ref = torch_ball(gen64, real64, norms[torch.float64][1], norms[torch.float64][0], r2_64)
            extra = {}
            if n <= 8192:
                extra['torch_f32_decisions_differing'] = decisions_differing(gen, real, r2_32, gen64, real64, r2_64)
                extra['decisions'] = n * n
            compare('ball', (n, n, D), {
                'hip': lambda: K.ball_counts(gen, real, r2_hip),
                'torch_f64': lambda: torch_ball(gen64, real64, norms[torch.float64][1], norms[torch.float64][0], r2_64),
                'torch_f32': lambda: torch_ball(gen, real, norms[torch.float32][1], norms[torch.float32][0], r2_32)}, args.reps, iters, 1, flops,
                hip_count_rows_differing=int((cnt.long() != ref[0]).sum()), max_abs_diff_dmin_vs_torch_f64=float((dmin - ref[1]).abs().max()),
                hip_launches=4, **extra)

        if args.only in 'finalize':
            mm = prdc.ManifoldMetrics(D, 'cuda', nearest_k=k)
            mm.add_real(real)
            mm.add_gen(gen)
            got = mm.finalize()
            want = torch_finalize(real64, gen64, *norms[torch.float64], k)
            f32 = torch_finalize(real, gen, *norms[torch.float32], k)
            compare('finalize', (n, n, D, k), {
                'hip': mm.finalize,
                'torch_f64': lambda: torch_finalize(real64, gen64, *norms[torch.float64], k),
                'torch_f32': lambda: torch_finalize(real, gen, *norms[torch.float32], k)}, args.reps, 1, 1, 4 * flops,
                hip=got, torch_f64=want, torch_f32=f32, equal_to_torch_f64=bool(got == want), hip_launches=16)
        del real, gen, real64, gen64, norms
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
