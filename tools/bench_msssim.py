#!/usr/bin/env python
"""The multi-scale SSIM's two costs (csrc/t2i_msssim.hip, evaluation/msssim.py), each next to the same steps written with
tensor-library calls in the same process — one JSON line per step and size, at 64 pairs of 256 x 256 x 3 and of 64 x 64 x 3:

  scale   one t2i_ssim_scale call (the cs and ssim of every pair and the next scale's images, two launches) against: the five
          products stacked into one [N, 5 C, H, W] tensor, one depthwise conv2d along y and one along x with the 1-D window (the
          separable form, the cheapest way to say it with a tensor library), the elementwise map, two means and avg_pool2d(2).
          The rival runs in float64, which has the kernel's accuracy; its float32 variant (off by 7e-5 on flat images, DESIGN
          4.33) is listed beside it as information.  `hip_no_downsample_ms` is the same call without the next scale: the difference
          is what the fused downsample costs; `hip_separate_downsample_ms` is that call followed by the next scale as launches of
          their own (t2i_pool2_sum with scale 0.25 on each image, the same means at these even sizes).
  add     a whole MultiScaleSSIM.add() — five scales, ten launches and two stacks — against the five-scale chain of the same rival.

The NCHW copies the rival reads are made outside the timed region.  Timing as tools/bench_swd.py: warm-up calls, then REPS rounds of
ITERS back-to-back calls between device events, the HIP and the tensor-library rounds alternating; the median round is reported and
the spread (fastest and slowest round) next to it.

    python tools/bench_msssim.py [--reps 5] [--only scale|add]
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
from t2i_amd.evaluation import msssim  # noqa: E402

F = torch.nn.functional


def _round(fn, iters):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def compare(step, shape, fns, reps, iters, warmup, **extra):
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
    line.update(reps=reps, iters=iters, **extra)
    print(json.dumps(line), flush=True)


def torch_scale(a, b, g, c1, c2, down):
    """One scale by the tensor library: a, b [N, C, H, W] in the arithmetic's dtype, g the 1-D window in that dtype."""
    C, S = a.shape[1], g.numel()
    x = torch.cat([a, b, a * a, b * b, a * b], 1)
    x = F.conv2d(x, g.view(1, 1, S, 1).expand(5 * C, 1, S, 1), groups=5 * C)
    x = F.conv2d(x, g.view(1, 1, 1, S).expand(5 * C, 1, 1, S), groups=5 * C)
    mu1, mu2, e11, e22, e12 = torch.split(x, C, 1)
    v1 = 2.0 * (e12 - mu1 * mu2) + c2
    v2 = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + c2
    cs = (v1 / v2).mean(dim=(1, 2, 3))
    ssim = (((2.0 * mu1 * mu2 + c1) * v1) / ((mu1 * mu1 + mu2 * mu2 + c1) * v2)).mean(dim=(1, 2, 3))
    if not down:
        return ssim, cs, None, None
    return ssim, cs, F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)


def torch_chain(a, b, windows, c1, c2):
    ssim, cs = [], []
    for l, g in enumerate(windows):
        s, c, a, b = torch_scale(a, b, g, c1, c2, l + 1 < len(windows))
        ssim.append(s)
        cs.append(c)
    return torch.stack(ssim), torch.stack(cs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_msssim.py measures on the GPU; there is nothing to measure without one'
    torch.manual_seed(0)
    for side, iters in ((256, 5), (64, 20)):
        N, C = 64, 3
        a = torch.randint(0, 256, (N, side, side, C), device='cuda').float()
        b = torch.clamp(torch.round(a + 25.0 * torch.randn_like(a)), 0, 255)
        ms = msssim.MultiScaleSSIM((side, side, C), 'cuda')
        nchw = {dt: (a.permute(0, 3, 1, 2).contiguous().to(dt), b.permute(0, 3, 1, 2).contiguous().to(dt)) for dt in (torch.float64, torch.float32)}
        wins = {dt: [torch.from_numpy(w).to('cuda', dt) for w in ms.windows] for dt in nchw}
        elems = a.numel()

        if args.only in 'scale':
            s, c, ah, bh = K.ssim_scale(a, b, ms.windows[0], ms.c1, ms.c2)
            ref = torch_scale(*nchw[torch.float64], wins[torch.float64][0], ms.c1, ms.c2, True)
            f32 = torch_scale(*nchw[torch.float32], wins[torch.float32][0], ms.c1, ms.c2, True)
            compare('scale', (N, side, side, C), {
                'hip': lambda: K.ssim_scale(a, b, ms.windows[0], ms.c1, ms.c2),
                'hip_no_downsample': lambda: K.ssim_scale(a, b, ms.windows[0], ms.c1, ms.c2, downsample=False),
                'hip_separate_downsample': lambda: (K.ssim_scale(a, b, ms.windows[0], ms.c1, ms.c2, downsample=False), K.pool2_sum(a, 0.25),
                                                    K.pool2_sum(b, 0.25)),
                'torch_f64': lambda: torch_scale(*nchw[torch.float64], wins[torch.float64][0], ms.c1, ms.c2, True),
                'torch_f32': lambda: torch_scale(*nchw[torch.float32], wins[torch.float32][0], ms.c1, ms.c2, True)}, args.reps, iters, 3,
                max_abs_diff_ssim_vs_torch_f64=float((s - ref[0]).abs().max()), max_abs_diff_cs_vs_torch_f64=float((c - ref[1]).abs().max()),
                max_abs_diff_ssim_torch_f32_vs_f64=float((f32[0].double() - ref[0]).abs().max()),
                next_scale_equal=bool(torch.equal(ah.permute(0, 3, 1, 2), ref[2].float())),
                separate_downsample_equal=bool(torch.equal(ah, K.pool2_sum(a, 0.25)) and torch.equal(bh, K.pool2_sum(b, 0.25))),
                hip_launches=2, hip_bytes_floor=int(4 * 2 * elems * 1.25), fp64_fma_per_output=int(7 * 11 * 42 / 32 + 5 * 11))

        if args.only in 'add':
            def hip_add():
                ms.cs, ms.ssim = [], []
                ms.add(a, b, quantized=True)
            hip_add()
            got = ms.finalize()
            ref = torch_chain(*nchw[torch.float64], wins[torch.float64], ms.c1, ms.c2)
            want, _ = msssim.combine(ref[1].cpu().numpy(), ref[0].cpu().numpy(), ms.weights)
            compare('add', (N, side, side, C), {
                'hip': hip_add,
                'torch_f64': lambda: torch_chain(*nchw[torch.float64], wins[torch.float64], ms.c1, ms.c2),
                'torch_f32': lambda: torch_chain(*nchw[torch.float32], wins[torch.float32], ms.c1, ms.c2)}, args.reps, iters, 3,
                max_abs_diff_values_vs_torch_f64=float(abs(got['values'] - want).max()), mean=got['mean'], hip_launches=10,
                windows=[len(w) for w in ms.windows])


if __name__ == '__main__':
    main()
