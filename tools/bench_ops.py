#!/usr/bin/env python
"""The memory-bound kernels of csrc/t2i_ops.hip (pixel_norm, nearest resize and its adjoint, pool AVG / MAX with their backward maps,
gn, the double backward of pixel_norm and layer_norm, the minibatch standard deviation) at PGGAN-sized tensors, and the Adam launch with and
without the weight EMA (`--only adam_ema`) and with per-slot multipliers (`--only adam_slots`) at the sizes of two generator arenas, and the
differentiable augmentation of csrc/t2i_augment.hip at the PGGAN trainer's shapes next to the same policy from tensor-library calls
(`--only diff_augment`), and the critic's optimizer step with and without spectral normalisation (`--only spectral_norm`), and the
anti-aliased resampling of csrc/t2i_resample.hip at the PGGAN trainer's full widths (`--only upfirdn`), and the style layer of
csrc/t2i_style.hip at the generator's B = 8 shapes next to layer_norm on the same tensors (`--only adain`), and the launches of a
weight-demodulated convolution besides its convolution (csrc/t2i_modconv.hip) next to the style layer in the same run (`--only modconv`), and that layer's second-order launches next to tensor-library calls (`--only modconv2`): one JSON line per kernel with the time per call, the bytes the algorithm moves (reads + writes, from the
shapes), bytes per second, and the ratio of that rate to a device-to-device copy that moves the SAME number of bytes (half read, half
written), timed in the same process.  Per measurement: 10 warm-up launches, then REPS rounds of 100 back-to-back launches between
device events, kernel and copy rounds alternating; the median round is reported.  Read the ratio, not the absolute rate, as the share
of what the memory system gives: a kernel and its copy touch the same number of bytes, so they sit in the same cache regime.  The
regime differs BETWEEN lines, though, and each line says which it is in: 'working_set_MB' is what one call touches and
'in_infinity_cache' whether that fits the 256 MiB Infinity Cache with room to spare (at most half of it).  Most lines do (a 34 MB
tensor and its results: repeated calls are served from the cache, kernel and copy alike); the x2 upscale and its adjoint touch 168 MB
per call, their copy likewise, and run at the rate of HBM.  Ratios are comparable within a regime, not across the two.

    python tools/bench_ops.py [--reps 5] [--iters 100] [--only SUBSTRING]
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


INFINITY_CACHE = 256 << 20


def _round(fn, iters):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def measure(name, shape, nbytes, fn, reps, iters, composed=None, others=None, extra=None):
    """extra: further fields of the line (a launch count); composed: the same operation as tensor-library calls, timed in the same alternating rounds ('composed_us', 'ratio_to_composed');
    others: {label: fn} of further launches on the same tensors, timed in the same rounds ('<label>_us')"""
    src = torch.empty(nbytes // 8, dtype=torch.float32, device='cuda').normal_()
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)          # moves nbytes: nbytes / 2 read + nbytes / 2 written
    for _ in range(10):
        fn(); copy()
        if composed is not None:
            composed()
        for other in (others or {}).values():
            other()
    torch.cuda.synchronize()
    tk, tc, tl, to = [], [], [], {k: [] for k in (others or {})}
    for _ in range(reps):
        tk.append(_round(fn, iters))
        tc.append(_round(copy, iters))
        if composed is not None:
            tl.append(_round(composed, iters))
        for k, other in (others or {}).items():
            to[k].append(_round(other, iters))
    t, c = statistics.median(tk), statistics.median(tc)
    line = {'kernel': name, 'shape': list(shape), 'us_per_call': round(t * 1e6, 2), 'bytes': nbytes,
            'working_set_MB': round(nbytes / 1e6, 1), 'in_infinity_cache': nbytes <= INFINITY_CACHE // 2,
            'GB_per_s': round(nbytes / t / 1e9, 1), 'copy_us': round(c * 1e6, 2), 'copy_GB_per_s': round(nbytes / c / 1e9, 1),
            'ratio_to_copy': round(c / t, 3), 'spread_us': [round(min(tk) * 1e6, 2), round(max(tk) * 1e6, 2)]}
    if composed is not None:
        line.update(composed_us=round(statistics.median(tl) * 1e6, 2), ratio_to_composed=round(statistics.median(tl) / t, 2))
    for k, ts in to.items():
        line['%s_us' % k] = round(statistics.median(ts) * 1e6, 2)
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def composed_diff_augment(x, P):
    """The policy 'color,translation,cutout' of utils.ops.diff_augment from tensor-library calls, the way the publication's code builds it
    (blends around the means, a padded index gather for the shift, a multiplicative mask for the cutout), NHWC, from the same table"""
    B, H, W, C = x.shape
    col = lambda j: P[:, j].view(B, 1, 1, 1)
    u = x + col(0)
    m = u.mean(3, keepdim=True)
    u = (u - m) * col(1) + m
    m = u.mean((1, 2, 3), keepdim=True)
    u = (u - m) * col(2) + m
    ar = lambda n, shape: torch.arange(n, device=x.device).view(shape)
    gy = (ar(H, (1, H, 1)) - P[:, 3].long().view(B, 1, 1) + 1).clamp(0, H + 1)
    gx = (ar(W, (1, 1, W)) - P[:, 4].long().view(B, 1, 1) + 1).clamp(0, W + 1)
    u = torch.nn.functional.pad(u, [0, 0, 1, 1, 1, 1])[ar(B, (B, 1, 1)), gy, gx]
    yy, xx = ar(H, (1, H, 1)), ar(W, (1, 1, W))
    inside = (yy >= P[:, 5].view(B, 1, 1)) & (yy < P[:, 6].view(B, 1, 1)) & (xx >= P[:, 7].view(B, 1, 1)) & (xx < P[:, 8].view(B, 1, 1))
    return u * (~inside).unsqueeze(3).to(u.dtype)


def composed_upfirdn(x, taps, u, d, p0, p1):
    """utils.ops.upfirdn2d from tensor-library calls, the way the publication's reference code builds it: zero-stuff, F.pad, a depthwise
    F.conv2d with the outer product of the reversed taps, a strided slice.  x: a channels-last NCHW view of the kernel's NHWC tensor."""
    B, C, H, W = x.shape
    if u == 2:
        z = x.new_zeros((B, C, 2 * H, 2 * W)).contiguous(memory_format=torch.channels_last)
        z[:, :, ::2, ::2] = x
    else:
        z = x
    z = torch.nn.functional.pad(z, [p0, p1, p0, p1])
    g = torch.tensor(taps, dtype=torch.float32, device=x.device).flip(0)
    w = (g[:, None] * g[None, :])[None, None].repeat(C, 1, 1, 1)
    y = torch.nn.functional.conv2d(z, w, groups=C)
    return y[:, :, ::d, ::d] if d == 2 else y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--only', default='', help='measure only the kernels whose line name contains this')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ops.py measures on the GPU; there is nothing to measure without one'
    m = lambda name, shape, nbytes, fn: measure(name, shape, nbytes, fn, a.reps, a.iters) if a.only in name else None
    for shape in ((8, 128, 128, 64), (64, 16, 16, 512)):
        B, H, W, C = shape
        x = torch.randn(shape, device='cuda')
        g = torch.randn(shape, device='cuda')
        n = x.numel()
        rows = n // C
        y, rn = K.pixel_norm_fwd(x, 1e-8, K.ACT_LRELU, 0.2)
        m('pixel_norm_fwd lrelu (r + w + rnorm)', shape, 8 * n + 4 * rows, lambda: K.pixel_norm_fwd(x, 1e-8, K.ACT_LRELU, 0.2))
        m('pixel_norm_bwd lrelu (2r + rnorm + w)', shape, 12 * n + 4 * rows, lambda: K.pixel_norm_bwd(g, y, rn, K.ACT_LRELU, 0.2))
        up = K.resize_nearest(x, 2 * H, 2 * W)
        m('resize_nearest x2 up (r + 4w)', shape, 20 * n, lambda: K.resize_nearest(x, 2 * H, 2 * W))
        m('resize_nearest_adj of x2 up (4r + w)', shape, 20 * n, lambda: K.resize_nearest_adj(up, H, W))
        m('resize_nearest /2 down (r/4 + w/4)', shape, 2 * n, lambda: K.resize_nearest(x, H // 2, W // 2))
        for op, nm in ((K.POOL_AVG, 'AVG'), (K.POOL_MAX, 'MAX')):
            yo, idx = K.pool_same_fwd(x, 2, op, want_idx=True)
            go = torch.randn_like(yo)
            extra = n if op == K.POOL_MAX else 0          # the int32 offsets, n / 4 of them
            m('pool_same_fwd %s s=2 (r + w/4%s)' % (nm, ' + idx/4' if extra else ''), shape, 5 * n + extra,
              lambda: K.pool_same_fwd(x, 2, op, want_idx=True))
            m('pool_same_bwd %s s=2 (r/4%s + w)' % (nm, ' + idx/4' if extra else ''), shape, 5 * n + extra,
              lambda: K.pool_same_bwd(go, idx, H, W, 2, op))
            if op == K.POOL_MAX:
                m('pool_same_take s=2 (r/4 + idx/4 + w/4)', shape, 3 * n, lambda: K.pool_same_take(x, idx, 2))
        yo3, _ = K.pool_same_fwd(x, 3, K.POOL_AVG)
        m('pool_same_fwd AVG s=3, padded (r + w/9)', shape, 4 * n + 4 * yo3.numel(), lambda: K.pool_same_fwd(x, 3, K.POOL_AVG))
        _, f = K.gn_fwd(x, 0.18)
        m('gn_fwd (r + 2w)', shape, 12 * n, lambda: K.gn_fwd(x, 0.18))
        m('mul, the gn backward (2r + w)', shape, 12 * n, lambda: K.mul(g, f))
        # second order of the two normalisations: v = the cotangent of the first-order input gradient
        v = torch.randn(shape, device='cuda')
        m('pixel_norm_bwd2 lrelu (3r + rnorm + 2w)', shape, 20 * n + 4 * rows, lambda: K.pixel_norm_bwd2(v, g, y, rn, K.ACT_LRELU, 0.2))
        gamma = torch.rand(C, device='cuda') + 0.5
        xhat = K.row_fma2(x, torch.ones(B, device='cuda'))                 # any [B, per] tensor serves as xhat for the timing
        yl = K.bn_apply(xhat, gamma, torch.zeros_like(gamma), K.ACT_LRELU, 0.2)
        rstd = torch.rand(B, device='cuda') + 0.5
        sums = K.layer_norm_bwd2_sums(v, g, xhat, yl, gamma, K.ACT_LRELU, 0.2)
        m('layer_norm_bwd2_sums lrelu (4r)', shape, 16 * n, lambda: K.layer_norm_bwd2_sums(v, g, xhat, yl, gamma, K.ACT_LRELU, 0.2))
        m('layer_norm_bwd2_apply lrelu (4r + 2w)', shape, 24 * n,
          lambda: K.layer_norm_bwd2_apply(v, g, xhat, yl, gamma, rstd, sums, K.ACT_LRELU, 0.2))
        m('layer_norm_bwd2_apply lrelu + hgz for dgamma (4r + 3w)', shape, 28 * n,
          lambda: K.layer_norm_bwd2_apply(v, g, xhat, yl, gamma, rstd, sums, K.ACT_LRELU, 0.2, want_hgz=True))

    # minibatch standard deviation: the critic's own 4x4 map, and a streaming size in the cache regime of the lines above
    for shape in ((64, 4, 4, 512), (64, 16, 16, 512)):
        x = torch.randn(shape, device='cuda')
        v = torch.randn(shape, device='cuda')
        gs = torch.randn(shape[0], 4, device='cuda')
        n = x.numel()
        m('minibatch_stddev_fwd G=4 F=4 (r)', shape, 4 * n, lambda: K.minibatch_stddev_fwd(x, 4, 4))
        m('minibatch_stddev_bwd G=4 F=4 (r + w)', shape, 8 * n, lambda: K.minibatch_stddev_bwd(gs, x, 4, 4))
        m('minibatch_stddev_bwd2 G=4 F=4 (2r + w)', shape, 12 * n, lambda: K.minibatch_stddev_bwd2(v, x, gs, 4, 4))

    # Adam with the exponential moving average of the weights, beta1 = 0 and m = NULL as the PGGAN and wgancls
    # optimizers run it, at the sizes of the stage-7 PGGAN generator arena and of the wgancls generator arena: the plain launch
    # (w, g, v read; w, v written), the fused launch (+ the shadow read and written), and the plain launch followed by the same
    # shadow update as tensor-library launches (sub, mul, sub in place: 3 reads + 1 write of an arena more than the fused form's 8 bytes)
    for n, arena in ((23598252, 'pggan stage 7 g_arena'), (22643292, 'wgancls g_arena')):
        w, g, v = torch.randn(n, device='cuda') * 0.05, torch.randn(n, device='cuda'), torch.rand(n, device='cuda') * 1e-2
        s, tmp = w.clone(), torch.empty(n, device='cuda')
        lr, dec = torch.full((4,), 2e-6, device='cuda'), torch.full((4,), 0.999, device='cuda')

        def plain():
            K.adam_tf(w, g, None, v, 0.0, 0.0, 0.99, 1e-8, 1.0, lr_t_dev=lr)

        def fused():
            K.adam_tf_ema(w, g, None, v, s, 0.0, 0.0, 0.99, 1e-8, 1.0, 0.999, lr_t_dev=lr, ema_decay_dev=dec)

        def two_step():
            plain()
            torch.sub(s, w, out=tmp)
            tmp.mul_(1.0 - 0.999)
            s.sub_(tmp)
        m('adam_ema: t2i_adam_tf beta1=0 m=NULL, %s (3r + 2w)' % arena, (n,), 20 * n, plain)
        m('adam_ema: t2i_adam_tf_ema beta1=0 m=NULL, %s (4r + 3w)' % arena, (n,), 28 * n, fused)
        m('adam_ema: t2i_adam_tf then sub, mul, sub_ by the tensor library, %s (8r + 5w)' % arena, (n,), 52 * n, two_step)

    # Adam with per-slot multipliers at the same two arena sizes, against the launch it stands in for, in the same
    # process: the new launch moves the same bytes, so its time against that launch is the comparison.  The table is the slot layout and the
    # equalized-learning-rate multipliers of the stage-7 (transition) PGGAN generator arena; for the wgancls size the same slot ends are
    # cut off at the arena's size.
    if a.only in 'adam_slots':
        from t2i_amd.models.pggan.pggan import PGGAN
        pg = PGGAN(8, 100, None, None, None, None, None, 7, True, device='cpu', equalized_lr=True)
        ends_pg, mult_pg = pg.G_optimizer.slot_end.tolist(), pg.G_optimizer.slot_mult.tolist()
        del pg
        for n, arena in ((23598252, 'pggan stage 7 g_arena'), (22643292, 'wgancls g_arena')):
            keep = [i for i, e in enumerate(ends_pg) if e < n]
            ends = [ends_pg[i] for i in keep] + [n]
            mult = [mult_pg[i] for i in keep] + [mult_pg[len(keep)] if len(keep) < len(mult_pg) else [1.0, 1.0]]
            slot_end = torch.tensor(ends, dtype=torch.int64, device='cuda')
            slot_mult = torch.tensor(mult, dtype=torch.float32, device='cuda')
            w, g, v = torch.randn(n, device='cuda') * 0.05, torch.randn(n, device='cuda'), torch.rand(n, device='cuda') * 1e-2
            s = w.clone()
            lr, dec = torch.full((4,), 2e-6, device='cuda'), torch.full((4,), 0.999, device='cuda')
            tag = '%s, %d slots' % (arena, len(ends))
            m('adam_slots: t2i_adam_tf beta1=0 m=NULL, %s (3r + 2w)' % arena, (n,), 20 * n,
              lambda: K.adam_tf(w, g, None, v, 0.0, 0.0, 0.99, 1e-8, 1.0, lr_t_dev=lr))
            m('adam_slots: t2i_adam_tf_slots beta1=0 m=NULL, %s (3r + 2w)' % tag, (n,), 20 * n,
              lambda: K.adam_tf_slots(w, g, None, v, slot_end, slot_mult, 0.0, 0.0, 0.99, 1e-8, 1.0, lr_t_dev=lr))
            m('adam_slots: t2i_adam_tf_ema beta1=0 m=NULL, %s (4r + 3w)' % arena, (n,), 28 * n,
              lambda: K.adam_tf_ema(w, g, None, v, s, 0.0, 0.0, 0.99, 1e-8, 1.0, 0.999, lr_t_dev=lr, ema_decay_dev=dec))
            m('adam_slots: t2i_adam_tf_slots + shadow beta1=0 m=NULL, %s (4r + 3w)' % tag, (n,), 28 * n,
              lambda: K.adam_tf_slots(w, g, None, v, slot_end, slot_mult, 0.0, 0.0, 0.99, 1e-8, 1.0, ema=s, ema_decay=0.999, lr_t_dev=lr,
                                      ema_decay_dev=dec))

    # differentiable augmentation at the PGGAN trainer's shapes, the 3B-row critic pass of stages 3, 5 and 7 (batch
    # 16, 16, 8), policy 'color,translation,cutout': the partial-sum pass reads the tensor, the apply kernel reads it again and writes it
    # (2r + w).  Next to each line: the same policy from tensor-library calls on the same table (for the adjoint, autograd's backward of that
    # composition on a retained graph), checked against the kernels before anything is timed.
    if a.only in 'diff_augment' or 'diff_augment' in a.only:
        from t2i_amd.utils import ops
        for shape in ((48, 16, 16, 3), (48, 64, 64, 3), (24, 256, 256, 3)):
            x = torch.randn(shape, device='cuda')
            g = torch.randn(shape, device='cuda')
            P = ops.diff_augment_params(shape[0], shape[1], shape[2], device='cuda')
            n = x.numel()
            xr = x.clone().requires_grad_(True)
            yr = composed_diff_augment(xr, P)
            back = lambda: torch.autograd.grad(yr, xr, g, retain_graph=True)
            assert float((K.diff_augment_fwd(x, P, 7) - yr.detach()).abs().max()) <= 1e-4
            assert float((K.diff_augment_adj(g, P, 7) - back()[0]).abs().max()) <= 1e-4
            with torch.no_grad():
                m2 = lambda name, fn, comp: measure(name, shape, 12 * n, fn, a.reps, a.iters, comp) if a.only in name else None
                m2('diff_augment_fwd color,translation,cutout (2r + w)', lambda: K.diff_augment_fwd(x, P, 7), lambda: composed_diff_augment(x, P))
            m2('diff_augment_adj color,translation,cutout (2r + w)', lambda: K.diff_augment_adj(g, P, 7), back)
            m('diff_augment_fwd translation,cutout, one launch (r + w)', shape, 8 * n, lambda: K.diff_augment_fwd(x, P, 6))

    # the parameter table drawn on the device: one launch of the sampler against diff_augment_params(out=) — the
    # tensor library's fifteen or so launches — into the same buffer, at the PGGAN trainer's two table heights (4B rows, B = 16 and 64)
    if a.only in 'diff_augment_draw' or 'diff_augment_draw' in a.only:
        from t2i_amd.utils import ops
        for rows, size in ((64, 16), (256, 64)):
            out = torch.empty(rows, 9, device='cuda')
            s = ops.DiffAugmentSampler('color,translation,cutout', p=1.0, device='cuda')
            measure('diff_augment_draw color,translation,cutout p=1 (w)', (rows, 9), 36 * rows, lambda: s.draw(rows, size, size, out=out),
                    a.reps, a.iters, lambda: ops.diff_augment_params(rows, size, size, out=out))

    # spectral normalisation in the critic's optimizer step at the critic arenas of PGGAN stages 3 and 7:
    # AdamTF.apply() as it is (one launch, 3r + 2w), with spectral= (the gradient transform, Adam on raw, one power iteration and the
    # rewrite of the arena: seven launches) and the six extra launches alone.  Bytes, per element of a normalised slot (nearly the whole
    # arena): the dot pass reads G and W, the correction reads and writes G, the row pass reads raw (its second pass over an item is served
    # from cache), the rewrite reads raw and writes the arena: 7 more streams, 28 bytes.  The filter cache is left out (refresh=False).
    # The gradient arena is transformed in place call after call, so its values drift towards 0: no kernel here takes a value-dependent path.
    if a.only and a.only in 'spectral_norm':
        from t2i_amd import optim
        from t2i_amd.models.pggan.pggan import PGGAN
        for stage, batch in ((3, 16), (7, 8)):
            pg = PGGAN(batch, 100, None, None, None, None, None, stage, False, device=torch.device('cuda'))
            arena = pg.d_arena
            names = pg.kernel_names(pg.d_vars)
            sn = optim.SpectralNorm(arena, names)
            plain, spec = optim.AdamTF(arena, 0.0, 0.99), optim.AdamTF(arena, 0.0, 0.99, spectral=sn)
            arena.grad.normal_()
            for o in (plain, spec):
                o.prepare(2e-6)
            n = arena.numel
            tag = 'pggan stage %d d_arena, %d of %d variables normalised' % (stage, len(names), len(arena.names))
            m('spectral_norm: AdamTF.apply(), %s (3r + 2w)' % tag, (n,), 20 * n, lambda: plain.apply(refresh=False))
            m('spectral_norm: AdamTF(spectral=).apply(), 7 launches, %s (8r + 4w)' % tag, (n,), 48 * n, lambda: spec.apply(refresh=False))
            m('spectral_norm: grad_() + normalize(1) alone, 6 launches, %s (5r + 2w)' % tag, (n,), 28 * n, lambda: (sn.grad_(), sn.normalize(1)))
            del pg, arena, sn, plain, spec

    # anti-aliased resampling with the taps (1, 3, 3, 1) at fp32 and the trainer's full widths: the generator's
    # upsample at stages 3, 5, 7 ([B, S/2, S/2, nf], B = 16 / 16 / 8), the critic's downsample at the same stages with its 3B rows, and the
    # C = 3 pair of the fade-in branches at stage 7.  Bytes: |x| + |y|.  Next to each line: t2i_upscale2 / t2i_pool2_sum on the same
    # tensors (what the option replaces) and the tensor-library composition on channels-last views, checked against the kernel first.
    if a.only and a.only in 'upfirdn':
        from t2i_amd.utils import ops
        k = (1.0, 3.0, 3.0, 1.0)
        up_taps, down_taps = tuple(2.0 * t / 8.0 for t in k), tuple(t / 8.0 for t in k)
        rows = [('upsample_2d', 'generator stage %d' % s, shape) for s, shape in ((3, (16, 8, 8, 512)), (5, (16, 32, 32, 512)), (7, (8, 128, 128, 128)))]
        rows += [('downsample_2d', 'critic stage %d, 3B rows' % s, shape) for s, shape in ((3, (48, 16, 16, 512)), (5, (48, 64, 64, 256)), (7, (24, 256, 256, 64)))]
        rows += [('upsample_2d', 'generator fade-in, stage 7', (8, 128, 128, 3)), ('downsample_2d', 'critic fade-in, stage 7, 3B rows', (24, 256, 256, 3))]
        with torch.no_grad():
            for kind, where, shape in rows:
                x = torch.randn(shape, device='cuda')
                xc = x.permute(0, 3, 1, 2)                       # the same memory as a channels-last NCHW tensor
                if kind == 'upsample_2d':
                    fn, base, comp = (lambda: K.upfirdn2d(x, up_taps, 2, 1, 2, 1, False)), (lambda: K.upscale2(x, 1.0)), (lambda: composed_upfirdn(xc, up_taps, 2, 1, 2, 1))
                    label, out = 'upscale2', 4 * x.numel()
                else:
                    fn, base, comp = (lambda: K.upfirdn2d(x, down_taps, 1, 2, 1, 1, False)), (lambda: K.pool2_sum(x, 0.25)), (lambda: composed_upfirdn(xc, down_taps, 1, 2, 1, 1))
                    label, out = 'pool2_sum', x.numel() // 4
                err = float((fn().permute(0, 3, 1, 2) - comp()).abs().max())
                assert err <= 1e-4 and torch.equal(fn(), getattr(ops, kind)(x, k)), (kind, shape, err)      # the helper's launch, called as upscale2 / pool2_sum are
                measure('upfirdn: %s (1,3,3,1), %s (r + w)' % (kind, where), shape, 4 * (x.numel() + out), fn, a.reps, a.iters, comp, {label: base})
                del x, xc

    # the style layer at the generator's B = 8 shapes, relu and noise as the model runs it: each entry alone, the
    # forward (3 launches) and the backward (4 launches) as the autograd Function issues them, and layer_norm(act=relu) forward and
    # backward on the same tensors (what the layer replaces) with one r + w pass standing in for a separate noise add.  Bytes: the passes
    # over the [B,H,W,C] tensors each line makes (stats r, apply r + w, bwd_sums 2r, bwd_apply 2r + w); layer_norm's lines are charged the
    # same bytes as the adain line they stand next to, so the two ratios compare directly.
    if a.only and a.only in 'adain':
        from t2i_amd import autograd as A
        from t2i_amd._lib import check, lib
        with torch.no_grad():
            for shape in ((8, 4, 4, 512), (8, 16, 16, 512), (8, 64, 64, 128), (8, 256, 256, 64)):
                B, H, W, C = shape
                R, n = H * W, B * H * W * C
                x, g = torch.randn(shape, device='cuda'), torch.randn(shape, device='cuda')
                nz, st = torch.randn((B, H, W), device='cuda'), torch.rand(C, device='cuda') - 0.5
                sty = torch.randn((B, 2 * C), device='cuda') * 0.3
                ys, yb = sty[:, :C], sty[:, C:]
                y, mean, rstd = K.adain_fwd(x, ys, yb, nz, st, K.ACT_RELU, 0.0)
                dx, ds, dys, dyb = K.adain_bwd(g, x, ys, mean, rstd, nz, st, K.ACT_RELU, 0.0)
                wsp, wsn = K._ws_args(x, int(lib.t2i_adain_workspace_bytes(B, R, C)))
                p, sm = K._ptr, K._stream
                one = lambda name, nbytes, fn, launches: measure('adain: ' + name, shape, nbytes, fn, a.reps, a.iters, extra={'launches': launches})
                one('t2i_adain_stats relu + noise (r)', 4 * n, lambda: check(lib.t2i_adain_stats(p(x), p(nz), p(st), B, R, C, K.ACT_RELU, 0.0, 1e-8,
                    p(mean), p(rstd), wsp, wsn, sm())), 2)
                one('t2i_adain_apply relu + noise (r + w)', 8 * n, lambda: check(lib.t2i_adain_apply(p(x), p(nz), p(st), p(mean), p(rstd), p(ys), p(yb),
                    2 * C, B, R, C, K.ACT_RELU, 0.0, p(y), sm())), 1)
                one('forward = stats + apply (2r + w)', 12 * n, lambda: K.adain_fwd(x, ys, yb, nz, st, K.ACT_RELU, 0.0), 3)
                one('t2i_adain_bwd_sums relu + noise (2r)', 8 * n, lambda: check(lib.t2i_adain_bwd_sums(p(g), p(x), p(nz), p(st), p(mean), p(rstd),
                    B, R, C, K.ACT_RELU, 0.0, p(dys), p(dyb), wsp, wsn, sm())), 2)
                one('t2i_adain_bwd_apply relu + noise + dstrength (2r + w)', 12 * n, lambda: check(lib.t2i_adain_bwd_apply(p(g), p(x), p(nz), p(st),
                    p(mean), p(rstd), p(ys), 2 * C, p(dys), p(dyb), B, R, C, K.ACT_RELU, 0.0, p(dx), p(ds), wsp, wsn, sm())), 2)
                one('backward = bwd_sums + bwd_apply (4r + w)', 20 * n, lambda: K.adain_bwd(g, x, ys, mean, rstd, nz, st, K.ACT_RELU, 0.0), 4)
                gamma, beta = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda') * 0.1
                one('layer_norm relu forward, same tensors (charged 2r + w)', 12 * n, lambda: A.LayerNormFn.apply(x, gamma, beta, 1e-12, K.ACT_RELU, 0.0), 3)
                s1, s2 = K.row_moments(x)
                lmean = s1 / (R * C)
                lrstd = torch.rsqrt(torch.clamp(s2 / (R * C) - lmean * lmean, min=0.0) + 1e-12)
                xhat = K.row_fma2(x, lrstd, delta=-lmean * lrstd)
                yl = K.bn_apply(xhat, gamma, beta, K.ACT_RELU, 0.0)
                one('layer_norm relu backward, same tensors (charged 4r + w)', 20 * n,
                    lambda: A.LayerNormBwdFn.apply(g, x, gamma, xhat, lrstd, yl, K.ACT_RELU, 0.0, R * C, True), 5)
                one('a separate noise add stood in for by bn_apply (r + w)', 8 * n, lambda: K.bn_apply(x, gamma, beta, K.ACT_NONE, 0.0), 1)
                del x, g, y, dx, xhat, yl

    # the weight-demodulated convolution's launches around its convolution at the same four shapes, Cin = Cout,
    # relu + noise: each call alone, the layer's non-convolution launches together forward (coef + modulate + epilogue) and backward
    # (epilogue + scale gradient + input adjoint + coef, as the autograd Functions issue them), and in the same run the adain forward /
    # backward and t2i_adain_apply at the shape: the path they replace and the plain r + w pass the two new ones are compared with.
    # Bytes: the passes over the [B,H,W,C] tensors (modulate r + w; bwd_scale 2r; demod_act r + w; its backward 2r + w); the coefficient
    # calls are charged their passes over the filter (coef: r of W; its backward: r of W + w of dW).
    if a.only and a.only in 'modconv':
        from t2i_amd._lib import check, lib
        with torch.no_grad():
            for shape in ((8, 4, 4, 512), (8, 16, 16, 512), (8, 64, 64, 128), (8, 256, 256, 64)):
                B, H, W, C = shape
                R, n, nw = H * W, B * H * W * C, 9 * C * C
                x, g, c = (torch.randn(shape, device='cuda') for _ in range(3))
                nz, st, bias = torch.randn((B, H, W), device='cuda'), torch.rand(C, device='cuda') - 0.5, torch.randn(C, device='cuda') * 0.1
                s, gd = 1.0 + 0.3 * torch.randn((B, C), device='cuda'), torch.randn((B, C), device='cuda')
                w = torch.randn((3, 3, C, C), device='cuda') * (2.0 / (9 * C)) ** 0.5
                d, q = K.demod_coef(w, s)
                one = lambda name, nbytes, fn, launches: measure('modconv: ' + name, shape, nbytes, fn, a.reps, a.iters, extra={'launches': launches})
                one('t2i_demod_coef (r of W)', 4 * nw, lambda: K.demod_coef(w, s), 2)
                one('t2i_demod_coef_bwd ds + dW (r + w of W)', 8 * nw, lambda: K.demod_coef_bwd(gd, d, w, s, q), 2)
                one('t2i_modulate (r + w)', 8 * n, lambda: K.modulate(x, s), 1)
                one('t2i_modulate_bwd_scale (2r)', 8 * n, lambda: K.modulate_bwd_scale(g, x), 2)
                one('t2i_demod_act relu + noise (r + w)', 8 * n, lambda: K.demod_act(c, d, bias, nz, st, K.ACT_RELU, 0.0), 1)
                one('t2i_demod_act_bwd relu + noise, every sum (2r + w)', 12 * n, lambda: K.demod_act_bwd(g, c, d, bias, nz, st, K.ACT_RELU, 0.0), 2)

                def fwd():
                    dd, _ = K.demod_coef(w, s)
                    K.modulate(x, s)
                    K.demod_act(c, dd, bias, nz, st, K.ACT_RELU, 0.0)

                def bwd():
                    K.demod_act_bwd(g, c, d, bias, nz, st, K.ACT_RELU, 0.0)
                    K.demod_coef_bwd(gd, d, w, s, q)
                    K.modulate(g, s)
                    K.modulate_bwd_scale(g, x)
                one('layer forward without its convolution = coef + modulate + demod_act (2r + 2w, r of W)', 16 * n + 4 * nw, fwd, 4)
                one('layer backward without its convolutions = demod_act_bwd + coef_bwd + modulate + bwd_scale (5r + 2w, r + w of W)',
                    28 * n + 8 * nw, bwd, 7)
                sty = torch.randn((B, 2 * C), device='cuda') * 0.3
                ys, yb = sty[:, :C], sty[:, C:]
                y, mean, rstd = K.adain_fwd(x, ys, yb, nz, st, K.ACT_RELU, 0.0)
                p, sm = K._ptr, K._stream
                one('t2i_adain_apply relu + noise, same run (r + w)', 8 * n, lambda: check(lib.t2i_adain_apply(p(x), p(nz), p(st), p(mean), p(rstd),
                    p(ys), p(yb), 2 * C, B, R, C, K.ACT_RELU, 0.0, p(y), sm())), 1)
                one('adain forward, same run (2r + w)', 12 * n, lambda: K.adain_fwd(x, ys, yb, nz, st, K.ACT_RELU, 0.0), 3)
                one('adain backward, same run (4r + w)', 20 * n, lambda: K.adain_bwd(g, x, ys, mean, rstd, nz, st, K.ACT_RELU, 0.0), 4)
                del x, g, c, y

    # the second-order launches of the weight-demodulated convolution at the same four shapes with B = 4 (the
    # regulariser runs on half a batch of 8), relu + noise, every cotangent and every output: each next to a device copy of the same bytes
    # and next to the same result from tensor-library calls, in the same alternating rounds.  Bytes: the passes over the [B,H,W,C]
    # tensors (demod_act_bwd2: g, c, vc read, gg, gc written; modulate2: vx, x read, gg written) and over the filter (coef_bwd2: r + w).
    if a.only == 'modconv2':
        with torch.no_grad():
            for shape in ((4, 4, 4, 512), (4, 16, 16, 512), (4, 64, 64, 128), (4, 256, 256, 64)):
                B, H, W, C = shape
                n, nw = B * H * W * C, 9 * C * C
                x, g, c, vc, vx = (torch.randn(shape, device='cuda') for _ in range(5))
                nz, st, bias = torch.randn((B, H, W), device='cuda'), torch.rand(C, device='cuda') - 0.5, torch.randn(C, device='cuda') * 0.1
                s, gd, vd, vs = (torch.randn((B, C), device='cuda') for _ in range(4))
                s = 1.0 + 0.3 * s
                w = torch.randn((3, 3, C, C), device='cuda') * (2.0 / (9 * C)) ** 0.5
                d, q = K.demod_coef(w, s)
                row = lambda t: t[:, None, None, :]

                def act2_composed():
                    m = ((row(d) * c + bias + st * nz[..., None]) > 0).to(c.dtype)
                    mg = m * g
                    return m * (row(d) * vc + c * row(vd)), mg * row(vd), (mg * vc).sum((1, 2))

                def coef2_composed():
                    vss = vs * s
                    r = vss @ q
                    return -(d ** 3) * r, -3.0 * d * d * gd * r, 4.0 * w * (vss.t() @ (-0.5 * d ** 3 * gd))
                one = lambda name, nbytes, fn, launches, composed: measure('modconv2: ' + name, shape, nbytes, fn, a.reps, a.iters, composed=composed,
                                                                         extra={'launches': launches})
                one('t2i_demod_act_bwd2 relu + noise, vc + vd -> gg, gc, gd (3r + 2w)', 20 * n,
                    lambda: K.demod_act_bwd2(g, c, d, bias, nz, st, vc, vd, K.ACT_RELU, 0.0), 2, act2_composed)
                one('t2i_modulate2 vx + vs -> gg (2r + w)', 12 * n, lambda: K.modulate2(s, vx, x, vs), 1, lambda: row(s) * vx + x * row(vs))
                one('t2i_demod_coef_bwd2 -> gg_d, gd_d, dW (r + w of W)', 8 * nw, lambda: K.demod_coef_bwd2(vs, gd, d, w, s, q), 2, coef2_composed)
                del x, g, c, vc, vx


if __name__ == '__main__':
    main()
