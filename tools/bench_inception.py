#!/usr/bin/env python
"""The evaluator's hot path on one GPU, with random He-scaled InceptionV3 weights and identity batch norm (so every
pre-activation keeps about unit variance through the network).  One JSON line per row:
  inception_fwd   per batch size (64, then 256): images/s of the forward after warm-up (device events over --iters calls),
                  multiply-adds per image from the layer table, TFLOP/s (2 x multiply-adds) and the fraction of the 157.3 TFLOP/s
                  fp32 matrix peak; the forward's time split into convolutions and the evaluator kernels (events before every
                  launch, one extra pass).
  resize          t2i_resample_bilinear of a gathered batch of 64 fp32 64x64 generator images to 299 x 299.
  gram            t2i_gram_accumulate of 64 rows at d = 2048.
  is_scoring      get_inception_score over --size generator images resident on the device (shuffle, gather + resize,
                  forward, softmax, 10 splits); the generator's own time is not included.
With --layers, one more line per convolution at B = 64 (time, TFLOP/s), in the style of tools/bench_conv.py."""
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

PEAK_F32_MATRIX = 157.3e12


def random_weights(num_classes=20, seed=0):
    rng = np.random.default_rng(seed)
    arrays = {}
    for k, shape in M.variable_shapes(num_classes).items():
        if k.endswith('weights'):
            arrays[k] = (rng.standard_normal(shape) * np.sqrt(2.0 / np.prod(shape[:3]))).astype(np.float32)
        elif k.endswith('moving_variance'):
            arrays[k] = np.full(shape, 1.0 - 0.001, np.float32)
        else:
            arrays[k] = np.zeros(shape, np.float32)
    return arrays


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e-3          # seconds per call


def split(net, x):
    """(conv seconds, other seconds) of one forward: an event before every launch, the gap to the next one is that launch's."""
    marks = []

    def tick(kind):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((kind, e))
    net(x, timer=tick)
    end = torch.cuda.Event(enable_timing=True)
    end.record()
    end.synchronize()
    out = {'conv': 0.0, 'other': 0.0}
    for (kind, e), (_, nxt) in zip(marks, marks[1:] + [(None, end)]):
        out[kind] += e.elapsed_time(nxt) * 1e-3
    return out['conv'], out['other']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,256')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--size', type=int, default=50000, help='images scored by the is_scoring row (0: skip it)')
    ap.add_argument('--layers', action='store_true', help='also time every convolution at B = 64')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_inception.py needs a GPU')
    dev = torch.device('cuda')
    net = M.InceptionV3.from_arrays(random_weights(), 20, dev)
    macs = M.multiply_adds(20)
    rng = np.random.default_rng(1)
    for B in [int(b) for b in args.batches.split(',')]:
        x = torch.from_numpy(rng.uniform(-1, 1, (B, 299, 299, 3)).astype(np.float32)).to(dev)
        try:
            sec = timed(lambda: net(x), args.iters)
        except (RuntimeError, MemoryError) as e:          # a batch that does not fit is reported, not fatal
            print(json.dumps({'row': 'inception_fwd', 'batch': B, 'error': str(e)[:200]}), flush=True)
            continue
        conv_s, other_s = split(net, x)
        tflops = 2 * macs * B / sec / 1e12
        print(json.dumps({'row': 'inception_fwd', 'batch': B, 'ms_per_batch': round(sec * 1e3, 3), 'images_per_s': round(B / sec, 1),
                          'macs_per_image': macs, 'tflops': round(tflops, 2), 'frac_f32_matrix_peak': round(tflops * 1e12 / PEAK_F32_MATRIX, 3),
                          'split_ms': {'conv': round(conv_s * 1e3, 3), 'eval_kernels': round(other_s * 1e3, 3)}}), flush=True)
        del x
    if args.layers:
        B = 64
        for name, (kh, kw, cin, cout, s, pad, Ho, Wo, bn) in M.layer_table(20).items():
            H = Ho * s if pad == 'SAME' else (Ho - 1) * s + kh
            W = Wo * s if pad == 'SAME' else (Wo - 1) * s + kw
            xi = torch.randn(B, H, W, cin, device=dev)
            w, b = net.params[name]
            d, ws = K.conv_desc(B, H, W, cin, cout, kh, kw, s, s, pad, math=K.MATH_F32)
            sec = timed(lambda: K.conv_fwd(xi, w, b, d, ws, act=K.ACT_RELU), 10)
            fl = 2.0 * B * Ho * Wo * kh * kw * cin * cout
            print(json.dumps({'row': 'conv_layer', 'name': name, 'shape': [B, H, W, cin, cout, kh, kw, s, pad],
                              'us': round(sec * 1e6, 1), 'tflops': round(fl / sec / 1e12, 2), 'algo': K.conv_algo(d, 'fwd')}), flush=True)
    # resize: 64 gathered 64x64 fp32 images -> 299 x 299
    store = torch.from_numpy(np.tanh(rng.standard_normal((1000, 64, 64, 3))).astype(np.float32)).to(dev)
    rows = torch.from_numpy(rng.permutation(1000)[:64].astype(np.int32)).to(dev)
    sec = timed(lambda: K.resample_bilinear(store, 299, 299, rows=rows), 50)
    moved = 64 * (64 * 64 * 3 * 4 + 299 * 299 * 3 * 4 + 2 * 64 * 299 * 3)
    print(json.dumps({'row': 'resize', 'batch': 64, 'us': round(sec * 1e6, 1), 'gb_per_s': round(moved / sec / 1e9, 1)}), flush=True)
    # gram: 64 rows at d = 2048
    acts = torch.rand(64, 2048, device=dev)
    s0 = torch.zeros(2048, device=dev)
    sm, G = torch.zeros(2048, dtype=torch.float64, device=dev), torch.zeros(2048, 2048, dtype=torch.float64, device=dev)
    sec = timed(lambda: K.gram_accumulate(acts, s0, sm, G), 50)
    print(json.dumps({'row': 'gram', 'n': 64, 'd': 2048, 'us': round(sec * 1e6, 1),
                      'tflops': round(2.0 * 64 * 2048 * 2048 / sec / 1e12, 2)}), flush=True)
    if args.size:
        from t2i_amd.evaluation.inception_score import get_inception_score
        del store
        gen = torch.empty((args.size, 64, 64, 3), dtype=torch.float32, device=dev)
        for i in range(0, args.size, 1000):
            n = min(1000, args.size - i)
            gen[i:i + n].copy_(torch.from_numpy(np.tanh(rng.standard_normal((n, 64, 64, 3))).astype(np.float32)))
        np.random.seed(0)
        torch.cuda.synchronize()
        t0 = time.time()
        mean, std, _ = get_inception_score(gen, net, 64, 10)
        torch.cuda.synchronize()
        el = time.time() - t0
        print(json.dumps({'row': 'is_scoring', 'images': args.size, 'incep_batch': 64, 'seconds': round(el, 2),
                          'images_per_s': round(args.size / el, 1), 'is_mean': round(mean, 4), 'is_std': round(std, 4)}), flush=True)


if __name__ == '__main__':
    main()
