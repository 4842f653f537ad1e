#!/usr/bin/env python
"""The InceptionV3 fine-tuning step (models/inception/train_net.py) on one GPU at the reference's batch, B = 64, with random
He-scaled weights.  Prints one JSON line:
  steps_per_s, images_per_s   of the whole training step (device events over --iters steps after --warmup)
  ms_per_step                 and its split, from events at the phase boundaries of one more step: trunk forward
                              (Conv2d_1a .. Mixed_7b), Mixed_7c + head forward / backward, optimizer
  launches_per_step           kernel launches of one step, counted by the torch profiler when available (else null)
  eval_fwd_ms                 the evaluator's inference forward (model.InceptionV3) at the same B in the same process, and
  step_over_eval              the ratio of the two."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd.models.inception import model as M  # noqa: E402
from t2i_amd.models.inception.train_net import InceptionTrainNet  # noqa: E402
from bench_inception import random_weights, timed  # noqa: E402


def phase_split(net, images, labels, counter):
    marks = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))
    mark('trunk')
    net.step(images, labels, counter, mark=mark)
    mark('end')
    torch.cuda.synchronize()
    t = {}
    for (name, a), (_, b) in zip(marks, marks[1:]):
        t[name] = t.get(name, 0.0) + a.elapsed_time(b)
    return {'trunk_fwd': t.get('trunk', 0.0), 'mixed_7c_head_fwd_bwd': t.get('mixed_7c', 0.0) + t.get('backward', 0.0),
            'optimizer': t.get('optimizer', 0.0)}


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower())
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    B, C = args.batch, args.classes
    arrays = random_weights(C)
    rng = np.random.default_rng(1)
    images = torch.from_numpy(rng.uniform(-1, 1, (B, 299, 299, 3)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rng.integers(0, C, B).astype(np.int32)).to(dev)
    net = InceptionTrainNet(arrays, C, dev)
    step = [0]

    def one():
        step[0] += 1
        net.step(images, labels, step[0])
    sec = timed(one, args.iters, args.warmup)
    split = phase_split(net, images, labels, 10 ** 6)
    launches = count_launches(one)
    evaluator = M.InceptionV3.from_arrays(arrays, C, dev)
    eval_sec = timed(lambda: evaluator(images), args.iters, args.warmup)
    print(json.dumps({'bench': 'incep_train_step', 'batch': B, 'classes': C, 'steps_per_s': round(1.0 / sec, 2),
                      'images_per_s': round(B / sec, 1), 'ms_per_step': round(sec * 1e3, 3),
                      'ms_split': {k: round(v, 3) for k, v in split.items()}, 'launches_per_step': launches,
                      'eval_fwd_ms': round(eval_sec * 1e3, 3), 'step_over_eval': round(sec / eval_sec, 3)}))


if __name__ == '__main__':
    main()
