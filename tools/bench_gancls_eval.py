#!/usr/bin/env python
"""GAN-CLS eval-mode generator and IS scoring on one GPU, at full width (flowers yml: Z 100, embeddings 1024, GF 128) with random
weights and random He-scaled InceptionV3 weights.  One JSON line:
  generator       per batch size (8, 64, 1000): the eval-mode generator pass on the unfused norm path (ops.batch_norm(train=False): [C]
                  vector math in tensor-library launches + t2i_bn_apply, a launch of its own for each bottleneck's closing add) and on
                  the fused path (t2i_bn_infer, one launch per norm) — ms per pass (median of --repeats regions of --iters passes, device
                  events, after a warm-up; both paths in this process, alternating) and kernel launches per pass;
  scoring         the IS path of eval_gancls.py at SAMPLE_SIZE 1000 / Inception batch 64: generator (fused) -> per Inception batch,
                  t2i_resample_bilinear 64 -> 299 from the fp32 store -> Inception forward; images/s of the whole step and of each
                  part timed alone."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.models.gancls.model import GanCls  # noqa: E402
from t2i_amd.models.inception import model as M  # noqa: E402
from t2i_amd.utils.config import config_from_yaml  # noqa: E402
from bench_incep_train import count_launches  # noqa: E402
from bench_inception import random_weights, timed  # noqa: E402

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'text-to-image_amd', 'models', 'gancls', 'cfg', 'flowers.yml')


def median_ms(fn, iters, repeats, warmup=3):
    timed(fn, 1, warmup)
    return statistics.median(timed(fn, iters, 0) for _ in range(repeats)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 64, 1000])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sample-size', type=int, default=1000, help='EVAL.SAMPLE_SIZE')
    ap.add_argument('--incep-batch', type=int, default=64, help='EVAL.INCEP_BATCH_SIZE')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_gancls_eval.py needs a GPU')
    dev = torch.device('cuda', 0)
    cfg = config_from_yaml(CFG)
    m = GanCls(cfg, device=dev)                           # every variable, random initial values
    with torch.no_grad():                                 # moving statistics that are not the identity
        for n, v in m.store.vars.items():
            if n.endswith('moving_mean'):
                v.normal_(0.0, 0.1)
            elif n.endswith('moving_variance'):
                v.uniform_(0.5, 1.5)
    g = torch.Generator(device=dev).manual_seed(0)

    def gen_fn(B, fused):
        z = torch.randn((B, m.z_dim), generator=g, device=dev)
        phi = torch.randn((B, m.embed_dim), generator=g, device=dev)

        def fn():
            m.fused_infer = fused
            return m.sampler(z, phi)
        return fn

    rows = {}
    for B in args.batches:
        old, new = gen_fn(B, False), gen_fn(B, True)
        t_old, t_new = [], []
        timed(old, 1, 3); timed(new, 1, 3)
        for _ in range(args.repeats):                     # alternating regions: drift of the clocks lands on both paths
            t_old.append(timed(old, args.iters, 0))
            t_new.append(timed(new, args.iters, 0))
        rows['B%d' % B] = {'unfused_ms': round(statistics.median(t_old) * 1e3, 4), 'fused_ms': round(statistics.median(t_new) * 1e3, 4),
                           'unfused_launches': count_launches(old), 'fused_launches': count_launches(new)}
        rows['B%d' % B]['speedup'] = round(rows['B%d' % B]['unfused_ms'] / rows['B%d' % B]['fused_ms'], 3)

    # ---- IS scoring at SAMPLE_SIZE / Inception batch ----
    S, c = args.sample_size, args.incep_batch
    net = M.InceptionV3.from_arrays(random_weights(20), 20, dev)
    gen = gen_fn(S, True)
    store = gen().float().contiguous()
    n_chunks = S // c
    idx = [torch.arange(i * c, (i + 1) * c, dtype=torch.int32, device=dev) for i in range(n_chunks)]
    x = torch.empty((c, M.IMAGE_SIZE, M.IMAGE_SIZE, 3), dtype=torch.float32, device=dev)

    def resize():
        for r in idx:
            K.resample_bilinear(store, M.IMAGE_SIZE, M.IMAGE_SIZE, rows=r, out=x)

    def incep():
        with torch.no_grad():
            for _ in idx:
                net(x)

    def step():
        s = gen().float().contiguous()
        with torch.no_grad():
            for r in idx:
                net(K.resample_bilinear(s, M.IMAGE_SIZE, M.IMAGE_SIZE, rows=r, out=x))
    it = max(args.iters // 3, 2)
    t_step, t_gen = median_ms(step, it, args.repeats, 1), median_ms(gen, it, args.repeats, 1)
    t_res, t_inc = median_ms(resize, it, args.repeats, 1), median_ms(incep, it, args.repeats, 1)
    scored = n_chunks * c
    print(json.dumps({'bench': 'gancls_eval', 'generator': rows,
                      'scoring': {'sample_size': S, 'incep_batch': c, 'images_per_s': round(scored / t_step * 1e3, 1), 'step_ms': round(t_step, 3),
                                  'split_ms': {'generator': round(t_gen, 3), 'resize': round(t_res, 3), 'inception': round(t_inc, 3)},
                                  'split_images_per_s': {'generator': round(S / t_gen * 1e3, 1), 'resize': round(scored / t_res * 1e3, 1),
                                                         'inception': round(scored / t_inc * 1e3, 1)}}}), flush=True)


if __name__ == '__main__':
    main()
