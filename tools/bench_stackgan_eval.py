#!/usr/bin/env python
"""StackGAN Stage-II scoring on one GPU, at full width (flowers yml: Z 100, embeddings 1024, GF 128) with random weights and
random He-scaled InceptionV3 weights, at the Stage-II yml's batch B = 32.  One JSON line:
  images_per_s    a whole scoring step per batch (the IS path of eval_stageii.py): Stage-I generator -> Stage-II generator (eval
                  mode) -> t2i_resample_bilinear 256 -> 299 from the fp32 store -> Inception forward, over --iters batches;
  split_ms        the same step's device time per batch in four parts: the two generators, the resize, Inception, and the IMD
                  cosine kernel over the batch's B pairs (the IMD path's extra launch);
  cosine_us       t2i_cosine_distance alone at n = 64 pairs, d = 2048 (device events over 100 calls)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.models.inception import model as M  # noqa: E402
from t2i_amd.models.stackgan.stageI.model import ConditionalGan as S1  # noqa: E402
from t2i_amd.models.stackgan.stageII.model import ConditionalGan as S2  # noqa: E402
from t2i_amd.utils.config import config_from_yaml  # noqa: E402
from bench_inception import random_weights, timed  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, '..', 'text-to-image_amd', 'models', 'stackgan')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32, help='EVAL.SAMPLE_SIZE (the Stage-II yml: 32)')
    ap.add_argument('--iters', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_stackgan_eval.py needs a GPU')
    dev = torch.device('cuda', 0)
    B = args.batch
    c1 = config_from_yaml(os.path.join(CFG, 'stageI', 'cfg', 'flowers.yml'))
    c2 = config_from_yaml(os.path.join(CFG, 'stageII', 'cfg', 'flowers.yml'))
    c1.TRAIN.BATCH_SIZE = c2.TRAIN.BATCH_SIZE = B
    s2 = S2(S1(c1, build_model=False, device=dev), c2)           # every variable, random initial values
    net = M.InceptionV3.from_arrays(random_weights(20), 20, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn((B, s2.stagei.z_dim), generator=g, device=dev)
    phi = torch.randn((B, s2.stagei.embed_dim), generator=g, device=dev)

    def gen():
        with torch.no_grad():
            img64, _, _ = s2.stagei.generator(z, phi, reuse=True, is_training=False)
            return s2.generator(img64, phi, reuse=True, is_training=False)[0].float().contiguous()

    img = gen()
    x = K.resample_bilinear(img, M.IMAGE_SIZE, M.IMAGE_SIZE)
    with torch.no_grad():
        _, pre = net(x)
    pre = pre.reshape(B, -1)
    half = B // 2 if B > 1 else 1

    def step():
        im = gen()
        xx = K.resample_bilinear(im, M.IMAGE_SIZE, M.IMAGE_SIZE)
        with torch.no_grad():
            net(xx)
    t_step = timed(step, args.iters)
    t_gen = timed(gen, args.iters)
    t_resize = timed(lambda: K.resample_bilinear(img, M.IMAGE_SIZE, M.IMAGE_SIZE, out=x), args.iters)

    def fwd():
        with torch.no_grad():
            net(x)
    t_incep = timed(fwd, args.iters)
    t_cos_b = timed(lambda: K.cosine_distance(pre[:half], pre[B - half:]), 100)
    a = torch.randn((64, M.PRELOGITS_DIM), generator=g, device=dev)
    b = torch.randn((64, M.PRELOGITS_DIM), generator=g, device=dev)
    t_cos = timed(lambda: K.cosine_distance(a, b), 100, warmup=10)
    print(json.dumps({'bench': 'stackgan_stageII_scoring', 'batch': B, 'images_per_s': round(B / t_step, 1),
                      'step_ms': round(t_step * 1e3, 3),
                      'split_ms': {'generators': round(t_gen * 1e3, 3), 'resize': round(t_resize * 1e3, 3),
                                   'inception': round(t_incep * 1e3, 3), 'cosine_pairs_%d' % half: round(t_cos_b * 1e3, 4)},
                      'cosine_us': {'n': 64, 'd': M.PRELOGITS_DIM, 'us': round(t_cos * 1e6, 2)}}), flush=True)


if __name__ == '__main__':
    main()
