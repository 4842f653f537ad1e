#!/usr/bin/env python
"""StackGAN's inference chain on one GPU, at full width (flowers yml: Z 100, embeddings 1024, GF 128) with random weights and moving
statistics that are not the identity.  One JSON line:
  generators      the eval-mode Stage-I generator at B = 8 / 64 and the chain Stage I -> Stage II at B = 8 / 32, on the unfused norm
                  path (ops.batch_norm(train=False): [C] vector math in tensor-library launches + t2i_bn_apply, a launch of its own
                  for each residual join — the launch sequence before the fused norms) and on the fused path (t2i_bn_infer, one launch
                  per norm): ms per pass (median of --repeats regions of --iters passes, device events, after a warm-up; both paths in
                  this process, alternating), the spread of each arm's regions, and kernel launches per pass;
  bytescale       kernels.bytescale_nearest on 8 and 64 images of 256 x 256 x 3 -> 128 x 128: us per call and the bytes it moves (the
                  first pass reads every float, the second gathers a quarter of them and writes the bytes);
  visualize       wall time of one StageIIVisualizer.visualize(interp=1) at B = 32 on a synthetic 304 x 304 data set of --images
                  train / test images written to a temporary directory (the special positions moved into that split), checkpoints of
                  the random weights included; PNG encoding and the host copies are part of it."""
import argparse
import json
import os
import pickle
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.models.stackgan.stageI.model import ConditionalGan as S1  # noqa: E402
from t2i_amd.models.stackgan.stageII.model import ConditionalGan as S2  # noqa: E402
from t2i_amd.utils.config import config_from_yaml  # noqa: E402
from bench_incep_train import count_launches  # noqa: E402
from bench_inception import timed  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, '..', 'text-to-image_amd', 'models', 'stackgan')


def build(B, dev):
    c1 = config_from_yaml(os.path.join(CFG, 'stageI', 'cfg', 'flowers.yml'))
    c2 = config_from_yaml(os.path.join(CFG, 'stageII', 'cfg', 'flowers.yml'))
    c1.TRAIN.BATCH_SIZE = c2.TRAIN.BATCH_SIZE = B
    m = S2(S1(c1, build_model=False, device=dev), c2)           # every variable, random initial values
    with torch.no_grad():
        for n, v in m.store.vars.items():
            if n.endswith('moving_mean'):
                v.normal_(0.0, 0.1)
            elif n.endswith('moving_variance'):
                v.uniform_(0.5, 1.5)
    return m, c1, c2


def ab(old, new, iters, repeats):
    """Both arms alternate; -> dict of medians, each arm's spread (max - min of its regions) and launches per pass."""
    t_old, t_new = [], []
    timed(old, 1, 3); timed(new, 1, 3)
    for _ in range(repeats):
        t_old.append(timed(old, iters, 0) * 1e3)
        t_new.append(timed(new, iters, 0) * 1e3)
    row = {'unfused_ms': round(statistics.median(t_old), 4), 'fused_ms': round(statistics.median(t_new), 4),
           'unfused_spread_ms': round(max(t_old) - min(t_old), 4), 'fused_spread_ms': round(max(t_new) - min(t_new), 4),
           'unfused_launches': count_launches(old), 'fused_launches': count_launches(new)}
    row['speedup'] = round(row['unfused_ms'] / row['fused_ms'], 3)
    return row


def write_split(root, split, n, rng, emb_dim):
    import joblib
    path = os.path.join(root, split)
    os.makedirs(path)
    joblib.dump(list(rng.integers(0, 256, (n, 304, 304, 3), dtype=np.uint8)), os.path.join(path, '304images.pickle'))
    pickle.dump(list(rng.standard_normal((n, 5, emb_dim)).astype(np.float32)), open(os.path.join(path, 'char-CNN-RNN-embeddings.pickle'), 'wb'))
    names = ['jpg/%s_%05d' % (split, i) for i in range(n)]
    pickle.dump(names, open(os.path.join(path, 'filenames.pickle'), 'wb'))
    pickle.dump([1] * n, open(os.path.join(path, 'class_info.pickle'), 'wb'))
    for name in names:
        f = os.path.join(root, 'text_c10', 'class_00001', name[len('jpg/'):] + '.txt')
        os.makedirs(os.path.dirname(f), exist_ok=True)
        with open(f, 'w') as fh:
            fh.write('\n'.join('this flower has petals that are yellow and a caption number %d' % k for k in range(5)) + '\n')


def visualize_wall(m, c1, c2, n_images):
    from t2i_amd.models.stackgan.stageI import visualize_stagei as VS
    from t2i_amd.models.stackgan.stageII.visualize_stageii import StageIIVisualizer
    from t2i_amd.models.wgancls.run import load_dataset
    from t2i_amd.utils.saver import Saver, save
    root = tempfile.mkdtemp(prefix='stackgan_infer_bench_')
    try:
        rng = np.random.default_rng(0)
        write_split(root + '/data', 'train', n_images, rng, c2.MODEL.EMBED_DIM)
        write_split(root + '/data', 'test', n_images, rng, c2.MODEL.EMBED_DIM)
        c1.CHECKPOINT_DIR, c2.CHECKPOINT_DIR = root + '/ckpt1/', root + '/ckpt2/'
        c2.DATASET_DIR, c2.SAMPLE_DIR = root + '/data/', root + '/samples/'
        save(Saver(m.store, var_list=['g_net']), None, c1.CHECKPOINT_DIR, 1)
        save(Saver(m.store, var_list=['stageII_g_net']), None, c2.CHECKPOINT_DIR, 1)
        dataset = load_dataset(c2, m.device)
        special, VS.SPECIAL['flowers'] = VS.SPECIAL['flowers'], [n_images - 1, n_images // 2, 0]
        try:
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = StageIIVisualizer(None, m, dataset, c2).visualize(interp=1)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        finally:
            VS.SPECIAL['flowers'] = special
        sheets = sum(len(v) for k, v in out.items() if isinstance(v, list)) + 1
        return {'batch': m.batch_size, 'interp': 1, 'train_images': n_images, 'sheets': sheets, 'wall_s': round(wall, 3)}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--images', type=int, default=64, help='train / test images of the synthetic data set of the visualiser run')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_stackgan_infer.py needs a GPU')
    dev = torch.device('cuda', 0)
    m, c1, c2 = build(32, dev)
    g = torch.Generator(device=dev).manual_seed(0)

    def fns(B, chain):
        z = torch.randn((B, m.stagei.z_dim), generator=g, device=dev)
        phi = torch.randn((B, m.stagei.embed_dim), generator=g, device=dev)

        def make(fused):
            def fn():
                m.fused_infer = m.stagei.fused_infer = fused
                with torch.no_grad():
                    img = m.stagei.generator(z, phi, reuse=True, is_training=False)[0]
                    return m.generator(img, phi, reuse=True, is_training=False)[0] if chain else img
            return fn
        return make(False), make(True)

    rows = {}
    for name, B, chain in (('stageI_B8', 8, False), ('stageI_B64', 64, False), ('chain_B8', 8, True), ('chain_B32', 32, True)):
        rows[name] = ab(*fns(B, chain), iters=args.iters, repeats=args.repeats)
    m.fused_infer = m.stagei.fused_infer = True

    scale = {}
    for N in (8, 64):
        x = torch.tanh(torch.randn((N, 256, 256, 3), generator=g, device=dev))
        t = statistics.median(timed(lambda: K.bytescale_nearest(x, 128), 50, 5 if i == 0 else 0) for i in range(args.repeats))
        moved = N * (256 * 256 * 3 * 4 + 128 * 128 * 3 * 4 + 128 * 128 * 3)
        scale['N%d' % N] = {'us': round(t * 1e6, 2), 'bytes': moved, 'GB_per_s': round(moved / t * 1e-9, 1),
                            'launches': count_launches(lambda: K.bytescale_nearest(x, 128))}

    print(json.dumps({'bench': 'stackgan_infer', 'generators': rows, 'bytescale_256_to_128': scale,
                      'visualize': visualize_wall(m, c1, c2, args.images)}), flush=True)


if __name__ == '__main__':
    main()
