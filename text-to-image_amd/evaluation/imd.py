"""Inception match distance (IMD) — reference evaluation/imd.py.

For paired real and generated images, the cosine distance (scipy.spatial.distance.cosine) between their InceptionV3 PreLogits
activations; the reference reports its mean and std.  Per batch, both halves are resized (Pillow's bilinear, the
t2i_resample_bilinear kernel) into one [2 c, 299, 299, 3] input, Inception runs once, and t2i_cosine_distance takes the
distance of PreLogits rows [0, c) against [c, 2c) in fp64 on the device.

    python -m t2i_amd.evaluation.imd --real DIR --gen DIR --checkpoint-dir DIR [--num-classes 20] [--batch-size 64]

reads both folders alphabetically (fid.load_inception_data) and pairs the i-th real image with the i-th generated one."""
import argparse
import os
import sys

import numpy as np
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    from t2i_amd.models.inception.model import IMAGE_SIZE
else:
    from .. import kernels as K
    from ..models.inception.model import IMAGE_SIZE


def get_cosine_dist(real_img_act, gen_img_act):
    """The host statement of the distance, row by row in float64: clip(1 - u.v / sqrt(u.u v.v), 0, 2), NaN when a norm is 0
    (scipy.spatial.distance.cosine).  real_img_act, gen_img_act: [n, d] (or [d]) -> float64 [n] (or a scalar)."""
    u = np.asarray(gen_img_act, np.float64)
    v = np.asarray(real_img_act, np.float64)
    uv = (u * v).sum(-1)
    uu = (u * u).sum(-1)
    vv = (v * v).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        dist = 1.0 - uv / np.sqrt(uu * vv)
    dist = np.where((uu == 0) | (vv == 0), np.nan, dist)
    return np.clip(dist, 0.0, 2.0)


def pair_features(real, gen, net):
    """real, gen: device stores [c, H, W, 3] (uint8, or float32 in [-1, 1] denormalised in the resize kernel; the two may differ
    in size) -> their PreLogits rows ([c, d], [c, d]) from one Inception forward over both halves."""
    c = real.shape[0]
    if gen.shape[0] != c:
        raise ValueError('pair_features: %d real and %d generated images' % (c, gen.shape[0]))
    x = torch.empty((2 * c, IMAGE_SIZE, IMAGE_SIZE, 3), dtype=torch.float32, device=real.device)
    K.resample_bilinear(real.contiguous(), IMAGE_SIZE, IMAGE_SIZE, out=x[:c])
    K.resample_bilinear(gen.contiguous(), IMAGE_SIZE, IMAGE_SIZE, out=x[c:])
    _, pre = net(x)
    pre = pre.reshape(2 * c, -1)
    return pre[:c], pre[c:]


def pair_distances(real, gen, net):
    """-> float64 [c] device distances of the pairs of pair_features: one Inception forward, one cosine launch."""
    return K.cosine_distance(*pair_features(real, gen, net))


def compute_imd(real_img, gen_img, net, batch_size, verbose=False):
    """real_img, gen_img: equal-length lists of uint8 [h, w, 3] images (any sizes).  The reference's batches:
    n_used = (n // batch_size) * batch_size pairs.  -> (mean, std, distances float64 [n_used])."""
    assert len(real_img) == len(gen_img)
    assert type(real_img[0]) == np.ndarray
    assert type(gen_img[0]) == np.ndarray
    assert len(real_img[0].shape) == 3
    assert len(gen_img[0].shape) == 3
    assert np.max(real_img[0]) > 10
    assert np.min(gen_img[0]) >= 0.0
    d0 = len(real_img)
    if batch_size > d0:
        raise RuntimeError('batch size is bigger than the data size')
    n_batches = d0 // batch_size
    device = torch.device('cuda', torch.cuda.current_device())
    distances = torch.empty(n_batches * batch_size, dtype=torch.float64, device=device)
    x = torch.empty((2 * batch_size, IMAGE_SIZE, IMAGE_SIZE, 3), dtype=torch.float32, device=device)
    for i in range(n_batches):
        if verbose:
            print('\rComputing batch %d/%d' % (i + 1, n_batches), end='', flush=True)
        for j in range(batch_size):               # each image is resized from its own size by a launch of its own
            for half, images in ((0, real_img), (batch_size, gen_img)):
                img = torch.from_numpy(np.ascontiguousarray(images[i * batch_size + j], np.uint8)).to(device)[None]
                K.resample_bilinear(img, IMAGE_SIZE, IMAGE_SIZE, out=x[half + j:half + j + 1])
        _, pre = net(x)
        pre = pre.reshape(2 * batch_size, -1)
        K.cosine_distance(pre[:batch_size], pre[batch_size:], out=distances[i * batch_size:(i + 1) * batch_size])
    if verbose:
        print(' done')
    d = distances.cpu().numpy()
    mean, std = float(np.mean(d)), float(np.std(d))
    print('Mean {}, Std: {}'.format(mean, std))
    return mean, std, d


def main(argv=None):
    from t2i_amd.evaluation.fid import load_inception_data
    from t2i_amd.models.inception.model import load_inception_inference
    ap = argparse.ArgumentParser(description='Inception match distance of paired real / generated image folders')
    ap.add_argument('--real', required=True, help='folder of the real images (read alphabetically)')
    ap.add_argument('--gen', required=True, help='folder of the generated images (read alphabetically)')
    ap.add_argument('--checkpoint-dir', required=True, help='the fine-tuned Inception checkpoint directory')
    ap.add_argument('--num-classes', type=int, default=20, help='20 for flowers')
    ap.add_argument('--batch-size', type=int, default=64)
    args = ap.parse_args(argv)
    if args.batch_size <= 0:
        raise ValueError('--batch-size must be positive, got %d' % args.batch_size)
    real_images = load_inception_data(args.real, alphabetic=True)
    gen_images = load_inception_data(args.gen, alphabetic=True)
    net = load_inception_inference(args.num_classes, args.checkpoint_dir, torch.device('cuda', torch.cuda.current_device()))
    return compute_imd(real_images, gen_images, net, args.batch_size)


if __name__ == '__main__':
    main()
