"""Inception score — the role of reference evaluation/inception_score.py.

`get_inception_score` takes the generated images as a device store ([N, H, W, 3]: uint8, or float32 generator output that
the resize kernel denormalises as denormalize_images does) and keeps them there: the reference's shuffle is a row-index
array, and each batch is gathered, resized to 299 x 299 (Pillow's bilinear, bit for bit) and normalised by one
t2i_resample_bilinear launch.  As in the reference only floor(N / batch_size) full batches are scored.  The softmax is fp32
(tf.nn.softmax's dtype); the score is reduced in float64 on the host with the reference's splits."""
import math

import numpy as np
import torch

from .. import kernels as K
from ..models.inception.model import IMAGE_SIZE


def softmax32(logits):
    """float32 softmax of [n, classes] logits on the host."""
    x = np.asarray(logits, np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def get_inception_from_predictions(preds, splits, verbose=True):
    """exp(mean_i KL(p_i || mean p)) per split of the rows, in float64 -> (mean, std) over the splits."""
    preds = np.asarray(preds, np.float64)
    n = preds.shape[0]
    scores = []
    for i in range(splits):
        if verbose:
            print('\rComputing score for slice %d/%d' % (i + 1, splits), end='', flush=True)
        part = preds[i * n // splits:(i + 1) * n // splits]
        marginal = part.mean(axis=0, keepdims=True)
        kl = (part * (np.log(part) - np.log(marginal))).sum(axis=1).mean()
        scores.append(np.exp(kl))
    if verbose:
        print()
    return float(np.mean(scores)), float(np.std(scores))


def inception_predictions(images, net, batch_size, indices, verbose=False):
    """Softmax predictions (float32 [n_batches * batch_size, classes], host) of the store rows indices[:n_batches * batch_size]."""
    n_batches = len(indices) // batch_size
    idx = torch.as_tensor(np.asarray(indices[:n_batches * batch_size], np.int64), dtype=torch.int32).to(images.device)
    preds = []
    for i in range(n_batches):
        if verbose:
            print('\rPropagating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
        x = K.resample_bilinear(images, IMAGE_SIZE, IMAGE_SIZE, rows=idx[i * batch_size:(i + 1) * batch_size])
        logits, _ = net(x)
        preds.append(logits.cpu().numpy())
    if verbose and n_batches:
        print()
    return softmax32(np.concatenate(preds, 0) if preds else np.zeros((0, net.num_classes), np.float32))


def get_inception_score(images, net, batch_size, splits, verbose=False):
    """images: device store [N, H, W, 3] (uint8 in [0, 255] or float32 in [-1, 1]).  Consumes np.random like the reference
    (one np.random.shuffle of the indices).  -> (mean, std, indices)."""
    num_examples = images.shape[0]
    if batch_size > num_examples:
        raise ValueError('Inception batch size %d is larger than the %d images' % (batch_size, num_examples))
    indices = list(np.arange(num_examples))
    np.random.shuffle(indices)
    preds = inception_predictions(images, net, batch_size, indices, verbose)
    mean, std = get_inception_from_predictions(preds, splits, verbose)
    return mean, std, np.asarray(indices[:int(math.floor(num_examples / batch_size)) * batch_size])
