"""Frechet Inception distance — the role of reference evaluation/fid.py.

Activation statistics are streamed: each batch's PreLogits [B, 2048] stays on the device and t2i_gram_accumulate adds
sum (x - s) and (x - s)^T (x - s) into fp64 accumulators, with s the first batch's mean (so the fp32 products never form the
uncentred moments that cancel).  `mu` and `sigma` (np.cov's n - 1 normaliser) come out in float64.  The distance itself is
computed once per evaluation on the host in float64 with scipy's sqrtm, as the reference does."""
import os
import warnings

import numpy as np
import torch

from .. import kernels as K
from ..models.inception.model import IMAGE_SIZE, PRELOGITS_DIM
from .resize import to_rgb


class ActivationStatistics(object):
    """Running mean / covariance of rows added on the device."""

    def __init__(self, d=PRELOGITS_DIM, device=None):
        self.d, self.n = d, 0
        self.device = device or torch.device('cuda', torch.cuda.current_device())
        self.shift = None
        self.sum = torch.zeros(d, dtype=torch.float64, device=self.device)
        self.gram = torch.zeros((d, d), dtype=torch.float64, device=self.device)

    def add(self, acts):
        """acts float32 [n, d] (device)."""
        if acts.shape[0] == 0:
            return
        if self.shift is None:
            first = acts.cpu().numpy().astype(np.float64).mean(axis=0).astype(np.float32)     # the shift: first batch's mean
            self.shift = torch.from_numpy(first).to(self.device)
        K.gram_accumulate(acts.contiguous(), self.shift, self.sum, self.gram)
        self.n += acts.shape[0]

    def finalize(self):
        """-> (mu float64 [d], sigma float64 [d, d])."""
        if self.n < 2:
            raise ValueError('activation statistics need at least 2 rows, got %d' % self.n)
        s = self.shift.double().cpu().numpy()
        m = self.sum.cpu().numpy() / self.n
        g = self.gram.cpu().numpy()
        sigma = (g - self.n * np.outer(m, m)) / (self.n - 1)
        return s + m, sigma


def get_activations(images, net, batch_size, verbose=False, stats=None):
    """PreLogits statistics of the store rows in order, floor(N / batch_size) full batches (reference get_activations).
    images: device store [N, H, W, 3] (uint8, or float32 generator output).  -> ActivationStatistics."""
    n = images.shape[0]
    if batch_size > n:
        raise RuntimeError('batch size is bigger than the data size')
    stats = stats or ActivationStatistics(device=images.device)
    n_batches = n // batch_size
    for i in range(n_batches):
        if verbose:
            print('\rPropagating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
        x = K.resample_bilinear(images[i * batch_size:(i + 1) * batch_size], IMAGE_SIZE, IMAGE_SIZE)
        _, pre = net(x)
        stats.add(pre)
    if verbose:
        print(' done')
    return stats


def calculate_activation_statistics(images, net, batch_size, verbose=False):
    """-> (mu, sigma) in float64."""
    return get_activations(images, net, batch_size, verbose).finalize()


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """||mu1 - mu2||^2 + Tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)) in float64.  A non-finite sqrtm is retried with eps on
    both diagonals; an imaginary part is dropped if the diagonal's is within 1e-3 of zero, else ValueError."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1).astype(np.float64), np.atleast_1d(mu2).astype(np.float64)
    sigma1, sigma2 = np.atleast_2d(sigma1).astype(np.float64), np.atleast_2d(sigma2).astype(np.float64)
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError('mean / covariance shapes differ: %s %s, %s %s' % (mu1.shape, mu2.shape, sigma1.shape, sigma2.shape))
    diff = mu1 - mu2
    root, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(root).all():
        warnings.warn('fid calculation produces singular product; adding %s to diagonal of cov estimates' % eps)
        offset = np.eye(sigma1.shape[0]) * eps
        root = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0, atol=1e-3):
            raise ValueError('Imaginary component {}'.format(np.max(np.abs(root.imag))))
        root = root.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(root))


def save_activation_statistics(mu, sigma, path):
    """npz(mu, sigma); refuses to overwrite, as the reference does."""
    if os.path.exists(path):
        raise RuntimeError('Path {} already exists. Statistics not saved'.format(path))
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, mu=mu, sigma=sigma)


def load_activation_statistics(path):
    with np.load(path) as f:
        return f['mu'][:], f['sigma'][:]


def load_inception_data(full_path, alphabetic=False):
    """uint8 images (any size; grayscale made [h, w, 3] by prep_incep_img's np.resize) of every file under full_path whose
    name contains 'jpg' or 'png' (reference utils/utils.py load_inception_data)."""
    from PIL import Image
    if not os.path.exists(full_path):
        raise RuntimeError('Path %s does not exits' % full_path)
    images = []
    for path, _, files in os.walk(full_path):
        for name in (sorted(files) if alphabetic else files):
            filename = os.path.join(path, name)
            if (name.rfind('jpg') != -1 or name.rfind('png') != -1) and os.path.isfile(filename):
                im = Image.open(filename)
                if im.mode not in ('L', 'RGB'):
                    im = im.convert('RGB')
                images.append(to_rgb(np.asarray(im)))
    if not images:
        raise RuntimeError('no images under %s' % full_path)
    print('x', len(images), images[0].shape)
    return images


def image_list_statistics(images, net, batch_size, device, verbose=False):
    """Statistics of host uint8 images of any sizes: each is uploaded and resized by its own launch into the batch."""
    if batch_size > len(images):
        raise RuntimeError('batch size is bigger than the data size')
    stats = ActivationStatistics(device=device)
    n_batches = len(images) // batch_size
    for i in range(n_batches):
        if verbose:
            print('\rPropagating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
        x = torch.empty((batch_size, IMAGE_SIZE, IMAGE_SIZE, 3), dtype=torch.float32, device=device)
        for j in range(batch_size):
            img = torch.from_numpy(np.ascontiguousarray(images[i * batch_size + j], np.uint8)).to(device)[None]
            K.resample_bilinear(img, IMAGE_SIZE, IMAGE_SIZE, out=x[j:j + 1])
        _, pre = net(x)
        stats.add(pre)
    if verbose:
        print(' done')
    return stats.finalize()


def compute_and_save_activation_statistics(img_path, net, batch_size, save_path, device, verbose=False):
    mu, sigma = image_list_statistics(load_inception_data(img_path), net, batch_size, device, verbose)
    save_activation_statistics(mu, sigma, save_path)
    return mu, sigma
