"""GeneratorEval — the one evaluator of the five models: Inception score, FID and Inception match distance of a restored generator
(reference models/*/eval_*.py, which are copies of models/wgancls/eval_wgan.py).

Every evaluation restores the generator and draws in the reference's order from the global np.random stream: per batch of
`self.bs`, z ~ N(0, 1) [bs, z_dim] (float64, then cast), then `dataset.test.next_batch(bs, 4, embeddings=True)`.  The images are
either
  - stored: the whole [SIZE // bs * bs, H, W, 3] float32 store stays on the device as the generator wrote it (the resize kernel
    denormalises as denormalize_images would) and is scored by evaluation/inception_score.py (one np.random.shuffle, full Inception
    batches only, 10 splits) or evaluation/fid.py (floor(N / incep) full batches in order); or
  - streamed: each batch is resized to 299 x 299 by t2i_resample_bilinear and scored before the next one is drawn, nothing kept
    between batches (50 000 images of 256 x 256 would take 39 GB in fp32): the predictions in generation order with NO shuffle,
    the PreLogits statistics through t2i_gram_accumulate.  Only keep_samples=True (for tests) returns the images, on the host.
The real images' statistics are read from EVAL.ACT_STAT_PATH, or computed from the images under EVAL.R_IMG_PATH and saved there
first; on a failure of the distance the reference prints the error and reports 500, which is kept.  evaluate_imd is an addition the
reference does not have (evaluation/imd.py): each real test image of the batch against the image generated from its embedding.
evaluate_swd is another (evaluation/swd.py): the sliced Wasserstein distance of the same pairs' Laplacian-pyramid patches, per
resolution level; it needs no Inception net and no EVAL.ACT_STAT_PATH.  evaluate_msssim (evaluation/msssim.py) is the one
evaluation that compares generated images with each other: the multi-scale structural similarity of pairs of them, which is 1 for a
generator that ignores z; it needs no Inception net either.  evaluate_prdc (evaluation/prdc.py) asks where the generated SET lies:
precision, recall, density and coverage from k-nearest-neighbour balls around the PreLogits features of evaluate_imd's batches.
evaluate_mmd (evaluation/mmd.py) is the Kernel Inception distance of the same two feature sets, the distance for small test splits.

A model's evaluator states what differs (DESIGN.md has the table): restore(), dims(), generate_batch(), and the attributes below."""
import os

import numpy as np
import torch

from .. import kernels as K
from ..models.inception.model import IMAGE_SIZE, load_inception_inference
from ..utils.saver import restore_g_net
from . import fid, imd, inception_score, mmd, msssim, prdc, swd


class GeneratorEval(object):
    stored = True                   # False: streamed
    fid_is_training = True          # FID's generator mode (the reference's default argument, kept); IS and IMD run is_training=False
    keep_preds = False              # streamed IS: the predictions in the result
    size_error = 'EVAL.SIZE %d is smaller than EVAL.SAMPLE_SIZE %d'
    announce = dict(inception='Generating x...', fid='Generating x...', imd='Generating pairs...')

    def __init__(self, sess, model, dataset, cfg, incep_batch_size=None):
        self.sess = sess                   # unused: there is no TF session
        self.model = model
        self.dataset = dataset
        self.cfg = cfg
        self.bs = self.batch_size()
        self.incep_batch_size = incep_batch_size or self.default_incep_batch_size()

    # ---- what a model states ------------------------------------------------------------------------------------------------
    def batch_size(self):
        return self.cfg.EVAL.SAMPLE_SIZE

    def default_incep_batch_size(self):
        return self.cfg.EVAL.INCEP_BATCH_SIZE

    def restore(self):
        """`g_net` (a launch-free dry pass creates its variables if the model has not) from the latest checkpoint."""
        restore_g_net(self.model, self.cfg.CHECKPOINT_DIR, self.bs, RuntimeError('Could not load the checkpoints of the generator'))

    def dims(self):
        return self.model.z_dim, self.model.embed_dim

    def generate_batch(self, z, cond, is_training):
        """-> the generated images [bs, H, W, 3] of device tensors z, cond."""
        raise NotImplementedError

    def is_chunk(self):
        """Rows per Inception call of the streamed IS (the Inception GEMMs choose their tiles by it)."""
        return self.incep_batch_size

    # ---- the batches ----------------------------------------------------------------------------------------------------------
    def _inception(self):
        return load_inception_inference(self.cfg.EVAL.NUM_CLASSES, self.cfg.EVAL.INCEP_CHECKPOINT_DIR, self.model.device)

    def _n_batches(self):
        n_batches = self.cfg.EVAL.SIZE // self.bs
        if n_batches == 0:
            raise ValueError(self.size_error % (self.cfg.EVAL.SIZE, self.bs))
        return n_batches

    def _draw_batch(self, with_real=False):
        """The reference's draws for one batch: z ~ N(0, 1) [bs, z_dim], then the test batch. -> (real images or None, z,
        embeddings) on the device."""
        dev = self.model.device
        z_dim, embed_dim = self.dims()
        sample_z = np.random.normal(0, 1, size=(self.bs, z_dim))
        images, _, embed, _, _ = self.dataset.test.next_batch(self.bs, 4, embeddings=True)
        z = torch.as_tensor(sample_z, dtype=torch.float32).to(dev)
        cond = embed if torch.is_tensor(embed) else torch.as_tensor(np.asarray(embed), dtype=torch.float32)
        cond = cond.to(device=dev, dtype=torch.float32).reshape(self.bs, embed_dim)
        if not with_real:
            return None, z, cond
        real = images if torch.is_tensor(images) else torch.as_tensor(np.asarray(images, np.float32))
        return real.to(device=dev, dtype=torch.float32).contiguous(), z, cond

    def _batches(self, is_training, keep_samples=False, with_real=False):
        """Yields (real or None, generated) per batch, device float32 contiguous; keeps host copies when asked."""
        n_batches = self._n_batches()
        self._kept = []
        for i in range(n_batches):
            print('\rGenerating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
            real, z, cond = self._draw_batch(with_real)
            self._cond = cond                             # evaluate_msssim('caption') generates from it a second time
            with torch.no_grad():
                img = self.generate_batch(z, cond, is_training).float().contiguous()
            if keep_samples:
                self._kept.append((real.cpu().numpy() if with_real else None, img.cpu().numpy()))
            yield real, img
        print()

    def _kept_samples(self, keep_samples):
        return dict(samples=np.concatenate([g for _, g in self._kept])) if keep_samples else {}

    def _generate(self, is_training):
        """-> device float32 [SIZE // bs * bs, H, W, 3]: the generator's images, batch after batch."""
        h, w, c = self.model.image_dims[:3]
        samples = torch.empty((self._n_batches() * self.bs, h, w, c), dtype=torch.float32, device=self.model.device)
        for i, (_, img) in enumerate(self._batches(is_training)):
            samples[i * self.bs:(i + 1) * self.bs].copy_(img.reshape(self.bs, h, w, c))
        return samples

    def _chunks(self, img, c):
        for s in range(0, img.shape[0], c):
            yield K.resample_bilinear(img[s:s + c], IMAGE_SIZE, IMAGE_SIZE)

    def _announce(self, mode):
        if mode in self.announce:
            print(self.announce[mode])

    # ---- the evaluations ------------------------------------------------------------------------------------------------------
    def evaluate_inception(self, keep_samples=False):
        """stored -> dict(mean, std, indices: the shuffled sample order that was scored, samples: the device store);
        streamed -> dict(mean, std) (+ preds: float32 [n, classes] in generation order) (+ samples, host, with keep_samples)."""
        net = self._inception()
        self.restore()
        self._announce('inception')
        if self.stored:
            samples = self._generate(is_training=False)
            print('Computing inception score...')
            mean, std, indices = inception_score.get_inception_score(samples, net, self.incep_batch_size, 10, verbose=True)
            out = dict(indices=indices, samples=samples)
        else:
            logits = []
            for _, img in self._batches(False, keep_samples):
                for x in self._chunks(img, self.is_chunk()):
                    logits.append(net(x)[0].cpu().numpy())
            print('Computing inception score...')
            preds = inception_score.softmax32(np.concatenate(logits, 0))
            mean, std = inception_score.get_inception_from_predictions(preds, 10)
            out = self._kept_samples(keep_samples)
            if self.keep_preds:
                out['preds'] = preds
        print('Inception Score | mean:', '%.2f' % mean, 'std:', '%.2f' % std)
        return dict(mean=mean, std=std, **out)

    def _real_statistics(self, net):
        path = self.cfg.EVAL.ACT_STAT_PATH
        if not os.path.exists(path):
            print('Computing activation statistics for real x')
            fid.compute_and_save_activation_statistics(self.cfg.EVAL.R_IMG_PATH, net, self.incep_batch_size, path,
                                                       self.model.device, verbose=True)
        print('Loading activation statistics for the real x')
        return fid.load_activation_statistics(path)

    def evaluate_fid(self, keep_samples=False):
        """-> dict(fid, mu_gen, sigma_gen, mu_real, sigma_real) + samples (stored: the device store; streamed: with keep_samples)."""
        net = self._inception()
        mu_real, sigma_real = self._real_statistics(net)
        self.restore()
        self._announce('fid')
        if self.stored:
            samples = self._generate(self.fid_is_training)
            print('Computing activation statistics for generated x...')
            mu_gen, sigma_gen = fid.calculate_activation_statistics(samples, net, self.incep_batch_size, verbose=True)
            out = dict(samples=samples)
        else:
            stats = fid.ActivationStatistics(device=self.model.device)
            for _, img in self._batches(self.fid_is_training, keep_samples):
                for x in self._chunks(img, self.incep_batch_size):
                    _, pre = net(x)
                    stats.add(pre.reshape(x.shape[0], -1))
            mu_gen, sigma_gen = stats.finalize()
            out = self._kept_samples(keep_samples)
        print('calculate FID:', end=' ', flush=True)
        try:
            value = fid.calculate_frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)
        except Exception as e:          # the reference's fallback
            print(e)
            value = 500
        print(value)
        return dict(fid=value, mu_gen=mu_gen, sigma_gen=sigma_gen, mu_real=mu_real, sigma_real=sigma_real, **out)

    def evaluate_imd(self, keep_samples=False):
        """-> dict(mean, std, distances float64 [n]) and, with keep_samples, the host pairs (real, gen: float32 [n, H, W, 3] in
        [-1, 1]).  Per chunk of INCEP_BATCH_SIZE pairs, one resize of each half, one Inception forward and one t2i_cosine_distance
        launch."""
        net = self._inception()
        self.restore()
        self._announce('imd')
        c = self.incep_batch_size
        dists = []
        for real, gen in self._batches(False, keep_samples, with_real=True):
            for s in range(0, self.bs, c):
                dists.append(imd.pair_distances(real[s:s + c], gen[s:s + c], net))
        d = torch.cat(dists).cpu().numpy()
        mean, std = float(np.mean(d)), float(np.std(d))
        print('IMD | mean: %.4f std: %.4f' % (mean, std))
        out = dict(mean=mean, std=std, distances=d)
        if keep_samples:
            out.update(real=np.concatenate([r for r, _ in self._kept]), gen=np.concatenate([g for _, g in self._kept]))
        return out

    def evaluate_swd(self, keep_samples=False):
        """-> dict(levels: SWD x 10^3 per pyramid level, finest first; mean; sides) of the real test images against the images
        generated from their embeddings, and, with keep_samples, the host pairs (real, gen).  One SlicedWasserstein.add per batch;
        its draws come from its own generator, so the batches are those of evaluate_imd."""
        self.restore()
        sw = None
        for real, gen in self._batches(False, keep_samples, with_real=True):
            if sw is None:
                sw = swd.SlicedWasserstein(tuple(gen.shape[1:]), self._n_batches() * self.bs, self.model.device)
            sw.add(real.reshape(gen.shape), gen)
        out = sw.finalize()
        for side, v in zip(out['sides'], out['levels']):
            print('SWD x 1e3 | %4d x %-4d: %.4f' % (side, side, v))
        print('SWD x 1e3 | mean: %.4f' % out['mean'])
        if keep_samples:
            out.update(real=np.concatenate([r for r, _ in self._kept]), gen=np.concatenate([g for _, g in self._kept]))
        return out

    def evaluate_msssim(self, pairs='random', keep_samples=False):
        """-> MultiScaleSSIM.finalize()'s dict (values, mean, std, cs_levels, clamped, sides) of pairs of GENERATED images (+ samples,
        host, with keep_samples); the batches and their draws from np.random are those of the streamed evaluate_inception.
        pairs='random' (the paper's protocol): image i of a batch against image i + bs // 2, different z and different captions,
        bs // 2 pairs per batch.  pairs='caption': the batch is generated a second time from the SAME embeddings and a fresh z, image i
        against its regeneration, bs pairs per batch: 1 means the generator ignores z.  The fresh z is normal(0, 1, (bs, z_dim)) cast
        to float32 from the evaluation's own np.random.RandomState(0); the global stream is left alone."""
        if pairs not in ('random', 'caption'):
            raise ValueError("evaluate_msssim: pairs must be 'random' or 'caption', got %r" % (pairs,))
        if pairs == 'random' and self.bs < 2:
            raise ValueError('evaluate_msssim: random pairs need a batch of at least 2 images, got %d' % self.bs)
        self.restore()
        rs = np.random.RandomState(0)
        ms, half = None, self.bs // 2
        for _, img in self._batches(False, keep_samples):
            if ms is None:
                ms = msssim.MultiScaleSSIM(tuple(img.shape[1:]), self.model.device)
            if pairs == 'random':
                ms.add(img[:half], img[half:2 * half])
            else:
                z = torch.as_tensor(rs.normal(0, 1, size=(self.bs, self.dims()[0])).astype(np.float32)).to(self.model.device)
                with torch.no_grad():
                    again = self.generate_batch(z, self._cond, False).float().contiguous()
                ms.add(img, again.reshape(img.shape))
        out = ms.finalize()
        print('MS-SSIM (%s) | mean: %.4f std: %.4f clamped: %d' % (pairs, out['mean'], out['std'], out['clamped']))
        print('MS-SSIM (%s) | cs per scale: %s' % (pairs, ' '.join('%dx%d: %.4f' % (h, w, v) for (h, w), v in zip(out['sides'], out['cs_levels']))))
        out.update(self._kept_samples(keep_samples))
        return out

    def evaluate_prdc(self, nearest_k=5, keep_samples=False, keep_features=False):
        """-> ManifoldMetrics.finalize()'s dict (precision, recall, density, coverage, nearest_k, n_real, n_gen) (+ the host pairs
        real, gen with keep_samples; + real_features, gen_features, host float32, with keep_features).  The batches and their draws
        from np.random are those of evaluate_imd; per chunk of INCEP_BATCH_SIZE pairs one Inception forward scores both halves.
        The test split starts a new permutation once it is exhausted, so real features are kept only for the first
        num_examples // bs batches (one epoch, no image twice: a repeated image's nearest neighbours would be its own copies and
        every radius would collapse); generated features are kept for all SIZE // bs batches."""
        if int(nearest_k) != nearest_k or not 1 <= int(nearest_k) <= K.KNN_MAX_K:
            raise ValueError('evaluate_prdc: nearest_k must be in 1..%d, got %r' % (K.KNN_MAX_K, nearest_k))
        mm = self._feature_sets(lambda dim: prdc.ManifoldMetrics(dim, self.model.device, nearest_k), keep_samples)
        out = mm.finalize()
        print('PRDC (k = %d) | precision: %.4f recall: %.4f density: %.4f coverage: %.4f | %d real, %d generated' % (
            out['nearest_k'], out['precision'], out['recall'], out['density'], out['coverage'], out['n_real'], out['n_gen']))
        return self._with_kept_sets(out, mm, keep_samples, keep_features)

    def _feature_sets(self, make, keep_samples):
        """The loop evaluate_prdc and evaluate_mmd share: -> make(dim), fed with the PreLogits features of evaluate_imd's batches, the
        real ones for the first num_examples // bs batches only."""
        net = self._inception()
        self.restore()
        c = self.incep_batch_size
        real_batches = self.dataset.test.num_examples // self.bs
        sets = None
        for i, (real, gen) in enumerate(self._batches(False, keep_samples, with_real=True)):
            for s in range(0, self.bs, c):
                pre_real, pre_gen = imd.pair_features(real[s:s + c], gen[s:s + c], net)
                if sets is None:
                    sets = make(pre_gen.shape[1])
                if i < real_batches:
                    sets.add_real(pre_real)
                sets.add_gen(pre_gen)
        return sets

    def _with_kept_sets(self, out, sets, keep_samples, keep_features):
        if keep_samples:
            out.update(real=np.concatenate([r for r, _ in self._kept]), gen=np.concatenate([g for _, g in self._kept]))
        if keep_features:
            out.update(real_features=sets.real.rows().cpu().numpy(), gen_features=sets.gen.rows().cpu().numpy())
        return out

    def evaluate_mmd(self, num_subsets=100, max_subset_size=1000, keep_samples=False, keep_features=False):
        """-> KernelDistance.finalize()'s dict (kid, kid_std, subsets, subset_size, n_real, n_gen, degree, gamma, coef0) (+ real, gen
        and real_features, gen_features as evaluate_prdc): the Kernel Inception distance (evaluation/mmd.py) of the feature sets of
        evaluate_prdc, by the same batches, chunks and one-epoch rule for the real set; the draws from the global np.random are those
        of evaluate_imd (the subsets come from the metric's own generator)."""
        if int(num_subsets) != num_subsets or not 1 <= int(num_subsets) <= mmd.MAX_SUBSETS:
            raise ValueError('evaluate_mmd: num_subsets must be in 1..%d, got %r' % (mmd.MAX_SUBSETS, num_subsets))
        if int(max_subset_size) != max_subset_size or int(max_subset_size) < 2:
            raise ValueError('evaluate_mmd: max_subset_size must be at least 2, got %r' % (max_subset_size,))
        kd = self._feature_sets(lambda dim: mmd.KernelDistance(dim, self.model.device, num_subsets, max_subset_size), keep_samples)
        out = kd.finalize()
        print('KID x 1e3 (--eval mmd) | mean: %.4f std: %.4f | %d subsets of %d | %d real, %d generated' % (
            1e3 * out['kid'], 1e3 * out['kid_std'], out['subsets'], out['subset_size'], out['n_real'], out['n_gen']))
        return self._with_kept_sets(out, kd, keep_samples, keep_features)
