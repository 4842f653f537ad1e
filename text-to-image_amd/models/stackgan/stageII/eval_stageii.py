"""StageIIEval — reference models/stackgan/stageII/eval_stageii.py: the images come from the chain Stage-I generator -> Stage-II
generator.  `g_net` is restored from the Stage-I config's CHECKPOINT_DIR and `stageII_g_net` from the Stage-II one; a failed
load raises with the reference's message.

The 256 x 256 images are streamed, not stored (50 000 of them in fp32 would take 39 GB): each batch of EVAL.SAMPLE_SIZE is
generated, resized to 299 x 299 from its fp32 store by t2i_resample_bilinear (denormalised in-kernel) and scored before the next
one is drawn.  Only keep_samples=True (for tests) returns the generated images, on the host.

- evaluate_inception: both generators in eval mode; per batch z ~ N(0, 1) then `test.next_batch(bs, 4, embeddings=True)`, the
  batch scored at once; the per-batch predictions in order, with NO shuffle, then get_inception_from_predictions(preds, 10).
- evaluate_fid: the reference's version feeds z to the Stage-II generator and keeps only the last batch, so it cannot run.  Here
  it is the same chain with both generators in training mode (is_training=True: the default argument eval_wgan keeps), the
  PreLogits statistics streamed over every image of every batch through t2i_gram_accumulate, and the real statistics read from
  EVAL.ACT_STAT_PATH (computed from EVAL.R_IMG_PATH first if absent), as wgancls does; 500 on a failure.
- evaluate_imd: StageIEval's, on the chain in eval mode, against the 256 x 256 test images."""
import os

import numpy as np
import torch

from .... import kernels as K
from ....evaluation import fid, inception_score
from ....models.inception.model import IMAGE_SIZE
from ....scope import trainable_variables
from ....utils.saver import Saver, load
from ..stageI.eval_stagei import StageIEval


class StageIIEval(StageIEval):
    def _restore_generator(self):
        m, s1 = self.model, self.model.stagei
        if not trainable_variables('stageII_g_net'):
            with K.dry_run(), torch.no_grad():
                z = torch.empty(self.bs, s1.z_dim, device=m.device)
                phi = torch.empty(self.bs, s1.embed_dim, device=m.device)
                img64, _, _ = s1.generator(z, phi, reuse=bool(trainable_variables('g_net')), is_training=False)
                m.generator(img64, phi, reuse=False, is_training=False)
        for scope, directory, what in (('g_net', s1.cfg.CHECKPOINT_DIR, 'stage I'), ('stageII_g_net', self.cfg.CHECKPOINT_DIR, 'stage II')):
            could_load, _ = load(Saver(m.store, var_list=[scope]), None, directory)
            if not could_load:
                print(' [!] Load failed...')
                raise RuntimeError('Could not load the checkpoints of %s' % what)
            print(' [*] Load SUCCESS')

    def _dims(self):
        return self.model.stagei.z_dim, self.model.stagei.embed_dim

    def _generate_batch(self, z, cond, is_training):
        m = self.model
        img64, _, _ = m.stagei.generator(z, cond, reuse=True, is_training=is_training)
        img, _, _ = m.generator(img64, cond, reuse=True, is_training=is_training)
        return img

    def _stream(self, is_training, keep_samples):
        """Yields each generated batch (device float32 [bs, 256, 256, 3]); keeps a host copy when asked."""
        n_batches = self._n_batches()
        self._kept = []
        for i in range(n_batches):
            print('\rGenerating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
            _, z, cond = self._draw_batch(*self._dims())
            with torch.no_grad():
                img = self._generate_batch(z, cond, is_training).float().contiguous()
            if keep_samples:
                self._kept.append(img.cpu().numpy())
            yield img
        print()

    def _samples(self, keep_samples):
        return dict(samples=np.concatenate(self._kept)) if keep_samples else {}

    def evaluate_inception(self, keep_samples=False):
        """-> dict(mean, std) (+ samples: the generated images in scoring order, with keep_samples)."""
        net = self._inception()
        self._restore_generator()
        print('Generating batches...')
        logits = []
        for img in self._stream(False, keep_samples):
            x = K.resample_bilinear(img, IMAGE_SIZE, IMAGE_SIZE)
            out, _ = net(x)
            logits.append(out.cpu().numpy())
        print('Computing inception score...')
        all_preds = inception_score.softmax32(np.concatenate(logits, 0))
        mean, std = inception_score.get_inception_from_predictions(all_preds, 10)
        print('Inception Score | mean:', '%.2f' % mean, 'std:', '%.2f' % std)
        return dict(mean=mean, std=std, **self._samples(keep_samples))

    def evaluate_fid(self, keep_samples=False):
        """-> dict(fid, mu_gen, sigma_gen, mu_real, sigma_real) (+ samples with keep_samples)."""
        net = self._inception()
        path = self.cfg.EVAL.ACT_STAT_PATH
        if not os.path.exists(path):
            print('Computing activation statistics for real x')
            fid.compute_and_save_activation_statistics(self.cfg.EVAL.R_IMG_PATH, net, self.incep_batch_size, path,
                                                       self.model.device, verbose=True)
        print('Loading activation statistics for the real x')
        mu_real, sigma_real = fid.load_activation_statistics(path)
        self._restore_generator()
        print('Generating batches and their activation statistics...')
        stats = fid.ActivationStatistics(device=self.model.device)
        c = self.incep_batch_size
        for img in self._stream(True, keep_samples):
            for s in range(0, img.shape[0], c):
                x = K.resample_bilinear(img[s:s + c], IMAGE_SIZE, IMAGE_SIZE)
                _, pre = net(x)
                stats.add(pre.reshape(x.shape[0], -1))
        mu_gen, sigma_gen = stats.finalize()
        print('calculate FID:', end=' ', flush=True)
        try:
            value = fid.calculate_frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)
        except Exception as e:          # the reference's fallback
            print(e)
            value = 500
        print(value)
        return dict(fid=value, mu_gen=mu_gen, sigma_gen=sigma_gen, mu_real=mu_real, sigma_real=sigma_real,
                    **self._samples(keep_samples))
