"""WGanClsEval — the evaluator of the reference's models/wgancls/eval_wgan.py (what run.py starts when EVAL.FLAG is set;
here behind `run.py --eval is|fid`).

Both evaluations restore only the generator (g_net) from the latest checkpoint and draw in the reference's order from the
global np.random stream: per batch of EVAL.SAMPLE_SIZE, z ~ N(0, 1) [bs, z_dim], then `dataset.test.next_batch(bs, 4,
embeddings=True)`.  The generated images stay on the device as the generator wrote them (float32 in [-1, 1]); the resize
kernel reads them as denormalize_images' uint8 would be, so the store is never copied or converted.

- evaluate_inception: the generator in eval mode (moving BN statistics, conditioning noise on), EVAL.SIZE // SAMPLE_SIZE
  batches, then evaluation/inception_score.py (shuffle, full Inception batches only, 10 splits).
- evaluate_fid: the generator with is_training=True, i.e. batch statistics over each SAMPLE_SIZE batch (the reference's
  default argument, kept).  The real images' statistics are read from EVAL.ACT_STAT_PATH, or computed from the JPEGs under
  EVAL.R_IMG_PATH and saved there first.  The distance is evaluation/fid.py's; on a failure the reference prints the error
  and reports 500, which is kept.

Both return their numbers as well as printing them, with what a caller needs to check them (the host samples' indices)."""
import numpy as np
import torch

from ... import kernels as K
from ...evaluation import fid, inception_score
from ...models.inception.model import load_inception_inference
from ...utils.saver import Saver, load


class WGanClsEval(object):
    def __init__(self, sess, model, dataset, cfg, incep_batch_size=None):
        self.sess = sess                   # unused: there is no TF session
        self.model = model
        self.dataset = dataset
        self.cfg = cfg
        self.bs = cfg.EVAL.SAMPLE_SIZE
        self.incep_batch_size = incep_batch_size or cfg.EVAL.INCEP_BATCH_SIZE

    def _restore_generator(self):
        m = self.model
        from ...scope import trainable_variables
        if not trainable_variables('g_net'):
            with K.dry_run(), torch.no_grad():
                m.generator(torch.empty(self.bs, m.z_dim, device=m.device), torch.empty(self.bs, m.embed_dim, device=m.device),
                            reuse=False, is_training=False)
        could_load, _ = load(Saver(m.store, var_list=['g_net']), None, self.cfg.CHECKPOINT_DIR)
        if not could_load:
            print(' [!] Load failed...')
            raise RuntimeError('Could not load the checkpoints of the generator')
        print(' [*] Load SUCCESS')

    def _inception(self):
        return load_inception_inference(self.cfg.EVAL.NUM_CLASSES, self.cfg.EVAL.INCEP_CHECKPOINT_DIR, self.model.device)

    def _generate(self, is_training):
        """-> device float32 [SIZE // bs * bs, H, W, 3]: the generator's images, batch after batch."""
        m = self.model
        n_batches = self.cfg.EVAL.SIZE // self.bs
        if n_batches == 0:
            raise ValueError('EVAL.SIZE %d is smaller than EVAL.SAMPLE_SIZE %d' % (self.cfg.EVAL.SIZE, self.bs))
        h, w, c = m.image_dims[0], m.image_dims[1], m.image_dims[2]
        samples = torch.empty((n_batches * self.bs, h, w, c), dtype=torch.float32, device=m.device)
        for i in range(n_batches):
            print('\rGenerating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
            sample_z = np.random.normal(0, 1, size=(self.bs, m.z_dim))
            _, _, embed, _, _ = self.dataset.test.next_batch(self.bs, 4, embeddings=True)
            z = torch.as_tensor(sample_z, dtype=torch.float32).to(m.device)
            cond = embed if torch.is_tensor(embed) else torch.as_tensor(np.asarray(embed), dtype=torch.float32)
            cond = cond.to(device=m.device, dtype=torch.float32)
            with torch.no_grad():
                img, _, _ = m.generator(z, cond.reshape(self.bs, m.embed_dim), reuse=True, is_training=is_training)
            samples[i * self.bs:(i + 1) * self.bs].copy_(img.float().reshape(self.bs, h, w, c))
        print()
        return samples

    def evaluate_inception(self):
        """-> dict(mean, std, indices: the shuffled sample order that was scored, samples: the device store)."""
        net = self._inception()
        self._restore_generator()
        print('Generating x...')
        samples = self._generate(is_training=False)
        print('Computing inception score...')
        mean, std, indices = inception_score.get_inception_score(samples, net, self.incep_batch_size, 10, verbose=True)
        print('Inception Score | mean:', '%.2f' % mean, 'std:', '%.2f' % std)
        return dict(mean=mean, std=std, indices=indices, samples=samples)

    def evaluate_fid(self):
        """-> dict(fid, mu_gen, sigma_gen, mu_real, sigma_real, samples)."""
        import os
        net = self._inception()
        path = self.cfg.EVAL.ACT_STAT_PATH
        if not os.path.exists(path):
            print('Computing activation statistics for real x')
            fid.compute_and_save_activation_statistics(self.cfg.EVAL.R_IMG_PATH, net, self.incep_batch_size, path,
                                                       self.model.device, verbose=True)
        print('Loading activation statistics for the real x')
        mu_real, sigma_real = fid.load_activation_statistics(path)
        self._restore_generator()
        print('Generating x...')
        samples = self._generate(is_training=True)
        print('Computing activation statistics for generated x...')
        mu_gen, sigma_gen = fid.calculate_activation_statistics(samples, net, self.incep_batch_size, verbose=True)
        print('calculate FID:', end=' ', flush=True)
        try:
            value = fid.calculate_frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)
        except Exception as e:          # the reference's fallback
            print(e)
            value = 500
        print(value)
        return dict(fid=value, mu_gen=mu_gen, sigma_gen=sigma_gen, mu_real=mu_real, sigma_real=sigma_real, samples=samples)
