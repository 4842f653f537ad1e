"""StageIEval — reference models/stackgan/stageI/eval_stagei.py, which is models/wgancls/eval_wgan.py with the class count taken
from EVAL.NUM_CLASSES.  evaluate_inception / evaluate_fid are WGanClsEval's (the Stage-I generator lives under `g_net` with the
wgancls generator's signature): IS with the generator in eval mode, shuffled scoring and 10 splits; FID with is_training=True.

evaluate_imd is an addition the reference does not have: the Inception match distance (evaluation/imd.py) between each real test
image of `test.next_batch(bs, 4, embeddings=True)` and the image generated from that image's embedding (eval-mode batch norm;
z is drawn first, as in the other evaluations).  Per chunk of INCEP_BATCH_SIZE pairs, one resize of each half, one Inception
forward and one t2i_cosine_distance launch."""
import numpy as np
import torch

from ....evaluation import imd
from ...wgancls.eval_wgan import WGanClsEval


class StageIEval(WGanClsEval):
    def _generate_batch(self, z, cond, is_training):
        m = self.model
        img, _, _ = m.generator(z, cond, reuse=True, is_training=is_training)
        return img

    def _draw_batch(self, z_dim, embed_dim):
        """The reference's draws for one batch: z ~ N(0, 1) [bs, z_dim], then the test batch. -> (real images, z, embeddings) on
        the device."""
        dev = self.model.device
        sample_z = np.random.normal(0, 1, size=(self.bs, z_dim))
        images, _, embed, _, _ = self.dataset.test.next_batch(self.bs, 4, embeddings=True)
        z = torch.as_tensor(sample_z, dtype=torch.float32).to(dev)
        cond = embed if torch.is_tensor(embed) else torch.as_tensor(np.asarray(embed), dtype=torch.float32)
        cond = cond.to(device=dev, dtype=torch.float32).reshape(self.bs, embed_dim)
        real = images if torch.is_tensor(images) else torch.as_tensor(np.asarray(images, np.float32))
        return real.to(device=dev, dtype=torch.float32).contiguous(), z, cond

    def _n_batches(self):
        n_batches = self.cfg.EVAL.SIZE // self.bs
        if n_batches == 0:
            raise ValueError('EVAL.SIZE %d is smaller than EVAL.SAMPLE_SIZE %d' % (self.cfg.EVAL.SIZE, self.bs))
        return n_batches

    def _dims(self):
        return self.model.z_dim, self.model.embed_dim

    def evaluate_imd(self, keep_samples=False):
        """-> dict(mean, std, distances float64 [n]) and, with keep_samples, the host pairs (real, gen: float32 [n, H, W, 3] in
        [-1, 1])."""
        net = self._inception()
        self._restore_generator()
        n_batches = self._n_batches()
        c = self.incep_batch_size
        dists, kept_real, kept_gen = [], [], []
        print('Generating pairs...')
        for i in range(n_batches):
            print('\rGenerating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
            real, z, cond = self._draw_batch(*self._dims())
            with torch.no_grad():
                gen = self._generate_batch(z, cond, is_training=False).float().contiguous()
            for s in range(0, self.bs, c):
                dists.append(imd.pair_distances(real[s:s + c], gen[s:s + c], net))
            if keep_samples:
                kept_real.append(real.cpu().numpy())
                kept_gen.append(gen.cpu().numpy())
        print()
        d = torch.cat(dists).cpu().numpy()
        mean, std = float(np.mean(d)), float(np.std(d))
        print('IMD | mean: %.4f std: %.4f' % (mean, std))
        out = dict(mean=mean, std=std, distances=d)
        if keep_samples:
            out.update(real=np.concatenate(kept_real), gen=np.concatenate(kept_gen))
        return out
