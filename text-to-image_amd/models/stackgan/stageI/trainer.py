"""ConditionalGanTrainer (Stage-I) — reference models/stackgan/stageI/trainer.py:11-165: sigmoid cross-entropy losses
(real label 0.9), KL term of the conditioning augmentation, two Adam optimizers on ONE learning-rate placeholder
(D_LR * 0.5 ** (epoch // 100)), both under tf.GraphKeys.UPDATE_OPS, D update then G update every iteration."""
import sys
import time

import torch

from .... import kernels as K
from ....graphs import StepGraphs
from ....utils.ops import update_ops
from ...cgan_trainer import CGanTrainer


class ConditionalGanTrainer(CGanTrainer):
    REAL_LABEL = 0.9                     # trainer.py:26 (Stage-II overrides with 0.95)

    def __init__(self, sess, model, dataset, cfg):
        self.lr = float(cfg.TRAIN.D_LR)
        self.kl_coeff = float(cfg.TRAIN.COEFF.KL)
        super().__init__(sess, model, dataset, cfg)

    @staticmethod
    def kl_loss(mean, log_sigma):
        return (-log_sigma + 0.5 * (-1.0 + torch.exp(2.0 * log_sigma) + mean * mean)).mean()

    # what the model's generator consumes differs per stage (Stage-II feeds the Stage-I image): one hook
    def _generate(self, feed, which):
        m = self.model
        return m.generator(feed['z'], feed['phi_inputs'], reuse=True, noise=feed.get('ca_noise_' + which))

    def d_losses(self, feed):
        """What sess.run([D_optim, ...]) evaluates before the update (trainer.py:19-41).  Gradients -> d_arena."""
        with update_ops(), torch.no_grad():
            G, _, _ = self._generate(feed, 'd')
        d, heads, _ = self.critic_step(feed, G, want_prob=False)      # the three heads: trainer.py:24-33
        # the three critic outputs (fake, match, mismatch logits) ride along for the D summary's histograms (trainer.py:59-61)
        d['D_logits'] = heads
        return d

    def g_losses(self, feed):
        with update_ops():
            G, mean, log_sigma = self._generate(feed, 'g')
        # G_loss = CE(fake, 1) + kl_coeff * KL (trainer.py:35-41,50-55): the KL term stays a differentiable tensor expression, seeded with
        # kl_coeff next to the CE head's d/d logits
        G_kl_loss = self.kl_loss(mean, log_sigma)
        G_gan_loss = self.generator_step(feed, G, [G_kl_loss], [torch.full_like(G_kl_loss, self.kl_coeff)])[1]
        G_loss = G_gan_loss + self.kl_coeff * G_kl_loss.detach()
        return dict(G_loss=G_loss, G_gan_loss=G_gan_loss, G_kl_loss=G_kl_loss.detach(), G=G.detach())

    NOISE_KEYS = ('ca_noise_d', 'ca_noise_g')

    def enable_graphs(self, feed):
        """Capture the two halves into hipGraphs and replay them from then on, cut at the exchange under data parallelism
        (graphs.DGSchedule.capture).  Call after at least one eager iteration with the same shapes.  The conditioning-augmentation
        noise lives in static buffers that are re-drawn before every replay (the reference draws it inside the graph on every run)."""
        m = self.model
        feed = dict(feed)
        for k in self.NOISE_KEYS:
            if feed.get(k) is None:
                feed[k] = torch.empty(feed['z'].shape[0], self._noise_dim(k), device=m.device)
        self._graphs = StepGraphs(feed, ('inputs', 'wrong_inputs', 'phi_inputs', 'z') + tuple(self.NOISE_KEYS),
                                  filters=(m.d_arena.flat, m.g_arena.flat))
        self._draw_noise(feed)
        self._graphs.load(feed)
        self.schedule.capture(self._graphs)

    def _noise_dim(self, key):
        return self.model.compressed_embed_dim

    def _draw_noise(self, feed):
        for k in self.NOISE_KEYS:
            if feed.get(k) is None or feed[k] is self._graphs.static.get(k):
                K.trunc_normal_(self._graphs.static[k])

    def iteration(self, feed, epoch=0):
        lr = self.lr * (0.5 ** (epoch // 100))                       # trainer.py:119,127
        if self._graphs is not None:
            self._draw_noise(feed)
        return self.schedule.run(feed, lr, lr, graphs=self._graphs)

    def write_summaries(self, counter, out):
        """The two merged summaries the reference adds per update (trainer.py:72-85,134-141).  D: histograms of the three critic
        outputs (the sigmoid of the logits: model.D_synthetic / D_real_match / D_real_mismatch), scalars of the three loss terms and
        d_loss; G: image g_sum, scalars g_loss / g_gan_loss / g_kl_loss (z_sum is defined by the reference but merged into neither) —
        from the values the iteration computed, as the reference fetches them in the same sess.run as the optimizer steps."""
        from ....utils import summary as S
        np_ = lambda t: t.detach().float().cpu().numpy()
        d, g = out['d'], out['g']
        prob = [np_(torch.sigmoid(l_)) for l_ in d['D_logits']]           # fake, match, mismatch
        self.writer.add_summary([S.histogram('d_real_mismatch_sum', prob[2]), S.histogram('d_real_match_sum', prob[1]),
                                 S.histogram('d_synthetic_sum', prob[0]), S.scalar('d_synthetic_sum_loss', float(d['D_synthetic_loss'])),
                                 S.scalar('d_real_mismatch_sum_loss', float(d['D_real_mismatch_loss'])),
                                 S.scalar('d_real_match_sum_loss', float(d['D_real_match_loss'])), S.scalar('d_loss', float(d['D_loss']))], counter)
        self.writer.add_summary([S.image('g_sum', np_(g['G'])), S.scalar('g_loss', float(g['G_loss'])),
                                 S.scalar('g_gan_loss', float(g['G_gan_loss'])), S.scalar('g_kl_loss', float(g['G_kl_loss']))], counter)
        self.writer.flush()

    # the reference's periods (stageI/trainer.py:151,163): a sample grid when counter % 500 == 0, a checkpoint when
    # counter % 500 == 0.  TRAIN.SAMPLE_PERIOD / TRAIN.CHECKPOINT_PERIOD override the periods; the phase stays
    SAMPLE_PERIOD, CHECKPOINT_PERIOD, CHECKPOINT_PHASE = 500, 500, 0

    def make_savers(self):
        """-> (the saver the run resumes from and saves to, [(saver, dir, loaded message, failed message)] to restore first).
        Stage I: tf.train.Saver() built before the optimizers (trainer.py:46) holds every variable of g_net and d_net, batch-norm
        moving statistics included, and no Adam slot: a resumed run restarts Adam from zero."""
        from ....utils.saver import Saver
        saver = Saver(self.model.store, var_list=[self.model.g_scope, self.model.d_scope],
                      max_to_keep=int(self.cfg.TRAIN.CHECKPOINTS_TO_KEEP))
        return saver, [(saver, self.cfg.CHECKPOINT_DIR, ' [*] Load SUCCESS', ' [!] Load failed...')]

    def _period(self, key, default):
        p = int(getattr(self.cfg.TRAIN, key, None) or default)
        if p <= 0:
            raise ValueError('TRAIN.%s must be positive, got %d' % (key, p))
        return p

    def train(self, max_updates=None, log=None, summaries=False, side_effects=False, graphs=False):
        """summaries=True: an event file in cfg.LOGS_DIR with the reference's per-update summaries (write_summaries).
        side_effects=True: the rest of reference trainer.py:95-165 — sample_z, then the fixed test batch and its captions
        (SAMPLE_DIR/captions.txt); resume from the latest checkpoint (counter from its name, epoch_start = counter //
        updates_per_epoch, idx from 0); a sampler grid `train_{epoch:02d}_{idx:04d}.png` and a checkpoint on the periods above.
        max_updates: updates run by this call.  graphs=True: the iteration is replayed from hipGraphs after its first eager run."""
        import numpy as np
        log = log or (lambda s: (sys.stdout.write(s + '\n'), sys.stdout.flush()))
        m = self.model
        if summaries and getattr(self.cfg, 'LOGS_DIR', None):
            self.define_summaries()
        counter = 1
        epoch_start = 0
        updates_per_epoch = self.dataset.train.num_examples // m.batch_size
        if side_effects:
            from ....utils.saver import load, save
            from ....utils.utils import get_balanced_factorization, save_captions, save_images
            sample_period = self._period('SAMPLE_PERIOD', self.SAMPLE_PERIOD)
            ckpt_period = self._period('CHECKPOINT_PERIOD', self.CHECKPOINT_PERIOD)
            self.saver, restores = self.make_savers()
            sample_z = np.random.normal(0, 1, (m.sample_num, m.z_dim))
            _, sample_embed, _, captions = self.dataset.test.next_batch_test(m.sample_num, 0, 1)
            sample_z = torch.as_tensor(sample_z, dtype=torch.float32).to(m.device)
            sample_embed = torch.as_tensor(sample_embed[0]).to(device=m.device, dtype=torch.float32).reshape(m.sample_num, -1)
            save_captions(self.cfg.SAMPLE_DIR, captions)
            for i, (saver, directory, ok, failed) in enumerate(restores):
                could_load, checkpoint_counter = load(saver, None, directory)
                if i == 0 and could_load:
                    counter = checkpoint_counter
                log(ok if could_load else failed)
            if updates_per_epoch <= 0:
                raise ValueError('the training split has %d examples, fewer than one batch of %d' % (
                    self.dataset.train.num_examples, m.batch_size))
            epoch_start = counter // updates_per_epoch
            self.start_counter, self.epoch_start = counter, epoch_start
        t0, done = time.time(), 0
        for epoch in range(epoch_start, self.cfg.TRAIN.EPOCH):
            for idx in range(updates_per_epoch):
                feed = self.make_feed()
                out = self.iteration(feed, epoch)
                if graphs and self._graphs is None:
                    self.enable_graphs(feed)
                if getattr(self, 'writer', None) is not None:
                    self.write_summaries(counter, out)
                counter += 1
                done += 1
                log('Epoch: [%2d] [%4d/%4d] time: %4.4f, d_loss: %.8f, g_loss: %.8f' % (
                    epoch, idx, updates_per_epoch, time.time() - t0, float(out['d']['D_loss']), float(out['g']['G_loss'])))
                if side_effects:
                    if counter % sample_period == 0:
                        save_images(m.sampler(sample_z, sample_embed), get_balanced_factorization(m.sample_num),
                                    '{}train_{:02d}_{:04d}.png'.format(self.cfg.SAMPLE_DIR, epoch, idx))
                    if counter % ckpt_period == self.CHECKPOINT_PHASE % ckpt_period:
                        save(self.saver, None, self.cfg.CHECKPOINT_DIR, counter)
                if max_updates is not None and done >= max_updates:
                    return
