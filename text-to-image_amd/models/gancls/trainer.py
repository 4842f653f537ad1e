"""GanClsTrainer — reference models/gancls/trainer.py:12-164: losses, the two Adam optimizers (both under UPDATE_OPS), the
D-then-G update order of every iteration and, behind train(side_effects=True), the loop's side effects: sampled captions, sample
grids, checkpoints and resume."""
import sys
import time

import torch

from ...graphs import StepGraphs
from ...utils.ops import update_ops
from ..cgan_trainer import CGanTrainer


class GanClsTrainer(CGanTrainer):
    REAL_LABEL = 0.9    # one-sided smoothing (trainer.py:24)

    def __init__(self, sess, model, dataset, cfg):
        # The D run and the G run of one iteration evaluate the generator on the SAME feed (trainer.py:115-134: same z, same phi), the generator
        # has no noise input (model.py:111-192) and D_optim does not touch its variables: the two evaluations are the same numbers.  iteration()
        # therefore evaluates it ONCE (with the autograd graph the G run needs), hands the critic step a detached view, and lets the batch norms'
        # moving averages take the batch statistics twice, as the two runs under UPDATE_OPS do (update_ops(times=2)).  Single process only: under
        # data parallelism the two halves live in separately captured graph segments.  share_g = False: evaluate twice.
        self.share_g = True
        self._shared_G = None
        super().__init__(sess, model, dataset, cfg)

    def d_losses(self, feed, keep_g=False):
        """What sess.run([D_optim, ...]) evaluates before the update (trainer.py:20-34,115-123; the critic passes: model.py:48-51).
        Gradients -> d_arena.
        keep_g (iteration() only): the generator is evaluated with its autograd graph and its moving averages move twice; the result is kept
        for g_losses(G=...) of the same iteration (see __init__)."""
        m = self.model
        if keep_g:
            with update_ops(times=2):
                self._shared_G = m.generator(feed['z'], feed['phi_inputs'], reuse=True)
            G = self._shared_G.detach()
        else:
            with update_ops(), torch.no_grad():
                G = m.generator(feed['z'], feed['phi_inputs'], reuse=True)
        d, _, probs = self.critic_step(feed, G, want_prob=True)
        shape = (G.shape[0], 1, 1, 1)
        d.update(D_synthetic=probs[0].view(shape), D_real_match=probs[1].view(shape), D_real_mismatch=probs[2].view(shape))
        return d

    def g_losses(self, feed, G=None):
        """G: the generator output d_losses(keep_g=True) evaluated for this iteration (with its autograd graph), or None: evaluate it here."""
        if G is None:
            with update_ops():
                G = self.model.generator(feed['z'], feed['phi_inputs'], reuse=True)
        losses = self.generator_step(feed, G)                     # G_loss: label 1 (trainer.py:36,46-51)
        return dict(G_loss=losses[0], G=G.detach())

    def _dg_body(self, feed):
        """Both halves with ONE generator evaluation (see __init__); the critic's cached filter images are regenerated behind its Adam step,
        because the generator half of the same capture reads the updated filters."""
        s = self.schedule
        d = s.step(s.d, feed, keep_g=True, refresh=True)
        G, self._shared_G = self._shared_G, None
        return d, s.step(s.g, feed, G=G)

    def _joint(self):
        """The one-body iteration, where it applies: single process only (under data parallelism the halves are separate segments)."""
        return self._dg_body if self.share_g and self.model.dp is None else None

    def enable_graphs(self, feed):
        """Capture the iteration into hipGraphs and replay it from then on (call after one eager iteration): one graph for both halves when
        the generator evaluation is shared (single process), else one per half, cut at the exchange under data parallelism
        (graphs.DGSchedule.capture)."""
        m = self.model
        self._graphs = StepGraphs(feed, ('inputs', 'wrong_inputs', 'phi_inputs', 'z'), filters=(m.d_arena.flat, m.g_arena.flat))
        self.schedule.capture(self._graphs, joint=self._joint())

    def iteration(self, feed):
        return self.schedule.run(feed, float(self.cfg.TRAIN.D_LR), float(self.cfg.TRAIN.G_LR), graphs=self._graphs, joint=self._joint())

    def write_summaries(self, counter, feed, out):
        """The two merged summaries the reference adds per update (trainer.py:66-72,115-134) — D: histograms of the three critic
        outputs and of the three loss terms, scalar d_loss; G: image g_sum, scalar g_loss (the reference defines a histogram z_sum but
        merges it into neither, so the event file has no 'z' tag) — from the values the iteration computed (the reference fetches
        them in the same sess.run as the optimizer steps)."""
        from ...utils import summary as S
        np_ = lambda t: t.detach().float().cpu().numpy()
        d, g = out['d'], out['g']
        self.writer.add_summary([S.histogram('d_real_mismatch_sum', np_(d['D_real_mismatch'])), S.histogram('d_real_match_sum', np_(d['D_real_match'])),
                                 S.histogram('d_synthetic_sum', np_(d['D_synthetic'])), S.histogram('d_synthetic_sum_loss', np_(d['D_synthetic_loss'])),
                                 S.histogram('d_real_mismatch_sum_loss', np_(d['D_real_mismatch_loss'])),
                                 S.histogram('d_real_match_sum_loss', np_(d['D_real_match_loss'])), S.scalar('d_loss', float(d['D_loss']))], counter)
        self.writer.add_summary([S.image('g_sum', np_(g['G'])), S.scalar('g_loss', float(g['G_loss']))], counter)
        self.writer.flush()

    def make_saver(self):
        """tf.train.Saver(max_to_keep=CHECKPOINTS_TO_KEEP) built after the optimizers (reference trainer.py:41-51): every global variable
        under its tf.layers name — weights, batch-norm moving statistics, both optimizers' Adam slots and their step counts (from which
        beta1_power / beta2_power follow) — so that a resumed run continues bit for bit."""
        from ...utils.saver import Saver
        return Saver(self.model.store, {'D_optim': self.D_optim, 'G_optim': self.G_optim},
                     max_to_keep=int(getattr(self.cfg.TRAIN, 'CHECKPOINTS_TO_KEEP', 5)))

    # the reference's periods (trainer.py:141,163): a sampler grid when counter % 100 == 0, a checkpoint when counter % 500 == 2
    SAMPLE_PERIOD, CHECKPOINT_PERIOD, CHECKPOINT_PHASE = 100, 500, 2

    def train(self, max_updates=None, log=None, summaries=False, side_effects=False, graphs=False):
        """summaries=True: an event file in cfg.LOGS_DIR with the reference's per-update summaries (write_summaries).
        max_updates: updates run by this call.
        side_effects=True: the rest of reference trainer.py:83-164 — sample_z and the test window at a random position, its captions
        printed; resume from the latest checkpoint of cfg.CHECKPOINT_DIR (counter from its name); the sampler's 8 x 8 grid
        `SAMPLE_DIR/train_{epoch:02d}_{idx:04d}.png` when counter % 100 == 0 (outside any captured graph); a checkpoint when
        counter % 500 == 2; the log line every update instead of every tenth.
        graphs=True: the iteration is replayed from a hipGraph after its first eager run."""
        log = log or (lambda s: (sys.stdout.write(s + '\n'), sys.stdout.flush()))
        m = self.model
        if summaries and getattr(self.cfg, 'LOGS_DIR', None):
            self.define_summaries()
        counter = 1
        if side_effects:
            from random import randint
            import numpy as np
            from ...utils.saver import load, save
            from ...utils.utils import get_balanced_factorization, save_images
            sample_z = np.random.normal(0, 1, size=(m.sample_num, m.z_dim))
            _, sample_embed, _, captions = self.dataset.test.next_batch_test(m.sample_num, randint(0, self.dataset.test.num_examples), 1)
            sample_z = torch.as_tensor(sample_z, dtype=torch.float32).to(m.device)
            sample_embed = torch.as_tensor(sample_embed[0]).to(device=m.device, dtype=torch.float32).reshape(m.sample_num, -1)
            log(str(tuple(sample_embed.shape)))

            def log_captions():
                log('\nCaptions of the sampled x:')
                for caption_idx, caption_batch in enumerate(captions):
                    log('{}: {}'.format(caption_idx + 1, caption_batch[0]))
                log('')
            log_captions()
            self.saver = self.make_saver()
            could_load, checkpoint_counter = load(self.saver, None, self.cfg.CHECKPOINT_DIR)
            if could_load:
                counter = checkpoint_counter
            log(' [*] Load SUCCESS' if could_load else ' [!] Load failed...')
            self.start_counter = counter
        t0, done, out = time.time(), 0, None
        for epoch in range(self.cfg.TRAIN.EPOCH):
            updates_per_epoch = self.dataset.train.num_examples // m.batch_size
            for idx in range(updates_per_epoch):
                feed = self.make_feed()
                out = self.iteration(feed)
                if graphs and self._graphs is None:
                    self.enable_graphs(feed)
                if getattr(self, 'writer', None) is not None:
                    self.write_summaries(counter, feed, out)
                if not side_effects and counter % 10 == 0:
                    log('Epoch: [%2d] [%4d/%4d] time: %4.4f, d_loss: %.8f, g_loss: %.8f' % (
                        epoch, idx, updates_per_epoch, time.time() - t0, float(out['d']['D_loss']), float(out['g']['G_loss'])))
                counter += 1
                done += 1
                if side_effects:
                    err_d, err_g = float(out['d']['D_loss']), float(out['g']['G_loss'])
                    log('Epoch: [%2d] [%4d/%4d] time: %4.4f, d_loss: %.8f, g_loss: %.8f' % (
                        epoch, idx, updates_per_epoch, time.time() - t0, err_d, err_g))
                    if counter % self.SAMPLE_PERIOD == 0:
                        save_images(m.sampler(sample_z, sample_embed), get_balanced_factorization(m.sample_num),
                                    '{}train_{:02d}_{:04d}.png'.format(self.cfg.SAMPLE_DIR, epoch, idx))
                        log('[Sample] d_loss: %.8f, g_loss: %.8f' % (err_d, err_g))
                        log_captions()
                    if counter % self.CHECKPOINT_PERIOD == self.CHECKPOINT_PHASE:
                        save(self.saver, None, self.cfg.CHECKPOINT_DIR, counter)
                if max_updates is not None and done >= max_updates:
                    return out
        return out
