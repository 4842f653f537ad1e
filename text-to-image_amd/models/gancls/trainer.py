"""GanClsTrainer — reference models/gancls/trainer.py:12-164: losses, the two Adam optimizers (both under UPDATE_OPS), the
D-then-G update order of every iteration and, behind train(side_effects=True), the loop's side effects: sampled captions, sample
grids, checkpoints and resume."""
import sys
import time

import torch

from ... import autograd as A
from ... import stacked as ST
from ... import kernels as K
from ... import optim
from ...utils.ops import update_ops


class GanClsTrainer(object):
    batched = True      # the critic's passes of one sess.run are one stacked batch (always: the unstacked forms are gone)

    def __init__(self, sess, model, dataset, cfg):
        self.sess, self.model, self.dataset, self.cfg = sess, model, dataset, cfg     # sess unused (no TF session)
        self.gen = torch.Generator(device=model.device).manual_seed(1234)
        # The D run and the G run of one iteration evaluate the generator on the SAME feed (trainer.py:115-134: same z, same phi), the generator
        # has no noise input (model.py:111-192) and D_optim does not touch its variables: the two evaluations are the same numbers.  iteration()
        # therefore evaluates it ONCE (with the autograd graph the G run needs), hands the critic step a detached view, and lets the batch norms'
        # moving averages take the batch statistics twice, as the two runs under UPDATE_OPS do (update_ops(times=2)).  Single process only: under
        # data parallelism the two halves live in separately captured graph segments.  share_g = False: evaluate twice.
        self.share_g = True
        self._shared_G = None
        self.define_losses()

    def define_losses(self):
        t = self.cfg.TRAIN
        self.alpha = float(t.COEFF.ALPHA_MISMATCH_LOSS)
        self.D_optim = optim.AdamTF(self.model.d_arena, float(t.D_BETA_DECAY), 0.999)
        self.G_optim = optim.AdamTF(self.model.g_arena, float(t.G_BETA_DECAY), 0.999)

    def d_losses(self, feed, keep_g=False):
        """What sess.run([D_optim, ...]) evaluates before the update (trainer.py:20-34,115-123).  Gradients -> d_arena.
        keep_g (iteration() only): the generator is evaluated with its autograd graph and its moving averages move twice; the result is kept
        for g_losses(G=...) of the same iteration (see __init__)."""
        m = self.model
        x, xw, phi, z = feed['inputs'], feed['wrong_inputs'], feed['phi_inputs'], feed['z']
        if keep_g:
            with update_ops(times=2):
                self._shared_G = m.generator(z, phi, reuse=True)
            G = self._shared_G.detach()
        with update_ops():      # D_optim is built under control_dependencies(UPDATE_OPS): every BN moving average moves
            if not keep_g:
                with torch.no_grad():
                    G = m.generator(z, phi, reuse=True)
            # the critic's three passes (fake / match / mismatch, model.py:48-51) as ONE stacked batch: per-sample layers run once on 3B
            # samples, every batch norm keeps its statistics per pass (discriminator(groups=3))
            _, logits = m.discriminator(torch.cat([G, x, xw], 0), torch.cat([phi, phi, phi], 0), reuse=True, _prob=False, groups=3)
            B = x.shape[0]
            lv = logits.detach().reshape(3, B)
            seed = torch.empty(3 * B, dtype=torch.float32, device=logits.device)
        # the three heads of trainer.py:20-34 in ONE launch (labels 0 / 0.9 one-sided smoothing / 0; D_loss = match + alpha mismatch +
        # (1 - alpha) fake): the loss scalars, d D_loss / d logits as the seeds of the backward pass, and the sigmoid outputs
        losses, _, probs = K.sigmoid_ce_head(list(lv), [0.0, 0.9, 0.0], [1.0 - self.alpha, 1.0, self.alpha], seeds_into=seed)
        m.d_arena.zero_grad()
        if m.dp is not None and not getattr(self, '_capturing', False):
            m.dp.arm(m.d_arena)
        torch.autograd.backward([logits], [seed.view_as(logits)], inputs=list(m.d_vars.values()))
        A.side_join()
        shape = (x.shape[0], 1, 1, 1)
        return dict(D_loss=losses[0], D_real_match_loss=losses[2], D_real_mismatch_loss=losses[3], D_synthetic_loss=losses[1], G=G,
                    D_synthetic=probs[0].view(shape), D_real_match=probs[1].view(shape), D_real_mismatch=probs[2].view(shape))

    def g_losses(self, feed, G=None):
        """G: the generator output d_losses(keep_g=True) evaluated for this iteration (with its autograd graph), or None: evaluate it here."""
        m = self.model
        x, xw, phi, z = feed['inputs'], feed['wrong_inputs'], feed['phi_inputs'], feed['z']
        with update_ops():
            if G is None:
                G = m.generator(z, phi, reuse=True)
            # G_optim also sits under ALL update ops of the graph: the match / mismatch critic passes run in this
            # sess.run too, only to move their batch-norm moving averages (trainer.py:46-51)
            if x.is_cuda:
                # round 6: fake | match | mismatch as ONE stacked pass of three evaluations (stacked.py): every conv once on 3B rows, per-evaluation
                # batch-norm statistics, the moving averages move once per evaluation in this order (as the three calls did); only the fake rows
                # carry a gradient, so the backward runs on B rows as before
                with m.store.frozen('d_net'):
                    _, ls = m.discriminator(ST.Stacked(G, torch.cat([x, xw], 0)), ST.Stacked(phi, torch.cat([phi, phi], 0)), reuse=True, _prob=False,
                                            groups=3)
                l_fake = ls.main
            else:
                with m.store.frozen('d_net'):
                    _, l_fake = m.discriminator(G, phi, reuse=True, _prob=False)
                with torch.no_grad():
                    m.discriminator(torch.cat([x, xw], 0), torch.cat([phi, phi], 0), reuse=True, _prob=False, groups=2)
        losses, seeds, _ = K.sigmoid_ce_head([l_fake.detach().reshape(-1)], [1.0], [1.0], want_prob=False)      # G_loss: label 1 (trainer.py:36)
        m.g_arena.zero_grad()
        if m.dp is not None and not getattr(self, '_capturing', False):
            m.dp.arm(m.g_arena)
        torch.autograd.backward([l_fake], [seeds[0].view_as(l_fake)], inputs=list(m.g_vars.values()))
        A.side_join()
        return dict(G_loss=losses[0], G=G.detach())

    # ---- device-only halves of an iteration (graph-capturable) ------------------------------------------------------------
    def _d_body(self, feed, keep_g=False, refresh=None):
        m = self.model
        d = self.d_losses(feed, keep_g=keep_g)
        scale = m.dp.allreduce_arena(m.d_arena) if m.dp is not None else 1.0
        self.D_optim.apply(grad_scale=scale, refresh=refresh)
        return d

    def _g_body(self, feed, G=None):
        m = self.model
        g = self.g_losses(feed, G=G)
        scale = m.dp.allreduce_arena(m.g_arena) if m.dp is not None else 1.0
        self.G_optim.apply(grad_scale=scale)
        return g

    def _dg_body(self, feed):
        """Both halves with ONE generator evaluation (see __init__); the critic's cached filter images are regenerated behind its Adam step,
        because the generator half of the same capture reads the updated filters."""
        d = self._d_body(feed, keep_g=True, refresh=True)
        G, self._shared_G = self._shared_G, None
        return d, self._g_body(feed, G=G)

    def enable_graphs(self, feed):
        """Capture the iteration into hipGraphs and replay it from then on (call after one eager iteration): one graph for both halves when
        the generator evaluation is shared (single process), else one per half.  With data parallelism each half is cut at its exchange step —
        [losses + backward] | all-reduce of the gradient arena, issued eagerly | [Adam] — as in models/wgancls and models/stackgan: no
        collective is ever captured."""
        from ...graphs import StepGraphs
        m = self.model
        self._graphs = StepGraphs(feed, ('inputs', 'wrong_inputs', 'phi_inputs', 'z'), filters=(m.d_arena.flat, m.g_arena.flat))
        if m.dp is None:
            if self.share_g:
                self._graphs.capture('dg', self._dg_body)
            else:
                self._graphs.capture('d', self._d_body)
                self._graphs.capture('g', self._g_body)
            return
        scale = 1.0 / m.dp.world
        self._capturing = True
        try:
            self._graphs.capture('d', self.d_losses, capture_error_mode='thread_local')
            self._graphs.capture('d_upd', lambda f: self.D_optim.apply(grad_scale=scale), capture_error_mode='thread_local', refresh=False)
            self._graphs.capture('g', self.g_losses, capture_error_mode='thread_local')
            self._graphs.capture('g_upd', lambda f: self.G_optim.apply(grad_scale=scale), capture_error_mode='thread_local', refresh=False)
        finally:
            self._capturing = False

    def iteration(self, feed):
        lr_d, lr_g = float(self.cfg.TRAIN.D_LR), float(self.cfg.TRAIN.G_LR)
        graphs = getattr(self, '_graphs', None)
        dp = self.model.dp
        if graphs is not None:
            graphs.load(feed)
            if 'dg' in graphs.graphs:
                self.D_optim.prepare(lr_d)
                self.G_optim.prepare(lr_g)
                d, g = graphs.replay('dg')
                return {'d': d, 'g': g}
            self.D_optim.prepare(lr_d)
            d = graphs.replay('d')
            if dp is not None:
                dp.allreduce_arena(self.model.d_arena)
                graphs.replay('d_upd')
            self.G_optim.prepare(lr_g)
            g = graphs.replay('g')
            if dp is not None:
                dp.allreduce_arena(self.model.g_arena)
                graphs.replay('g_upd')
            return {'d': d, 'g': g}
        if self.share_g and dp is None:
            self.D_optim.prepare(lr_d)
            self.G_optim.prepare(lr_g)
            d, g = self._dg_body(feed)
            return {'d': d, 'g': g}
        self.D_optim.prepare(lr_d)
        d = self._d_body(feed)
        self.G_optim.prepare(lr_g)
        return {'d': d, 'g': self._g_body(feed)}

    def make_feed(self):
        m = self.model
        images, wrong_images, embed, _, _ = self.dataset.train.next_batch(m.batch_size, 4, embeddings=True, wrong_img=True)
        return {'inputs': images, 'wrong_inputs': wrong_images, 'phi_inputs': embed,
                'z': torch.randn((m.batch_size, m.z_dim), generator=self.gen, device=m.device)}

    def define_summaries(self):
        """reference trainer.py:53-75: the FileWriter on cfg.LOGS_DIR (utils/summary.py: TensorBoard event files without TensorFlow)."""
        from ...utils.summary import FileWriter
        self.writer = FileWriter(self.cfg.LOGS_DIR)

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
                if graphs and getattr(self, '_graphs', None) is None:
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
