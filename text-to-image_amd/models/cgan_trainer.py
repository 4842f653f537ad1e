"""What the sigmoid-cross-entropy conditional-GAN trainers share (models/gancls and models/stackgan, reference
models/gancls/trainer.py and models/stackgan/stage{I,II}/trainer.py): the critic step and the generator step around the stacked
critic pass, the two Adam optimizers under UPDATE_OPS, the D-then-G schedule (graphs.DGSchedule), the feed and the event writer.
How the fake image is made, the real label, what rides along in the results, the summaries, the savers and the train() loop are
each trainer's own."""
import torch

from .. import stacked as ST
from .. import kernels as K
from .. import optim
from ..graphs import DGSchedule
from ..utils.ops import update_ops


class CGanTrainer(object):
    batched = True      # the critic's passes of one sess.run are one stacked batch (always: the unstacked forms are gone)
    # REAL_LABEL: the one-sided label smoothing of the match head, each trainer's own

    def __init__(self, sess, model, dataset, cfg):
        self.sess, self.model, self.dataset, self.cfg = sess, model, dataset, cfg     # sess unused (no TF session)
        self.gen = torch.Generator(device=model.device).manual_seed(1234)
        self._graphs = None               # a graphs.StepGraphs once enable_graphs() has run; None: eager
        self.define_losses()

    def define_losses(self):
        t, m = self.cfg.TRAIN, self.model
        self.alpha = float(t.COEFF.ALPHA_MISMATCH_LOSS)
        self.D_optim = optim.AdamTF(m.d_arena, float(t.D_BETA_DECAY), 0.999)
        self.G_optim = optim.AdamTF(m.g_arena, float(t.G_BETA_DECAY), 0.999)
        self.schedule = DGSchedule(m.dp, self.d_losses, m.d_arena, self.D_optim, self.g_losses, m.g_arena, self.G_optim)

    def critic_step(self, feed, G, want_prob):
        """The critic's half of what sess.run([D_optim, ...]) evaluates before the update, from the fake image G (no gradient into
        it).  Gradients -> d_arena.  -> (the four loss scalars and G as a dict, the logits of the three heads fake / match /
        mismatch, their sigmoids or None)"""
        m = self.model
        x, xw, phi = feed['inputs'], feed['wrong_inputs'], feed['phi_inputs']
        with update_ops():      # D_optim is built under control_dependencies(UPDATE_OPS): every BN moving average moves
            # the critic's three passes (fake / match / mismatch) as ONE stacked batch: per-sample layers run once on 3B
            # samples, every batch norm keeps its statistics per pass (discriminator(groups=3))
            _, logits = m.discriminator(torch.cat([G, x, xw], 0), torch.cat([phi, phi, phi], 0), reuse=True, _prob=False, groups=3)
            B = x.shape[0]
            heads = list(logits.detach().reshape(3, B))
            seed = torch.empty(3 * B, dtype=torch.float32, device=logits.device)
        # the three heads in ONE launch (labels 0 / REAL_LABEL / 0; D_loss = match + alpha mismatch + (1 - alpha) fake): the loss
        # scalars, d D_loss / d logits as the seeds of the backward pass and, if wanted, the sigmoid outputs
        losses, _, probs = K.sigmoid_ce_head(heads, [0.0, self.REAL_LABEL, 0.0], [1.0 - self.alpha, 1.0, self.alpha], want_prob=want_prob,
                                             seeds_into=seed)
        self.schedule.backward(m.d_arena, [logits], [seed.view_as(logits)], m.d_vars.values())
        return dict(D_loss=losses[0], D_real_match_loss=losses[2], D_real_mismatch_loss=losses[3], D_synthetic_loss=losses[1], G=G), heads, probs

    def generator_step(self, feed, G, extra_roots=(), extra_seeds=()):
        """The generator's half from the fake image G (with its autograd graph): CE(D(G), 1) and its gradient, together with
        the gradients of extra_roots seeded by extra_seeds, -> g_arena.  -> the head's loss scalars [total, CE]"""
        m = self.model
        x, xw, phi = feed['inputs'], feed['wrong_inputs'], feed['phi_inputs']
        with update_ops():
            # G_optim also sits under ALL update ops of the graph: the match / mismatch critic passes run in this
            # sess.run too, only to move their batch-norm moving averages
            if x.is_cuda:
                # fake | match | mismatch as ONE stacked pass of three evaluations (stacked.py): every conv once on 3B rows, per-evaluation
                # batch-norm statistics, the moving averages move once per evaluation in this order (as the three calls did); only the fake rows
                # carry a gradient, so the backward runs on B rows as before
                with m.store.frozen(m.d_scope):
                    _, ls = m.discriminator(ST.Stacked(G, torch.cat([x, xw], 0)), ST.Stacked(phi, torch.cat([phi, phi], 0)), reuse=True, _prob=False,
                                            groups=3)
                l_fake = ls.main
            else:
                with m.store.frozen(m.d_scope):
                    _, l_fake = m.discriminator(G, phi, reuse=True, _prob=False)
                with torch.no_grad():
                    m.discriminator(torch.cat([x, xw], 0), torch.cat([phi, phi], 0), reuse=True, _prob=False, groups=2)
        # label 1: the CE head gives its value and d/d logits; extra roots stay differentiable tensor expressions, seeded together with it
        losses, seeds, _ = K.sigmoid_ce_head([l_fake.detach().reshape(-1)], [1.0], [1.0], want_prob=False)
        self.schedule.backward(m.g_arena, [l_fake] + list(extra_roots), [seeds[0].view_as(l_fake)] + list(extra_seeds), m.g_vars.values())
        return losses

    def make_feed(self):
        m = self.model
        images, wrong_images, embed, _, _ = self.dataset.train.next_batch(m.batch_size, 4, embeddings=True, wrong_img=True)
        return {'inputs': images, 'wrong_inputs': wrong_images, 'phi_inputs': embed,
                'z': torch.randn((m.batch_size, m.z_dim), generator=self.gen, device=m.device)}

    def define_summaries(self):
        """The reference's FileWriter on cfg.LOGS_DIR (utils/summary.py: TensorBoard event files without TensorFlow)."""
        from ..utils.summary import FileWriter
        self.writer = FileWriter(self.cfg.LOGS_DIR)
