"""ConditionalGanTrainer (Stage-II) — reference models/stackgan/stageII/trainer.py:11-177.  Same losses and schedule as
Stage-I with real label 0.95 (trainer.py:27); the generator input is the Stage-I generator's image, produced inside the
same run in training mode with frozen weights (stageII/model.py:50)."""
import torch

from ..stageI.trainer import ConditionalGanTrainer as _StageITrainer


class ConditionalGanTrainer(_StageITrainer):
    REAL_LABEL = 0.95
    NOISE_KEYS = ('ca_noise_d', 'ca_noise_g', 'ca_noise_d_s1', 'ca_noise_g_s1')

    def _noise_dim(self, key):
        return self.model.stagei.compressed_embed_dim if key.endswith('_s1') else self.model.compressed_embed_dim

    def __init__(self, sess, model, dataset, cfg, cfg_stage_i=None):
        self.cfg_stage_i = cfg_stage_i
        super().__init__(sess, model, dataset, cfg)

    # reference stageII/trainer.py:162,176: a sample grid when counter % 2000 == 0, a checkpoint when counter % 500 == 2
    SAMPLE_PERIOD, CHECKPOINT_PERIOD, CHECKPOINT_PHASE = 2000, 500, 2

    def make_savers(self):
        """stageII/trainer.py:44-49,107-121: the checkpoints hold stageII_g_net + stageII_d_net only; the Stage-I generator (g_net)
        is restored from cfg_stage_i.CHECKPOINT_DIR, and a failed load there only warns."""
        from ....utils.saver import Saver
        m = self.model
        saver = Saver(m.store, var_list=[m.g_scope, m.d_scope], max_to_keep=int(self.cfg.TRAIN.CHECKPOINTS_TO_KEEP))
        restores = [(saver, self.cfg.CHECKPOINT_DIR, ' [*] Load SUCCESS: Stage II networks are loaded.',
                     ' [!] Load failed for stage II networks...')]
        if self.cfg_stage_i is not None:
            restores.append((Saver(m.store, var_list=[m.stagei.g_scope]), self.cfg_stage_i.CHECKPOINT_DIR,
                             ' [*] Load SUCCESS: Stage I generator is loaded',
                             ' [!] WARNING!!! Failed to load the parameters for stage I generator...'))
        return saver, restores

    def _generate(self, feed, which):
        m = self.model
        with torch.no_grad():      # Stage-I variables are in no var_list; under update_ops() its BN moving averages move
            img64, _, _ = m.stagei.generator(feed['z'], feed['phi_inputs'], reuse=True, noise=feed.get('ca_noise_%s_s1' % which))
        return m.generator(img64, feed['phi_inputs'], reuse=True, noise=feed.get('ca_noise_' + which))
