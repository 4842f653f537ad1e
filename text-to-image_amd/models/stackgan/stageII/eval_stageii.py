"""StageIIEval — reference models/stackgan/stageII/eval_stageii.py: the images come from the chain Stage-I generator -> Stage-II
generator.  `g_net` is restored from the Stage-I config's CHECKPOINT_DIR and `stageII_g_net` from the Stage-II one; a failed
load raises with the reference's message.  The 256 x 256 images are streamed (evaluation/evaluator.py).

- evaluate_inception: both generators in eval mode, each batch of EVAL.SAMPLE_SIZE scored in one Inception call.
- evaluate_fid: the reference's version feeds z to the Stage-II generator and keeps only the last batch, so it cannot run.  Here
  it is the same chain with both generators in training mode (is_training=True: the default argument eval_wgan keeps), the
  PreLogits statistics streamed over every image of every batch in chunks of the Inception batch.
- evaluate_imd: on the chain in eval mode, against the 256 x 256 test images."""
import torch

from ....utils.saver import restore_scopes
from ..stageI.eval_stagei import StageIEval

STAGES = {'g_net': 'stage I', 'stageII_g_net': 'stage II'}


def restore_chain(m, directory, batch, error):
    """`g_net` from the Stage-I config's CHECKPOINT_DIR, then `stageII_g_net` from `directory`; a launch-free pass through the
    chain creates the variables the model does not have.  error('stage I' | 'stage II') -> the exception of a failed load."""
    s1 = m.stagei

    def create():
        z = torch.empty(batch, s1.z_dim, device=m.device)
        phi = torch.empty(batch, s1.embed_dim, device=m.device)
        img64, _, _ = s1.generator(z, phi, reuse=bool(m.store.trainable_variables('g_net')), is_training=False)
        m.generator(img64, phi, reuse=False, is_training=False)
    restore_scopes(m.store, [('g_net', s1.cfg.CHECKPOINT_DIR), ('stageII_g_net', directory)], create, lambda scope: error(STAGES[scope]))


class StageIIEval(StageIEval):
    stored = False
    announce = dict(inception='Generating batches...', fid='Generating batches and their activation statistics...',
                    imd='Generating pairs...')

    def restore(self):
        restore_chain(self.model, self.cfg.CHECKPOINT_DIR, self.bs, lambda what: RuntimeError('Could not load the checkpoints of %s' % what))

    def dims(self):
        return self.model.stagei.z_dim, self.model.stagei.embed_dim

    def generate_batch(self, z, cond, is_training):
        m = self.model
        img64, _, _ = m.stagei.generator(z, cond, reuse=True, is_training=is_training)
        return m.generator(img64, cond, reuse=True, is_training=is_training)[0]

    def is_chunk(self):
        return self.bs          # the whole batch at once, whatever the Inception batch
