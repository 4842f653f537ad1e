"""StageIIVisualizer — the caption visualiser of the reference's models/stackgan/stageII/visualize_stageiI.py (behind
`run.py --visualize`): StageIVisualizer's sheets drawn by the chain Stage-I generator -> Stage-II generator, 256 x 256.

`g_net` is restored from the Stage-I config's CHECKPOINT_DIR and `stageII_g_net` from the Stage-II one, each failure with the
reference's LookupError.  As in the reference graph the Stage-I generator under the chain always draws its conditioning noise;
`gen` / `gen_no_noise` switch the Stage-II generator's.  Per `interp` round, in the reference's draw order (here `dataset_pos2` is a
plain `randint`), the Stage-I sheets and then
  - `stages/stage{idx}.png`, text `Stage I and Stage II`: utils/visualize.py gen_multiple_stage_img([gen_stagei, gen], size=128)
    for the test window at `dataset_pos` — 8 Stage-I images over the 8 chain images of the same z and captions, each resized to
    128 x 128 as the reference's float `scipy.misc.imresize(..., 'nearest')` does (t2i_bytescale_nearest).  The two rows are
    separate generator runs, as in the reference: each draws its own conditioning noise.
The special positions follow DATASET_NAME (the reference always uses its birds list), and `neighb/neighb.png`, commented out in
the reference, is built: the 304 x 304 train store searched with 256 x 256 crops by one t2i_nearest_images launch (8 queries: the
crop table and the workspace hold 8 x N_train entries each, a few hundred KB for either data set)."""
import numpy as np

from ....utils import visualize as V
from ..stageI.visualize_stagei import StageIVisualizer
from .eval_stageii import restore_chain

STAGES_TEXT = 'Stage I and Stage II'


class StageIIVisualizer(StageIVisualizer):
    neighbour_text = V.NEIGHBOUR_TEXT

    def _dims(self):
        return self.model.stagei.z_dim, self.model.stagei.embed_dim

    def _stage_i_images(self, z, cond):
        return self.model.stagei.generator(z, cond, reuse=True, is_training=False)[0]

    def _images(self, z, cond, cond_noise):
        return self.model.generator(self._stage_i_images(z, cond), cond, reuse=True, is_training=False, cond_noise=cond_noise)[0]

    def _restore_generator(self):
        restore_chain(self.model, self.config.CHECKPOINT_DIR, self.model.batch_size,
                      lambda what: LookupError('Could not load any checkpoints for %s' % what))

    def _second_position(self, dataset_pos):
        return np.random.randint(0, self.dataset.test.num_examples)          # visualize_stageiI.py:44

    def _round_extras(self, idx, dataset_pos, gen, out):
        m = self.model
        _, cond, _, _ = self.dataset.test.next_batch_test(m.batch_size, dataset_pos, 1)
        samples = V.gen_multiple_stage_img([self._generator(self._stage_i_images), gen], cond[0], self._dims()[0], m.batch_size, size=128)
        out.setdefault('stages', []).append(V.save_cap_batch(samples, STAGES_TEXT, self._path('stages', 'stage%d' % idx)))
