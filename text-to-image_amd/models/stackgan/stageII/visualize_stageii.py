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
import torch

from .... import kernels as K
from ....scope import trainable_variables
from ....utils import visualize as V
from ....utils.saver import Saver, load
from ..stageI.visualize_stagei import StageIVisualizer

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
        m, s1 = self.model, self.model.stagei
        if not trainable_variables('stageII_g_net'):
            with K.dry_run(), torch.no_grad():
                z = torch.empty(m.batch_size, s1.z_dim, device=m.device)
                phi = torch.empty(m.batch_size, s1.embed_dim, device=m.device)
                img64, _, _ = s1.generator(z, phi, reuse=bool(trainable_variables('g_net')), is_training=False)
                m.generator(img64, phi, reuse=False, is_training=False)
        for scope, directory, what in (('g_net', s1.cfg.CHECKPOINT_DIR, 'stage I'), ('stageII_g_net', self.config.CHECKPOINT_DIR, 'stage II')):
            could_load, _ = load(Saver(m.store, var_list=[scope]), None, directory)
            if not could_load:
                print(' [!] Load failed...')
                raise LookupError('Could not load any checkpoints for %s' % what)
            print(' [*] Load SUCCESS')

    def _second_position(self, dataset_pos):
        return np.random.randint(0, self.dataset.test.num_examples)          # visualize_stageiI.py:44

    def _round_extras(self, idx, dataset_pos, gen, out):
        m = self.model
        _, cond, _, _ = self.dataset.test.next_batch_test(m.batch_size, dataset_pos, 1)
        samples = V.gen_multiple_stage_img([self._generator(self._stage_i_images), gen], cond[0], self._dims()[0], m.batch_size, size=128)
        out.setdefault('stages', []).append(V.save_cap_batch(samples, STAGES_TEXT, self._path('stages', 'stage%d' % idx)))
