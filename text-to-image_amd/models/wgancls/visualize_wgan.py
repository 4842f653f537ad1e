"""WGanClsVisualizer — the caption visualiser of the reference's models/wgancls/visualize_wgan.py (what run.py starts when
TRAIN.FLAG is False; here behind `run.py --visualize`): utils/visualizer.py's sheets with the reference's own choices.  The
special positions are its literal list, taken as they are (a window past the end of the test split is moved back by
next_batch_test); the embedding interpolation runs between the two images of one test window at `dataset_pos`; the two
generators of the reference graph are the eval-mode generator with conditioning noise (`gen`) and without (`gen_no_noise`)."""
from ...utils.saver import restore_g_net
from ...utils.visualizer import CaptionVisualizer


class WGanClsVisualizer(CaptionVisualizer):
    def special_positions(self):
        return [1126, 908, 398]

    def _restore_generator(self):
        restore_g_net(self.model, self.config.CHECKPOINT_DIR, self.model.batch_size,
                      RuntimeError('Could not load the checkpoints of the generator'))
