"""GanClsVisualizer — the caption visualiser of the reference's models/gancls/visualize_gancls.py (what its run.py starts when
neither EVAL.FLAG nor TRAIN.FLAG is set; here behind `run.py --visualize`): utils/visualizer.py's sheets.  The special positions
are the reference's, checked against the test split before anything is restored; the embedding interpolation runs between the
two images of one test window at `dataset_pos`; the generator has no conditioning noise, so the same eval-mode generator
serves every sheet."""
from ...utils.visualizer import CaptionVisualizer

SPECIAL_POSITIONS = (1126, 908, 398)          # visualize_gancls.py:73


class GanClsVisualizer(CaptionVisualizer):
    neighbour_text = 'Generated images (first row) and their closest neighbours (second row)'

    def special_positions(self):
        n = self.dataset.test.num_examples
        for pos in SPECIAL_POSITIONS:          # (next_batch_test would silently move a window past the end back)
            if not 0 <= pos < n:
                raise ValueError('special test position %d is outside the test split of %d examples' % (pos, n))
        return SPECIAL_POSITIONS

    def _images(self, z, cond, cond_noise):
        return self.model.generator(z, cond, reuse=True, is_training=False)
