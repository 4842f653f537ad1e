"""StageIVisualizer — the caption visualiser of the reference's models/stackgan/stageI/visualize_stagei.py (what its run.py
starts when neither EVAL.FLAG nor TRAIN.FLAG is set; here behind `run.py --visualize`).

utils/visualizer.py's sheets; the calls are the reference's, in its order, so the global `np.random` stream is consumed the same
way: one `dataset_pos`, then `interp` rounds (the reference's loop is `range(0)`, i.e. none, the default here) of
  - `z_interp/z_interp{idx}.png`: z slerped between two draws, one caption, the generator WITHOUT conditioning noise;
  - `cond_interp/cond_interp{idx}.png`: the embedding lerped between the test images at `dataset_pos` and at
    `dataset_pos2 = dataset_pos + randint(...)`, which can pass the end of the split (kept: next_batch_test's own window rule
    applies), fresh z per image, the generator without conditioning noise;
  - `cap/cap{idx}.png`: a batch of one caption from the generator with conditioning noise;
then `special_cap/cap{0,1,2}.png` at three fixed test positions, all under SAMPLE_DIR/<dataset>_visual/.  Both generators are
callables over the eval-mode generator (is_training=False, no gradient: its norms run fused, model.py) at TRAIN.BATCH_SIZE.

Deviations, on purpose:
  - the reference always takes its special positions from `special_birds` = [12, 908, 1005] and never reads `special_flowers`;
    here the list follows DATASET_NAME, as models/pggan/visualize_pggan.py does (flowers: [1126, 908, 398]);
  - `neighb/neighb.png` is commented out in the reference; it is built here: the first 8 images generated for the test window
    at `dataset_pos`, clipped to [-1, 1], above their closest train images (utils/visualize.py gen_closest_neighbour_img: one
    t2i_nearest_images launch over the resident 76 x 76 uint8 store with 64 x 64 crops).  It is drawn last, so the sheets the
    reference writes see the random streams it would give them."""
import numpy as np

from ....utils.visualizer import CaptionVisualizer

SPECIAL = {'flowers': [1126, 908, 398], 'birds': [12, 908, 1005]}      # visualize_stagei.py:76-77
NEIGHBOUR_TEXT = 'Generated images (first row) and their closest neighbours (second row)'


class StageIVisualizer(CaptionVisualizer):
    neighbour_text = NEIGHBOUR_TEXT          # the commented-out line of each reference file

    def __init__(self, sess, model, dataset, cfg):
        super(StageIVisualizer, self).__init__(sess, model, dataset, cfg)

    def special_positions(self):
        """The three test positions of DATASET_NAME; a test split they do not fit in raises (next_batch_test would silently move a
        window past the end back)."""
        name = self.config.get('DATASET_NAME', self.dataset.name)
        if name not in SPECIAL:
            raise ValueError('DATASET_NAME %r has no special positions (known: %s)' % (name, sorted(SPECIAL)))
        n = self.dataset.test.num_examples
        for pos in SPECIAL[name]:
            if not 0 <= pos < n:
                raise ValueError('special test position %d is outside the test split of %d examples' % (pos, n))
        return SPECIAL[name]

    def _second_position(self, dataset_pos):
        return dataset_pos + np.random.randint(0, self.dataset.test.num_examples)          # visualize_stagei.py:35

    def _cond_pair(self, dataset_pos, dataset_pos2):
        """Two single-image windows, at `dataset_pos` and at `dataset_pos2`."""
        test = self.dataset.test
        _, cond1, _, caps1 = test.next_batch_test(1, dataset_pos, 1)
        _, cond2, _, caps2 = test.next_batch_test(1, dataset_pos2, 1)
        return cond1[0], cond2[0], self._first_caption(caps1), self._first_caption(caps2)
