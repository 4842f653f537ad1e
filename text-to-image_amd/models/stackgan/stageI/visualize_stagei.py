"""StageIVisualizer — the caption visualiser of the reference's models/stackgan/stageI/visualize_stagei.py (what its run.py
starts when neither EVAL.FLAG nor TRAIN.FLAG is set; here behind `run.py --visualize`).

The calls are the reference's, in its order, so the global `np.random` stream is consumed the same way: one `dataset_pos`, then
`interp` rounds (the reference's loop is `range(0)`, i.e. none, the default here) of
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
import torch

from .... import kernels as K
from ....scope import trainable_variables
from ....utils import visualize as V
from ....utils.saver import Saver, load
from ...wgancls.visualize_wgan import WGanClsVisualizer

SPECIAL = {'flowers': [1126, 908, 398], 'birds': [12, 908, 1005]}      # visualize_stagei.py:76-77
NEIGHBOUR_TEXT = 'Generated images (first row) and their closest neighbours (second row)'


class StageIVisualizer(object):
    neighbour_text = NEIGHBOUR_TEXT          # the commented-out line of each reference file

    def __init__(self, sess, model, dataset, cfg):
        self.sess = sess                   # unused: there is no TF session
        self.model = model
        self.dataset = dataset
        self.config = cfg
        self.samples_dir = cfg.SAMPLE_DIR

    def _path(self, kind, name):
        return '{}/{}_visual/{}/{}.png'.format(self.samples_dir, self.dataset.name, kind, name)

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

    # ---- what Stage II replaces -----------------------------------------------------------------------------------------
    def _dims(self):
        return self.model.z_dim, self.model.embed_dim

    def _images(self, z, cond, cond_noise):
        return self.model.generator(z, cond, reuse=True, is_training=False, cond_noise=cond_noise)[0]

    def _restore_generator(self):
        """`g_net` (a launch-free dry pass creates its variables if the model has not) from CHECKPOINT_DIR:
        tf.train.Saver(tf.global_variables('g_net')) + load in the reference, whose error is kept."""
        m = self.model
        if not trainable_variables('g_net'):
            with K.dry_run(), torch.no_grad():
                m.generator(torch.empty(m.batch_size, m.z_dim, device=m.device), torch.empty(m.batch_size, m.embed_dim, device=m.device),
                            reuse=False, is_training=False)
        could_load, _ = load(Saver(m.store, var_list=['g_net']), None, self.config.CHECKPOINT_DIR)
        if not could_load:
            print(' [!] Load failed...')
            raise LookupError('Could not load any checkpoints')
        print(' [*] Load SUCCESS')

    def _round_extras(self, idx, dataset_pos, gen, out):
        """Sheets of one interpolation round behind the captioned batch (Stage II: the stage sheet)."""

    # ---- the visualiser -------------------------------------------------------------------------------------------------
    def _generator(self, images):
        """gen(z, cond) on host arrays -> host float32 images, at the model's batch; `images(z, cond)` runs on the device."""
        m, B = self.model, self.model.batch_size
        z_dim, embed_dim = self._dims()

        def gen(z, cond):
            z = torch.as_tensor(np.asarray(z, dtype=np.float32), device=m.device)
            cond = torch.as_tensor(V._host(cond), dtype=torch.float32).to(m.device).reshape(-1, embed_dim)
            if tuple(z.shape) != (B, z_dim) or cond.shape[0] != B:
                raise ValueError('the generator takes batches of %d, got z %s and cond %s' % (B, tuple(z.shape), tuple(cond.shape)))
            with torch.no_grad():
                img = images(z, cond)
            return img.float().cpu().numpy()
        return gen

    def _second_position(self, dataset_pos):
        return dataset_pos + np.random.randint(0, self.dataset.test.num_examples)          # visualize_stagei.py:35

    def visualize(self, interp=0):
        """-> dict of the uint8 sheets written ('z_interp', 'cond_interp', 'cap', 'special_cap' (and 'stages' for Stage II):
        lists; 'neighb'), plus 'neighbour_ids' (int64 [Q]), 'crops' ((row0, col0, flip) int32 [Q, N_train] each, or None),
        'samples' (the clipped float32 queries [Q,s,s,3]) and 'neighbours' ([Q,s,s,3]) of the neighbour search."""
        m, test = self.model, self.dataset.test
        specials = self.special_positions()
        self._restore_generator()
        gen = self._generator(lambda z, cond: self._images(z, cond, True))
        gen_no_noise = self._generator(lambda z, cond: self._images(z, cond, False))
        B, z_dim = m.batch_size, self._dims()[0]
        cap = WGanClsVisualizer._first_caption
        out = {'z_interp': [], 'cond_interp': [], 'cap': [], 'special_cap': []}

        dataset_pos = np.random.randint(0, test.num_examples)
        for idx in range(interp):
            dataset_pos = np.random.randint(0, test.num_examples)
            dataset_pos2 = self._second_position(dataset_pos)
            # interpolation in z space
            _, cond, _, captions = test.next_batch_test(1, dataset_pos, 1)
            samples = V.gen_noise_interp_img(gen_no_noise, cond[0], z_dim, B)
            out['z_interp'].append(V.save_cap_batch(samples, cap(captions), self._path('z_interp', 'z_interp%d' % idx)))
            # interpolation in embedding space
            _, cond1, _, caps1 = test.next_batch_test(1, dataset_pos, 1)
            _, cond2, _, caps2 = test.next_batch_test(1, dataset_pos2, 1)
            samples = V.gen_cond_interp_img(gen_no_noise, cond1[0], cond2[0], z_dim, B)
            out['cond_interp'].append(V.save_interp_cap_batch(samples, cap(caps1), cap(caps2),
                                                              self._path('cond_interp', 'cond_interp%d' % idx)))
            # captioned batch
            _, cond, _, captions = test.next_batch_test(1, dataset_pos, 1)
            samples = V.gen_captioned_img(gen, cond[0], z_dim, B)
            out['cap'].append(V.save_cap_batch(samples, cap(captions), self._path('cap', 'cap%d' % idx)))
            self._round_extras(idx, dataset_pos, gen, out)

        for idx, special_pos in enumerate(specials):
            print(special_pos)
            _, cond, _, captions = test.next_batch_test(1, special_pos, 1)
            samples = V.gen_captioned_img(gen, cond[0], z_dim, B)
            out['special_cap'].append(V.save_cap_batch(samples, cap(captions), self._path('special_cap', 'cap%d' % idx)))

        # generated images above their closest train images
        _, cond, _, _ = test.next_batch_test(B, dataset_pos, 1)
        samples, neighbours, ids, crops = V.gen_closest_neighbour_img(gen, cond[0], z_dim, B, self.dataset)
        out['neighb'] = V.save_cap_batch(np.concatenate([samples, neighbours]), self.neighbour_text, self._path('neighb', 'neighb'))
        out.update(neighbour_ids=ids.cpu().numpy(), crops=crops, samples=samples, neighbours=neighbours)
        return out
