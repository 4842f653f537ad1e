"""CaptionVisualizer — the one caption visualiser of wgancls, GAN-CLS and the two StackGAN stages (reference
models/*/visualize_*.py, copies of models/wgancls/visualize_wgan.py; what each run.py starts behind `--visualize`).

The calls are the reference's, in its order, so the global `np.random` / `random` streams are consumed the same way: one
`dataset_pos`, then `interp` rounds (the reference's loop is `range(0)`, i.e. none, the default here) of
  - `z_interp/z_interp{idx}.png`: z slerped between two draws, one caption, the generator WITHOUT conditioning noise;
  - `cond_interp/cond_interp{idx}.png`: the embedding lerped between two test images, fresh z per image, without conditioning noise;
  - `cap/cap{idx}.png`: a batch of one caption from the generator with conditioning noise;
then `special_cap/cap{0,1,2}.png` at three fixed test positions and `neighb/neighb.png`: the first 8 images generated for the test
window at `dataset_pos`, clipped to [-1, 1], above their closest train images (utils/visualize.py gen_closest_neighbour_img: one
t2i_nearest_images launch over the resident uint8 store), all under SAMPLE_DIR/<dataset>_visual/.  The neighbour sheet is drawn
last, so the sheets before it see the random streams the reference would give them.  Both generators are callables over the
eval-mode generator (is_training=False, no gradient) at TRAIN.BATCH_SIZE, the batch the reference feeds.

A model's visualiser states what differs (DESIGN.md has the table) through the hooks of the first section."""
import numpy as np
import torch

from . import visualize as V
from .saver import restore_g_net


class CaptionVisualizer(object):
    neighbour_text = V.NEIGHBOUR_TEXT

    def __init__(self, sess, model, dataset, config):
        self.sess = sess                   # unused: there is no TF session
        self.model = model
        self.dataset = dataset
        self.config = config
        self.samples_dir = config.SAMPLE_DIR

    # ---- what a model states ------------------------------------------------------------------------------------------------
    def special_positions(self):
        """The three test positions of the special sheets; checked before anything is restored."""
        raise NotImplementedError

    def _dims(self):
        return self.model.z_dim, self.model.embed_dim

    def _images(self, z, cond, cond_noise):
        return self.model.generator(z, cond, reuse=True, is_training=False, cond_noise=cond_noise)[0]

    def _restore_generator(self):
        """`g_net` (a launch-free dry pass creates its variables if the model has not) from CHECKPOINT_DIR:
        tf.train.Saver(tf.global_variables('g_net')) + load in the reference, whose error is kept."""
        restore_g_net(self.model, self.config.CHECKPOINT_DIR, self.model.batch_size, LookupError('Could not load any checkpoints'))

    def _second_position(self, dataset_pos):
        """The round's second test position, drawn right behind `dataset_pos` (None: the embedding pair needs none)."""

    def _cond_pair(self, dataset_pos, dataset_pos2):
        """The two embeddings of the embedding interpolation and their captions: one window of two test images."""
        _, cond, _, captions = self.dataset.test.next_batch_test(2, dataset_pos, 1)
        return cond[0][0], cond[0][1], self._first_caption(captions, 0), self._first_caption(captions, 1)

    def _round_extras(self, idx, dataset_pos, gen, out):
        """Sheets of one interpolation round behind the captioned batch (Stage II: the stage sheet)."""

    # ---- the visualiser -------------------------------------------------------------------------------------------------------
    def _path(self, kind, name):
        return '{}/{}_visual/{}/{}.png'.format(self.samples_dir, self.dataset.name, kind, name)

    @staticmethod
    def _first_caption(captions, i=0):
        """The first caption of image i of a next_batch_test window; '' when the split has no caption files (the reference
        would raise IndexError there)."""
        return captions[i][0] if len(captions) > i and captions[i] else ''

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
        cap = self._first_caption
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
            cond1, cond2, cap1, cap2 = self._cond_pair(dataset_pos, dataset_pos2)
            samples = V.gen_cond_interp_img(gen_no_noise, cond1, cond2, z_dim, B)
            out['cond_interp'].append(V.save_interp_cap_batch(samples, cap1, cap2, self._path('cond_interp', 'cond_interp%d' % idx)))
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
