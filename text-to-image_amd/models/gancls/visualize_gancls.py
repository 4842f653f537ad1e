"""GanClsVisualizer — the caption visualiser of the reference's models/gancls/visualize_gancls.py (what its run.py starts when
neither EVAL.FLAG nor TRAIN.FLAG is set; here behind `run.py --visualize`).

The calls are the reference's, in its order, so the global `np.random` / `random` streams are consumed the same way:
`dataset_pos`, then `interp` rounds of z-interpolation / embedding-interpolation / captioned sheets (the reference's loop is
`range(0)`, i.e. none, the default here), then the three special test positions, then the neighbour sheet: the first 8 images
generated for the test window at `dataset_pos`, clipped to [-1, 1], above their closest train images (utils/visualize.py; the
search is one t2i_nearest_images launch over the resident uint8 store).  The generator has no conditioning noise, so one
callable over the eval-mode generator serves every sheet; it runs at TRAIN.BATCH_SIZE, the batch the reference feeds."""
import numpy as np
import torch

from ... import kernels as K
from ...utils import visualize as V
from ...utils.saver import Saver, load

SPECIAL_POSITIONS = (1126, 908, 398)          # visualize_gancls.py:73


class GanClsVisualizer(object):
    def __init__(self, sess, model, dataset, config):
        self.sess = sess                   # unused: there is no TF session
        self.model = model
        self.dataset = dataset
        self.config = config
        self.samples_dir = config.SAMPLE_DIR

    def _path(self, kind, name):
        return '{}/{}_visual/{}/{}.png'.format(self.samples_dir, self.dataset.name, kind, name)

    def _generator(self):
        m, B = self.model, self.model.batch_size

        def gen(z, cond):
            z = torch.as_tensor(np.asarray(z, dtype=np.float32), device=m.device)
            cond = torch.as_tensor(V._host(cond), dtype=torch.float32).to(m.device).reshape(-1, m.embed_dim)
            if z.shape[0] != B or cond.shape[0] != B:
                raise ValueError('the generator takes batches of %d, got z %s and cond %s' % (B, tuple(z.shape), tuple(cond.shape)))
            with torch.no_grad():
                img = m.generator(z, cond, reuse=True, is_training=False)
            return img.float().cpu().numpy()
        return gen

    def _restore_generator(self):
        """The generator's variables (a launch-free dry pass creates them if the model has not), restored from the latest
        checkpoint: tf.train.Saver(tf.global_variables('g_net')) + load in the reference, whose error is kept."""
        m = self.model
        from ...scope import trainable_variables
        if not trainable_variables('g_net'):
            with K.dry_run(), torch.no_grad():
                m.generator(torch.empty(m.batch_size, m.z_dim, device=m.device), torch.empty(m.batch_size, m.embed_dim, device=m.device),
                            reuse=False, is_training=False)
        could_load, _ = load(Saver(m.store, var_list=['g_net']), None, self.config.CHECKPOINT_DIR)
        if not could_load:
            print(' [!] Load failed...')
            raise LookupError('Could not load any checkpoints')
        print(' [*] Load SUCCESS')

    @staticmethod
    def _first_caption(captions, i=0):
        return captions[i][0] if len(captions) > i and captions[i] else ''

    def visualize(self, interp=0):
        """-> dict of the uint8 sheets written ('z_interp', 'cond_interp', 'cap', 'special_cap': lists; 'neighb'), plus
        'neighbour_ids' (int64 [Q]), 'crops' ((row0, col0, flip) int32 [Q, N_train] each, or None), 'samples' (the clipped float32
        queries [Q,64,64,3]) and 'neighbours' ([Q,64,64,3]) of the neighbour search."""
        m, test = self.model, self.dataset.test
        for pos in SPECIAL_POSITIONS:          # (next_batch_test would silently move a window past the end back)
            if not 0 <= pos < test.num_examples:
                raise ValueError('special test position %d is outside the test split of %d examples' % (pos, test.num_examples))
        self._restore_generator()
        gen = self._generator()
        B, z_dim = m.batch_size, m.z_dim
        out = {'z_interp': [], 'cond_interp': [], 'cap': [], 'special_cap': []}

        dataset_pos = np.random.randint(0, test.num_examples)
        for idx in range(interp):
            dataset_pos = np.random.randint(0, test.num_examples)
            # interpolation in z space
            _, cond, _, captions = test.next_batch_test(1, dataset_pos, 1)
            samples = V.gen_noise_interp_img(gen, cond[0], z_dim, B)
            out['z_interp'].append(V.save_cap_batch(samples, self._first_caption(captions), self._path('z_interp', 'z_interp%d' % idx)))
            # interpolation in embedding space
            _, cond, _, captions = test.next_batch_test(2, dataset_pos, 1)
            samples = V.gen_cond_interp_img(gen, cond[0][0], cond[0][1], z_dim, B)
            out['cond_interp'].append(V.save_interp_cap_batch(samples, self._first_caption(captions, 0), self._first_caption(captions, 1),
                                                              self._path('cond_interp', 'cond_interp%d' % idx)))
            # captioned batch
            _, cond, _, captions = test.next_batch_test(1, dataset_pos, 1)
            samples = V.gen_captioned_img(gen, cond[0], z_dim, B)
            out['cap'].append(V.save_cap_batch(samples, self._first_caption(captions), self._path('cap', 'cap%d' % idx)))

        for idx, special_pos in enumerate(SPECIAL_POSITIONS):
            print(special_pos)
            _, cond, _, captions = test.next_batch_test(1, special_pos, 1)
            samples = V.gen_captioned_img(gen, cond[0], z_dim, B)
            out['special_cap'].append(V.save_cap_batch(samples, self._first_caption(captions), self._path('special_cap', 'cap%d' % idx)))

        # generated images above their closest train images
        _, cond, _, _ = test.next_batch_test(B, dataset_pos, 1)
        samples, neighbours, ids, crops = V.gen_closest_neighbour_img(gen, cond[0], z_dim, B, self.dataset)
        text = 'Generated images (first row) and their closest neighbours (second row)'
        out['neighb'] = V.save_cap_batch(np.concatenate([samples, neighbours]), text, self._path('neighb', 'neighb'))
        out.update(neighbour_ids=ids.cpu().numpy(), crops=crops, samples=samples, neighbours=neighbours)
        return out
