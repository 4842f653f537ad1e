"""WGanClsVisualizer — the caption visualiser of the reference's models/wgancls/visualize_wgan.py (what run.py starts when
TRAIN.FLAG is False; here behind `run.py --visualize`).

The calls are the reference's, in its order, so the global `np.random` / `random` streams are consumed the same way:
`dataset_pos`, then `interp` rounds of noise-interpolation / embedding-interpolation / captioned sheets (the reference runs
`range(0)` of them, i.e. none, which is the default here), then the three special test positions, then the neighbour sheet
of the first 8 generated images of the batch at `dataset_pos` above their closest train images (utils/visualize.py; the
search is one HIP launch over the resident uint8 store).  The two generators of the reference graph are callables over the
eval-mode generator: with conditioning noise (`gen`) and without (`gen_no_noise`); they run at TRAIN.BATCH_SIZE, the
reference placeholder's batch."""
import numpy as np
import torch

from ... import kernels as K
from ...utils import visualize as V
from ...utils.saver import Saver, load


class WGanClsVisualizer(object):
    def __init__(self, sess, model, dataset, config):
        self.sess = sess                   # unused: there is no TF session
        self.model = model
        self.dataset = dataset
        self.config = config
        self.samples_dir = config.SAMPLE_DIR

    def _path(self, kind, name):
        return '{}/{}_visual/{}/{}.png'.format(self.samples_dir, self.dataset.name, kind, name)

    def _generator(self, cond_noise):
        m, B = self.model, self.model.batch_size

        def gen(z, cond):
            z = torch.as_tensor(np.asarray(z, dtype=np.float32), device=m.device)
            cond = torch.as_tensor(V._host(cond), dtype=torch.float32).to(m.device).reshape(-1, m.embed_dim)
            if z.shape[0] != B or cond.shape[0] != B:
                raise ValueError('the generator takes batches of %d, got z %s and cond %s' % (B, tuple(z.shape), tuple(cond.shape)))
            with torch.no_grad():
                img, _, _ = m.generator(z, cond, reuse=True, is_training=False, cond_noise=cond_noise)
            return img.float().cpu().numpy()
        return gen

    def _restore_generator(self):
        """The generator's variables (a launch-free dry pass creates them if the model has not), restored from the latest
        checkpoint: tf.train.Saver(tf.global_variables('g_net')) + load in the reference."""
        m = self.model
        from ...scope import trainable_variables
        if not trainable_variables('g_net'):
            with K.dry_run(), torch.no_grad():
                m.generator(torch.empty(m.batch_size, m.z_dim, device=m.device), torch.empty(m.batch_size, m.embed_dim, device=m.device),
                            reuse=False, is_training=False)
        could_load, _ = load(Saver(m.store, var_list=['g_net']), None, self.config.CHECKPOINT_DIR)
        if not could_load:
            print(' [!] Load failed...')
            raise RuntimeError('Could not load the checkpoints of the generator')
        print(' [*] Load SUCCESS')

    @staticmethod
    def _first_caption(captions, i=0):
        """The first caption of image i of a next_batch_test window; '' when the split has no caption files (the reference
        would raise IndexError there)."""
        return captions[i][0] if len(captions) > i and captions[i] else ''

    def visualize(self, interp=0):
        """-> dict of the uint8 sheets written ('z_interp', 'cond_interp', 'cap', 'special_cap': lists; 'neighb'), plus
        'neighbour_ids' (int64 [Q]), 'crops' ((row0, col0, flip) int32 [Q, N_train] each, or None) and 'samples' (the clipped
        float32 queries [Q,64,64,3]) of the neighbour search, and 'neighbours' ([Q,64,64,3])."""
        self._restore_generator()
        gen, gen_no_noise = self._generator(True), self._generator(False)
        m, test = self.model, self.dataset.test
        B, z_dim = m.batch_size, m.z_dim
        out = {'z_interp': [], 'cond_interp': [], 'cap': [], 'special_cap': []}

        dataset_pos = np.random.randint(0, test.num_examples)
        for idx in range(interp):
            dataset_pos = np.random.randint(0, test.num_examples)
            # interpolation in z space
            _, cond, _, captions = test.next_batch_test(1, dataset_pos, 1)
            samples = V.gen_noise_interp_img(gen_no_noise, cond[0], z_dim, B)
            out['z_interp'].append(V.save_cap_batch(samples, self._first_caption(captions), self._path('z_interp', 'z_interp%d' % idx)))
            # interpolation in embedding space
            _, cond, _, captions = test.next_batch_test(2, dataset_pos, 1)
            samples = V.gen_cond_interp_img(gen_no_noise, cond[0][0], cond[0][1], z_dim, B)
            out['cond_interp'].append(V.save_interp_cap_batch(samples, self._first_caption(captions, 0), self._first_caption(captions, 1),
                                                              self._path('cond_interp', 'cond_interp%d' % idx)))
            # captioned batch
            _, cond, _, captions = test.next_batch_test(1, dataset_pos, 1)
            samples = V.gen_captioned_img(gen, cond[0], z_dim, B)
            out['cap'].append(V.save_cap_batch(samples, self._first_caption(captions), self._path('cap', 'cap%d' % idx)))

        for idx, special_pos in enumerate([1126, 908, 398]):
            print(special_pos)
            _, cond, _, captions = test.next_batch_test(1, special_pos, 1)
            samples = V.gen_captioned_img(gen, cond[0], z_dim, B)
            out['special_cap'].append(V.save_cap_batch(samples, self._first_caption(captions), self._path('special_cap', 'cap%d' % idx)))

        # generated images above their closest train images
        _, cond, _, _ = test.next_batch_test(B, dataset_pos, 1)
        samples, neighbours, ids, crops = V.gen_closest_neighbour_img(gen, cond[0], z_dim, B, self.dataset)
        out['neighb'] = V.save_cap_batch(np.concatenate([samples, neighbours]), V.NEIGHBOUR_TEXT, self._path('neighb', 'neighb'))
        out.update(neighbour_ids=ids.cpu().numpy(), crops=crops, samples=samples, neighbours=neighbours)
        return out
