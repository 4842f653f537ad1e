"""PGGANVisualizer — reference models/pggan/visualize_pggan.py: caption sheets of a stage's generator (stage 7 by default).

    python text-to-image_amd/models/pggan/visualize_pggan.py --cfg models/pggan/cfg/flowers.yml [--interp 40] [--stage 7]

The calls are the reference's, in its order, so the global `np.random` stream is consumed the same way: one `dataset_pos`, then
`interp` rounds (the reference loops 40 times) of
  - `z_interp/z_interp{idx}.png`: z slerped between two draws, one caption, the generator WITHOUT conditioning noise;
  - `cond_interp/cond_interp{idx}.png` and `cond_interp/gifs/cond_interp{idx}.gif`: the embedding lerped between the test
    images at two random positions, fresh z per image, the generator without conditioning noise;
  - `cap/cap{idx}.png`: 64 images of one caption from the generator with conditioning noise;
then `special_cap/cap{0,1,2}.png` at three fixed test positions, all under SAMPLE_DIR/<dataset>_visual/.

Deviations, on purpose:
  - the reference always takes its special positions from `special_birds` = [12, 908, 1005], even for flowers; here the list
    follows DATASET_NAME (flowers: [1126, 908, 398], the reference's `special_flowers`);
  - the reference's make_gif renders with moviepy, which this project does not depend on; `make_gif` writes the same frames
    (((x + 1) / 2 * 255) as uint8, the batch in order, each shown for duration / len(batch) seconds, looping) with Pillow.  Pillow
    folds identical consecutive frames into one longer frame.
The sheets are utils/visualize.py's; the generator runs at the reference's batch of 64."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd.models.pggan.eval_pggan import Reader, generate, restore_generator  # noqa: E402
from t2i_amd.models.wgancls.visualize_wgan import WGanClsVisualizer  # noqa: E402
from t2i_amd.utils import visualize as V  # noqa: E402

SPECIAL = {'flowers': [1126, 908, 398], 'birds': [12, 908, 1005]}      # visualize_pggan.py:113-114


def make_gif(images, fname, duration=2):
    """reference utils/utils.py make_gif (true_image=False) with Pillow: images [n, h, w, 3] in [-1, 1] -> an animated GIF of
    n frames, duration / n seconds each, looping.  -> the uint8 frames written."""
    from PIL import Image
    images = V._host(images)
    frames = ((images + 1) / 2 * 255).astype(np.uint8)
    d = os.path.dirname(fname)
    if d and not os.path.exists(d):
        os.makedirs(d)
    pil = [Image.fromarray(f) for f in frames]
    pil[0].save(fname, save_all=True, append_images=pil[1:], duration=1000.0 * duration / len(pil), loop=0)
    return frames


def generator_fn(m, cond_noise):
    """gen(z, cond) on host arrays -> host float32 images in [-1, 1], at the model's batch."""
    def gen(z, cond):
        z = torch.as_tensor(np.asarray(z, dtype=np.float32), device=m.device)
        cond = torch.as_tensor(V._host(cond), dtype=torch.float32).to(m.device).reshape(-1, m.embed_dim)
        if z.shape[0] != m.batch_size or cond.shape[0] != m.batch_size:
            raise ValueError('the generator takes batches of %d, got z %s and cond %s' % (m.batch_size, tuple(z.shape), tuple(cond.shape)))
        return generate(m, z, cond, cond_noise).cpu().numpy()
    return gen


class PGGANVisualizer(object):
    def __init__(self, sess, model, dataset, config, ema=False):
        self.sess = sess                   # unused: there is no TF session
        self.ema = ema                     # True: draw from the moving average of the generator's weights
        self.model = model
        self.dataset = dataset
        self.config = config
        self.samples_dir = config.SAMPLE_DIR

    def _path(self, kind, name, ext='png'):
        return '{}/{}_visual/{}/{}.{}'.format(self.samples_dir, self.dataset.name, kind, name, ext)

    def special_positions(self):
        name = self.config.get('DATASET_NAME', self.dataset.name)
        if name not in SPECIAL:
            raise ValueError('DATASET_NAME %r has no special positions (known: %s)' % (name, sorted(SPECIAL)))
        return SPECIAL[name]

    def visualize(self, interp=40):
        """-> dict of the uint8 sheets written ('z_interp', 'cond_interp', 'cap', 'special_cap': lists) and the GIF frames
        ('gifs': list of uint8 [64, h, w, 3])."""
        m, test = self.model, self.dataset.test
        specials = self.special_positions()
        restore_generator(m, ema=self.ema)
        gen, gen_no_noise = generator_fn(m, True), generator_fn(m, False)
        B, z_dim = m.batch_size, m.z_dim
        cap = WGanClsVisualizer._first_caption
        out = {'z_interp': [], 'cond_interp': [], 'cap': [], 'special_cap': [], 'gifs': []}

        dataset_pos = np.random.randint(0, test.num_examples)
        for idx in range(interp):
            dataset_pos = np.random.randint(0, test.num_examples)
            dataset_pos2 = np.random.randint(0, test.num_examples)
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
            out['gifs'].append(make_gif(samples, self._path('cond_interp/gifs', 'cond_interp%d' % idx, 'gif'), duration=10))
            # captioned batch
            _, cond, _, captions = test.next_batch_test(1, dataset_pos, 1)
            samples = V.gen_captioned_img(gen, cond[0], z_dim, B)
            out['cap'].append(V.save_cap_batch(samples, cap(captions), self._path('cap', 'cap%d' % idx)))

        for idx, special_pos in enumerate(specials):
            print(special_pos)
            _, cond, _, captions = test.next_batch_test(1, special_pos, 1)
            samples = V.gen_captioned_img(gen, cond[0], z_dim, B)
            out['special_cap'].append(V.save_cap_batch(samples, cap(captions), self._path('special_cap', 'cap%d' % idx)))
        return out


def main(argv=None, **widths):
    from t2i_amd.utils.config import config_from_yaml
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', required=True, help='models/pggan/cfg/flowers.yml or birds.yml')
    ap.add_argument('--interp', type=int, default=40, help='rounds of interpolation / caption sheets [40]')
    ap.add_argument('--stage', type=int, default=7, help='the stage whose generator draws the sheets [7]')
    ap.add_argument('--ema', action='store_true', help="draw from the moving average of the generator's weights (a checkpoint of train_pggan.py --g-ema)")
    reader = Reader(ap, argv, widths)
    args = reader.args
    if args.interp < 0 or not 1 <= args.stage <= 8:
        ap.error('--interp must be >= 0 and --stage in 1..8')
    cfg = config_from_yaml(args.cfg)
    if cfg.DATASET_NAME not in SPECIAL:
        raise ValueError('DATASET_NAME %r has no special positions (known: %s)' % (cfg.DATASET_NAME, sorted(SPECIAL)))
    reader.need_checkpoint(cfg, args.stage)
    dataset, m = reader.open(cfg, args.stage, 64)
    return PGGANVisualizer(None, m, dataset, cfg, ema=args.ema).visualize(args.interp)


if __name__ == '__main__':
    main()
