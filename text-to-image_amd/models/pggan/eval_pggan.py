"""PGGANEval — reference models/pggan/eval_pggan.py: the Inception score of a stage's generator (stage 7, 256 x 256, by default).

    python text-to-image_amd/models/pggan/eval_pggan.py --cfg models/pggan/cfg/flowers.yml --eval is|fid [--stage 7] [--batch 64]

The generator's variables (`g_net`) are restored from CHECKPOINT_DIR/stage%d/; a failed load raises with the reference's
message.  The dataset is `TextDataset(DATASET_DIR, MODEL.SIZES[stage - 1])` (256 at stage 7, as the reference reads).  Per batch
of `--batch` (EVAL.SIZE // batch batches; 50 000 // 64 in the reference's configs), in the reference's order from the global
np.random stream: z ~ N(0, 1) [batch, 128], then `dataset.test.next_batch(batch, 4, embeddings=True)` (the means of four caption
embeddings), the generator with conditioning noise on (the reference's `gen_op`), clip to [-1, 1], the resize to 299 x 299 by
t2i_resample_bilinear straight from the fp32 images (denormalize_images + prep_incep_img, bit for bit), InceptionV3 and a float32
softmax.  Nothing is kept between batches: 50 000 images of 256 x 256 would take 39 GB in fp32.

- evaluate_inception: the predictions in generation order, with NO shuffle, then get_inception_from_predictions(preds, 10), as
  the reference's evaluator does.
- evaluate_fid: an addition: the reference's PGGAN evaluator computes IS only.  The same batches' PreLogits statistics are
  streamed through t2i_gram_accumulate and compared with the real statistics of EVAL.ACT_STAT_PATH, which are computed from the
  images under EVAL.R_IMG_PATH first if the file is absent (as for wgancls); 500 on a failure, the other evaluators' fallback.

The PGGAN generator has no batch norm, so there is no training / inference mode to choose between the two."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.evaluation import fid, inception_score  # noqa: E402
from t2i_amd.models.inception.model import IMAGE_SIZE, load_inception_inference  # noqa: E402
from t2i_amd.utils.saver import Saver, load  # noqa: E402


def stage_model(cfg, stage, batch_size, dataset, device, **widths):
    """The stage's PGGAN without its training graph (build_model=False), g_net created by a launch-free pass.  `widths`
    (fmap_base, fmap_max, z_dim, embed_dim, compr_embed_dim) default to the reference's."""
    from t2i_amd.models.pggan.pggan import PGGAN
    from t2i_amd.scope import trainable_variables
    m = PGGAN(batch_size=batch_size, steps=None, check_dir_write='', check_dir_read=os.path.join(cfg.CHECKPOINT_DIR, 'stage%d/' % stage),
              dataset=dataset, sample_path=None, log_dir=None, stage=stage, trans=False, build_model=False, device=device, **widths)
    if not trainable_variables('g_net'):
        with K.dry_run(), torch.no_grad():
            m.generator(torch.empty(batch_size, m.z_dim, device=m.device), torch.empty(batch_size, m.embed_dim, device=m.device),
                        stages=stage, t=False)
    return m


def restore_generator(m):
    could_load, _ = load(Saver(m.store, var_list=['g_net']), None, m.check_dir_read)
    if not could_load:
        raise RuntimeError('Could not load stage %d' % m.stage)


def generate(m, z, cond, cond_noise=True):
    """The stage generator on device tensors (fresh truncated-normal conditioning noise when cond_noise), clipped to [-1, 1]."""
    with torch.no_grad():
        m._ca = None
        img, _, _ = m.generator(z, cond, stages=m.stage, t=False, reuse=True, cond_noise=cond_noise)
        return torch.clamp(img.float(), -1.0, 1.0).contiguous()


class PGGANEval(object):
    def __init__(self, sess, model, dataset, cfg, incep_batch_size=None):
        self.sess = sess                   # unused: there is no TF session
        self.model = model
        self.dataset = dataset
        self.cfg = cfg
        self.bs = model.batch_size
        self.incep_batch_size = incep_batch_size or self.bs      # eval_pggan.py: incep_batch_size = batch_size

    def _inception(self):
        return load_inception_inference(self.cfg.EVAL.NUM_CLASSES, self.cfg.EVAL.INCEP_CHECKPOINT_DIR, self.model.device)

    def _n_batches(self):
        n = self.cfg.EVAL.SIZE // self.bs
        if n == 0:
            raise ValueError('EVAL.SIZE %d is smaller than the batch %d' % (self.cfg.EVAL.SIZE, self.bs))
        return n

    def _stream(self, keep_samples):
        """Yields each clipped generated batch (device float32 [bs, S, S, 3]); keeps a host copy when asked."""
        m, dev = self.model, self.model.device
        n_batches = self._n_batches()
        self._kept = []
        for i in range(n_batches):
            print('\rGenerating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
            sample_z = np.random.normal(0, 1, size=(self.bs, m.z_dim))
            _, _, embed, _, _ = self.dataset.test.next_batch(self.bs, 4, embeddings=True)
            z = torch.as_tensor(sample_z, dtype=torch.float32).to(dev)
            cond = embed if torch.is_tensor(embed) else torch.as_tensor(np.asarray(embed), dtype=torch.float32)
            img = generate(m, z, cond.to(device=dev, dtype=torch.float32).reshape(self.bs, m.embed_dim))
            if keep_samples:
                self._kept.append(img.cpu().numpy())
            yield img
        print()

    def _chunks(self, img):
        c = self.incep_batch_size
        for s in range(0, img.shape[0], c):
            yield K.resample_bilinear(img[s:s + c], IMAGE_SIZE, IMAGE_SIZE)

    def _samples(self, keep_samples):
        return dict(samples=np.concatenate(self._kept)) if keep_samples else {}

    def evaluate_inception(self, keep_samples=False):
        """-> dict(mean, std, preds: float32 [n, classes] in generation order) (+ samples, host, with keep_samples)."""
        net = self._inception()
        restore_generator(self.model)
        preds = []
        for img in self._stream(keep_samples):
            for x in self._chunks(img):
                logits, _ = net(x)
                preds.append(inception_score.softmax32(logits.cpu().numpy()))
        print('Computing inception score...')
        preds = np.concatenate(preds, 0)
        mean, std = inception_score.get_inception_from_predictions(preds, 10)
        print('Inception Score | mean:', '%.2f' % mean, 'std:', '%.2f' % std)
        return dict(mean=mean, std=std, preds=preds, **self._samples(keep_samples))

    def evaluate_fid(self, keep_samples=False):
        """-> dict(fid, mu_gen, sigma_gen, mu_real, sigma_real) (+ samples with keep_samples)."""
        net = self._inception()
        path = self.cfg.EVAL.ACT_STAT_PATH
        if not os.path.exists(path):
            print('Computing activation statistics for real x')
            fid.compute_and_save_activation_statistics(self.cfg.EVAL.R_IMG_PATH, net, self.incep_batch_size, path,
                                                       self.model.device, verbose=True)
        print('Loading activation statistics for the real x')
        mu_real, sigma_real = fid.load_activation_statistics(path)
        restore_generator(self.model)
        stats = fid.ActivationStatistics(device=self.model.device)
        for img in self._stream(keep_samples):
            for x in self._chunks(img):
                _, pre = net(x)
                stats.add(pre.reshape(x.shape[0], -1))
        mu_gen, sigma_gen = stats.finalize()
        print('calculate FID:', end=' ', flush=True)
        try:
            value = fid.calculate_frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)
        except Exception as e:          # the other evaluators' fallback
            print(e)
            value = 500
        print(value)
        return dict(fid=value, mu_gen=mu_gen, sigma_gen=sigma_gen, mu_real=mu_real, sigma_real=sigma_real,
                    **self._samples(keep_samples))


def load_stage_dataset(cfg, stage, device):
    from t2i_amd.preprocess.dataset import TextDataset
    datadir = cfg.DATASET_DIR
    dataset = TextDataset(datadir, cfg.MODEL.SIZES[stage - 1], device=device)
    dataset.test = dataset.get_data('%s/test' % datadir)
    dataset.train = dataset.get_data('%s/train' % datadir)
    return dataset


def main(argv=None, **widths):
    from t2i_amd.utils.config import config_from_yaml
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', required=True, help='models/pggan/cfg/flowers.yml or birds.yml')
    ap.add_argument('--eval', choices=['is', 'fid'], default='is')
    ap.add_argument('--stage', type=int, default=7, help='the stage whose generator is scored [7]')
    ap.add_argument('--batch', type=int, default=64, help='images generated (and scored) per batch [64]')
    ap.add_argument('--incep-batch', type=int, default=None, help='Inception batch (default: --batch)')
    args = ap.parse_args(argv)
    if not 1 <= args.stage <= 8:
        ap.error('--stage must be in 1..8')
    if args.batch < 1 or (args.incep_batch is not None and args.incep_batch < 1):
        ap.error('--batch and --incep-batch must be positive')
    cfg = config_from_yaml(args.cfg)
    if not os.path.isfile(os.path.join(cfg.CHECKPOINT_DIR, 'stage%d' % args.stage, 'checkpoint')):
        raise RuntimeError('Could not load stage %d (no checkpoint in %s)' % (args.stage, os.path.join(cfg.CHECKPOINT_DIR, 'stage%d' % args.stage)))
    if cfg.EVAL.SIZE // args.batch == 0:
        raise ValueError('EVAL.SIZE %d is smaller than --batch %d' % (cfg.EVAL.SIZE, args.batch))
    dev = torch.device('cuda')
    dataset = load_stage_dataset(cfg, args.stage, dev)
    m = stage_model(cfg, args.stage, args.batch, dataset, dev, **widths)
    ev = PGGANEval(None, m, dataset, cfg, incep_batch_size=args.incep_batch)
    out = ev.evaluate_inception() if args.eval == 'is' else ev.evaluate_fid()
    out.pop('preds', None)
    return out


if __name__ == '__main__':
    main()
