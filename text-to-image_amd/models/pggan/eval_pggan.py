"""PGGANEval — reference models/pggan/eval_pggan.py: the Inception score of a stage's generator (stage 7, 256 x 256, by default).

    python text-to-image_amd/models/pggan/eval_pggan.py --cfg models/pggan/cfg/flowers.yml --eval is|fid|swd|msssim|prdc|mmd [--stage 7] [--batch 64]
                                                        [--msssim-pairs random|caption] [--prdc-k K] [--mmd-subsets S] [--mmd-subset-size M]
                                                        [--style-dim D [--mapping-layers N] [--no-style-noise] [--modulated-conv] [--truncation-psi PSI]]

The generator's variables (`g_net`) are restored from CHECKPOINT_DIR/stage%d/; a failed load raises with the reference's
message.  The dataset is `TextDataset(DATASET_DIR, MODEL.SIZES[stage - 1])` (256 at stage 7, as the reference reads).  Per batch
of `--batch` (EVAL.SIZE // batch batches; 50 000 // 64 in the reference's configs), in the reference's order from the global
np.random stream: z ~ N(0, 1) [batch, 128], then `dataset.test.next_batch(batch, 4, embeddings=True)` (the means of four caption
embeddings), the generator with conditioning noise on (the reference's `gen_op`), clip to [-1, 1], the resize to 299 x 299 by
t2i_resample_bilinear straight from the fp32 images (denormalize_images + prep_incep_img, bit for bit), InceptionV3 and a float32
softmax.  Nothing is kept between batches: evaluation/evaluator.py's streamed evaluator, IS and FID both in chunks of the Inception
batch (default: `--batch`).

- evaluate_inception: the predictions in generation order, with NO shuffle, then get_inception_from_predictions(preds, 10), as
  the reference's evaluator does.
- evaluate_fid: an addition: the reference's PGGAN evaluator computes IS only.  The same batches' PreLogits statistics are
  streamed through t2i_gram_accumulate and compared with the real statistics of EVAL.ACT_STAT_PATH, which are computed from the
  images under EVAL.R_IMG_PATH first if the file is absent (as for wgancls); 500 on a failure, the other evaluators' fallback.

- evaluate_swd: an addition (evaluation/swd.py): the sliced Wasserstein distance between the Laplacian-pyramid patches of the
  test images and of the images generated from their embeddings, one value per level from the stage's resolution down to
  16 x 16 — the paper's own metric.  It needs no Inception net; stages 1 and 2 (4 x 4, 8 x 8) are too small for it.

- evaluate_msssim: an addition (evaluation/msssim.py): the multi-scale SSIM between pairs of generated images, the paper's
  diversity metric — `--msssim-pairs random` pairs image i of a batch with image i + batch // 2, `caption` pairs two images of one
  caption and different z.  It needs no Inception net; its five scales need images of at least 16 x 16, so stage 3 or later.

- evaluate_prdc: an addition (evaluation/prdc.py): precision, recall, density and coverage of the generated set against the real
  test images in Inception feature space (`--prdc-k K` nearest neighbours, default 5).  It needs the Inception checkpoint but not
  EVAL.ACT_STAT_PATH; `--ema` and `--stage` apply.

- evaluate_mmd: an addition (evaluation/mmd.py): the Kernel Inception distance (KID) of the same two feature sets, `--eval mmd`
  (`--mmd-subsets S` subsets, default 100, of `--mmd-subset-size M` rows at most, default 1000).  It needs what evaluate_prdc needs;
  `--ema` and `--stage` apply.

The PGGAN generator has no batch norm, so there is no training / inference mode to choose between the two."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.evaluation.evaluator import GeneratorEval  # noqa: E402
from t2i_amd.models import cli  # noqa: E402
from t2i_amd.models.pggan import options  # noqa: E402
from t2i_amd.models.pggan.pggan import PGGAN  # noqa: E402
from t2i_amd.utils.saver import restore_scopes  # noqa: E402


def stage_model(cfg, stage, batch_size, dataset, device, **kw):
    """The stage's PGGAN without its training graph (build_model=False), g_net created by a launch-free pass.  kw: the widths (fmap_base,
    fmap_max, z_dim, embed_dim, compr_embed_dim; default: the reference's) and the architecture the checkpoint was trained with
    (resample_filter, style_dim, ...: options.kwargs_of); restore_generator refuses a checkpoint built otherwise."""
    from t2i_amd.scope import trainable_variables
    m = PGGAN(batch_size=batch_size, steps=None, check_dir_write='', check_dir_read=os.path.join(cfg.CHECKPOINT_DIR, 'stage%d/' % stage),
              dataset=dataset, sample_path=None, log_dir=None, stage=stage, trans=False, build_model=False, device=device, **kw)
    if not trainable_variables('g_net'):
        with K.dry_run(), torch.no_grad():
            m.generator(torch.empty(batch_size, m.z_dim, device=m.device), torch.empty(batch_size, m.embed_dim, device=m.device),
                        stages=stage, t=False)
    return m


def restore_generator(m, ema=False):
    """ema=True: the moving average of the weights that `train_pggan.py --g-ema` keeps in the checkpoint, as the weights.
    The checkpoint's generator must be the model's, or its weights would be sampled through another function: a checkpoint built with
    another --style-dim, --mapping-layers, --no-style-noise or --modulated-conv (`train_pggan.py --style-dim`), or trained with other resampling taps
    (`g_net/resample_filter`, written by `train_pggan.py --resample-filter`; the key present in a model without taps and the taps given
    for a checkpoint without the key included), raises RuntimeError naming both sides, before any variable is read."""
    arch = options.checkpoint_architecture(m.check_dir_read)
    if arch is not None:
        ckpt_style, model_style = options.style_of_names(arch[0]), (m.style_dim, m.mapping_layers if m.style_dim is not None else None,
                                                                    m.style_noise if m.style_dim is not None else None)
        if ckpt_style != model_style:
            raise RuntimeError('the checkpoint in %s holds %s, but this model was built with %s: pass the same --style-dim / --mapping-layers / '
                               '--no-style-noise (style_dim=, mapping_layers=, style_noise=) the trainer was given' % (
                                   m.check_dir_read, options.describe_style(ckpt_style), options.describe_style(model_style)))
        if options.modulated_of_names(arch[0]) != m.modulated_conv:
            raise RuntimeError('the checkpoint in %s holds a generator with %s, but this model was built with %s: pass --modulated-conv '
                               '(modulated_conv=True) exactly when the trainer was given it' % (
                                   m.check_dir_read, options.describe_modulated(not m.modulated_conv), options.describe_modulated(m.modulated_conv)))
        if not options.same_taps(arch[1], m.resample_taps):
            raise RuntimeError('the checkpoint in %s was trained with %s, but this model resamples with %s: pass the same --resample-filter '
                               '(resample_filter=) the trainer was given' % (
                                   m.check_dir_read, options.describe_taps(arch[1]), options.describe_taps(m.resample_taps)))
    restore_scopes(m.store, [('g_net', m.check_dir_read)], error=lambda scope: RuntimeError('Could not load stage %d' % m.stage), verbose=False,
                   ema=ema)


def checkpoint_names(directory):
    """{variable name: shape} of the generator's mapping-network and style-block entries in the newest checkpoint of `directory` (what
    utils/saver.load would read); None when there is no checkpoint."""
    arch = options.checkpoint_architecture(directory)
    return None if arch is None else arch[0]


def generate(m, z, cond, cond_noise=True):
    """The stage generator on device tensors (fresh truncated-normal conditioning noise when cond_noise), clipped to [-1, 1]."""
    with torch.no_grad():
        m._ca = None
        m._sn = None                   # (style_dim: fresh style noise; the constructor's truncation_psi applies)
        img, _, _ = m.generator(z, cond, stages=m.stage, t=False, reuse=True, cond_noise=cond_noise)
        return torch.clamp(img.float(), -1.0, 1.0).contiguous()


class PGGANEval(GeneratorEval):
    stored = False
    keep_preds = True
    size_error = 'EVAL.SIZE %d is smaller than the batch %d'
    announce = {}
    ema = False                            # True: score the moving average of the generator's weights

    def batch_size(self):
        return self.model.batch_size

    def default_incep_batch_size(self):
        return self.bs                     # eval_pggan.py: incep_batch_size = batch_size

    def restore(self):
        restore_generator(self.model, ema=self.ema)

    def generate_batch(self, z, cond, is_training):
        return generate(self.model, z, cond)          # no batch norm: no mode


def load_stage_dataset(cfg, stage, device):
    from t2i_amd.preprocess.dataset import TextDataset
    datadir = cfg.DATASET_DIR
    dataset = TextDataset(datadir, cfg.MODEL.SIZES[stage - 1], device=device)
    dataset.test = dataset.get_data('%s/test' % datadir)
    dataset.train = dataset.get_data('%s/train' % datadir)
    return dataset


class Reader(object):
    """What the evaluator and the two visualisers do before their own work, with room for their own checks between the steps: the
    reader flags added to `ap`, `argv` parsed and the architecture keywords made of it (an argument error before anything else); the
    check that a stage has a checkpoint; the (dataset, model) of a stage on the device."""

    def __init__(self, ap, argv, widths):
        options.add_reader_arguments(ap)
        self.args = ap.parse_args(argv)
        self.kw = dict(widths, **options.kwargs_of(ap, self.args))

    @staticmethod
    def need_checkpoint(cfg, stage):
        d = os.path.join(cfg.CHECKPOINT_DIR, 'stage%d' % stage)
        if not os.path.isfile(os.path.join(d, 'checkpoint')):
            raise RuntimeError('Could not load stage %d (no checkpoint in %s)' % (stage, d))

    def open(self, cfg, stage, batch):
        """-> (the stage's dataset, its model at `batch`) on the device."""
        dev = torch.device('cuda')
        dataset = load_stage_dataset(cfg, stage, dev)
        return dataset, stage_model(cfg, stage, batch, dataset, dev, **self.kw)


def main(argv=None, **widths):
    from t2i_amd.utils.config import config_from_yaml
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', required=True, help='models/pggan/cfg/flowers.yml or birds.yml')
    ap.add_argument('--eval', choices=['is', 'fid', 'swd', 'msssim', 'prdc', 'mmd'], default='is')
    cli.add_pairs_argument(ap)
    cli.add_nearest_k_argument(ap)
    cli.add_subsets_arguments(ap)
    ap.add_argument('--stage', type=int, default=7, help='the stage whose generator is scored [7]')
    ap.add_argument('--batch', type=int, default=64, help='images generated (and scored) per batch [64]')
    ap.add_argument('--incep-batch', type=int, default=None, help='Inception batch (default: --batch)')
    ap.add_argument('--ema', action='store_true', help="score the moving average of the generator's weights (a checkpoint of train_pggan.py --g-ema)")
    reader = Reader(ap, argv, widths)
    args = reader.args
    if not 1 <= args.stage <= 8:
        ap.error('--stage must be in 1..8')
    if args.batch < 1 or (args.incep_batch is not None and args.incep_batch < 1):
        ap.error('--batch and --incep-batch must be positive')
    if args.eval in ('swd', 'msssim') and args.stage < 3:
        ap.error('--eval %s needs images of at least 16 x 16: --stage 3 or later' % args.eval)
    cli.check_pairs(ap, args)
    cli.check_nearest_k(ap, args)
    cli.check_subsets(ap, args)
    if args.eval == 'msssim' and args.msssim_pairs != 'caption' and args.batch < 2:
        ap.error('--eval msssim pairs image i of a batch with image i + batch // 2: --batch 2 or more (or --msssim-pairs caption)')
    cfg = config_from_yaml(args.cfg)
    reader.need_checkpoint(cfg, args.stage)
    if cfg.EVAL.SIZE // args.batch == 0:
        raise ValueError('EVAL.SIZE %d is smaller than --batch %d' % (cfg.EVAL.SIZE, args.batch))
    dataset, m = reader.open(cfg, args.stage, args.batch)
    ev = PGGANEval(None, m, dataset, cfg, incep_batch_size=args.incep_batch)
    ev.ema = args.ema
    out = cli.run_eval(ev, args.eval, args.msssim_pairs, args.prdc_k, cli.subsets_of(args))
    out.pop('preds', None)
    return out


if __name__ == '__main__':
    main()
