"""Entry point of the wgancls model — reference models/wgancls/run.py:13-74.

    python -m t2i_amd.models.wgancls.run --cfg <yaml> [--train | --visualize [--interp N] | --eval is|fid|swd|msssim|prdc|mmd [--incep-batch N]
                                         [--msssim-pairs random|caption] [--prdc-k K] [--mmd-subsets S] [--mmd-subset-size M]]
                                         [--synthetic] [--steps N] [--batch B] [--graphs 0|1]

Behaviour of the reference's main(): read the config, create CHECKPOINT_DIR / SAMPLE_DIR / LOGS_DIR, load the pickled
dataset from cfg.DATASET_DIR (`TextDataset(datadir, 64)`, splits `<datadir>/test` and `<datadir>/train`), then switch on
the mode flags: EVAL.FLAG -> Inception-score evaluation, TRAIN.FLAG -> `WGanClsTrainer(...).train()` with its periodic
side effects (captions, sample grids, checkpoints, resume), neither -> the caption visualiser.
Additions that the reference does not have, all explicit: `--train` forces the training mode whatever the yml says (the
shipped yml has TRAIN.FLAG: False); `--visualize` selects the caption visualiser (visualize_wgan.py) whatever TRAIN.FLAG
says, with `--interp N` rounds of interpolation sheets (the reference runs none) — without it TRAIN.FLAG: False still
raises, so that no run of the shipped yml starts something the caller did not ask for; `--eval is|fid` runs the
Inception-score or FID evaluator (eval_wgan.py) whatever EVAL.FLAG says, with `--incep-batch N` overriding
EVAL.INCEP_BATCH_SIZE, `--eval swd` the sliced Wasserstein distance per pyramid level (evaluation/swd.py; no Inception net) and
`--eval msssim` the multi-scale SSIM between pairs of generated images (evaluation/msssim.py; `--msssim-pairs caption` pairs two
images of one caption), `--eval prdc` precision, recall, density and coverage of the generated set in Inception feature space
(evaluation/prdc.py; `--prdc-k K` nearest neighbours, default 5; needs the Inception checkpoint but not EVAL.ACT_STAT_PATH),
`--eval mmd` the Kernel Inception distance (KID) of the same feature sets (evaluation/mmd.py; `--mmd-subsets S` subsets, default 100,
of `--mmd-subset-size M` rows at most, default 1000) —
EVAL.FLAG: True without it still raises, for the same reason; `--synthetic` replaces the pickled dataset by the on-device synthetic one
(t2i_amd.data) for machines without the data; `--steps` / `--batch` override TRAIN.MAX_STEPS / TRAIN.BATCH_SIZE."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd.models import cli  # noqa: E402
from t2i_amd.models.wgancls.model import WGanCls  # noqa: E402
from t2i_amd.models.wgancls.trainer import WGanClsTrainer  # noqa: E402
from t2i_amd.utils.config import config_from_yaml  # noqa: E402


def load_dataset(cfg, device, synthetic=False):
    """reference run.py:33-40.  The pickles are read once; images and caption embeddings then live in HBM."""
    if synthetic:
        from t2i_amd.data import SyntheticTextDataset
        return SyntheticTextDataset(cfg, device)
    from t2i_amd.preprocess.dataset import TextDataset
    datadir = cfg.DATASET_DIR
    if not os.path.isdir(datadir):
        raise FileNotFoundError('DATASET_DIR %r does not exist (expected <dir>/train and <dir>/test with the pickles of '
                                'preprocess/dataset.py); pass --synthetic to train on synthetic inputs instead' % datadir)
    dataset = TextDataset(datadir, cfg.MODEL.OUTPUT_SIZE, device=device)
    dataset.test = dataset.get_data('%s/test' % datadir)
    dataset.train = dataset.get_data('%s/train' % datadir)
    return dataset


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cfg', 'flowers.yml'),
                    help='Relative path to the config of the model')
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument('--train', action='store_true', help='train even if the yml says TRAIN.FLAG: False')
    mode.add_argument('--visualize', action='store_true', help='run the caption visualiser on the latest checkpoint (needs the '
                      'pickled dataset)')
    mode.add_argument('--eval', choices=('is', 'fid', 'swd', 'msssim', 'prdc', 'mmd'), default=None, help='run the Inception-score, FID, '
                      'sliced-Wasserstein, multi-scale-SSIM, precision / recall / density / coverage or Kernel Inception distance (mmd) evaluator on the latest checkpoint (needs the pickled dataset and, except '
                      'for swd and msssim, an Inception checkpoint in EVAL.INCEP_CHECKPOINT_DIR)')
    ap.add_argument('--incep-batch', type=int, default=None, help='--eval: Inception batch size (default EVAL.INCEP_BATCH_SIZE)')
    cli.add_pairs_argument(ap)
    cli.add_nearest_k_argument(ap)
    cli.add_subsets_arguments(ap)
    ap.add_argument('--interp', type=int, default=0, help='--visualize: rounds of interpolation / captioned sheets (default 0)')
    ap.add_argument('--synthetic', action='store_true', help='synthetic on-device dataset instead of cfg.DATASET_DIR')
    ap.add_argument('--steps', type=int, default=None, help='override TRAIN.MAX_STEPS')
    ap.add_argument('--batch', type=int, default=None, help='override TRAIN.BATCH_SIZE')
    ap.add_argument('--graphs', type=int, default=1, help='1: replay the iteration from hipGraphs once it has run eagerly (default)')
    args = ap.parse_args(argv)
    cli.check_pairs(ap, args)
    cli.check_nearest_k(ap, args)
    cli.check_subsets(ap, args)
    print(args.cfg)
    cfg = config_from_yaml(args.cfg)
    if args.batch:
        cfg.TRAIN.BATCH_SIZE = args.batch
    if args.steps:
        cfg.TRAIN.MAX_STEPS = args.steps
    for d in (cfg.CHECKPOINT_DIR, cfg.SAMPLE_DIR, cfg.LOGS_DIR):
        if not os.path.exists(d):
            os.makedirs(d)

    if args.incep_batch is not None and (not args.eval or args.incep_batch <= 0):
        raise ValueError('--incep-batch takes a positive batch size and needs --eval (got %r)' % args.incep_batch)
    if args.eval:
        if args.synthetic:
            raise ValueError('--eval needs the pickled dataset (embeddings are drawn from its test split); the --synthetic data '
                             'set has none')
        from t2i_amd.models.wgancls.eval_wgan import WGanClsEval
        wgan = WGanCls(cfg, build_model=False)           # the evaluator creates and restores the generator's variables only
        dataset = load_dataset(cfg, wgan.device)
        ev = WGanClsEval(sess=None, model=wgan, dataset=dataset, cfg=cfg, incep_batch_size=args.incep_batch)
        return cli.run_eval(ev, args.eval, args.msssim_pairs, args.prdc_k, cli.subsets_of(args))
    if cfg.EVAL.FLAG:
        raise NotImplementedError('EVAL.FLAG: pass --eval is or --eval fid to run the Inception-score / FID evaluation '
                                  '(reference models/wgancls/eval_wgan.py)')
    if args.visualize:
        if args.synthetic:
            raise ValueError('--visualize needs the pickled dataset (the neighbour search reads its uint8 image store); the '
                             '--synthetic data set has none')
        from t2i_amd.models.wgancls.visualize_wgan import WGanClsVisualizer
        wgan = WGanCls(cfg, build_model=False)           # the visualiser creates and restores the generator's variables only
        dataset = load_dataset(cfg, wgan.device)
        return WGanClsVisualizer(sess=None, model=wgan, dataset=dataset, config=cfg).visualize(interp=args.interp)
    if not (cfg.TRAIN.FLAG or args.train):
        raise NotImplementedError('TRAIN.FLAG is False: the reference would start its caption visualiser (visualize_wgan.py); '
                                  'pass --visualize for it, or --train / TRAIN.FLAG: True to train')

    from t2i_amd import kernels as K
    K.filter_cache(os.environ.get('T2I_FILTER_CACHE', '1') != '0')     # weights change only through Adam / Saver here
    wgan = WGanCls(cfg)
    dataset = load_dataset(cfg, wgan.device, synthetic=args.synthetic)
    trainer = WGanClsTrainer(sess=None, model=wgan, dataset=dataset, cfg=cfg)
    return trainer.train(side_effects=True, graphs=bool(args.graphs))


if __name__ == '__main__':
    main()
