"""Entry point of StackGAN Stage I — reference models/stackgan/stageI/run.py:20-79.

    python -m t2i_amd.models.stackgan.stageI.run --cfg <yaml> [--train | --eval is|fid|imd [--incep-batch N] | --visualize [--interp N]]
                                                 [--synthetic] [--steps N] [--batch B] [--graphs 0|1]

As models/wgancls/run.py follows its reference: read the config, create CHECKPOINT_DIR / SAMPLE_DIR / LOGS_DIR, load
`TextDataset(DATASET_DIR, 64)` (76images.pickle) with its test and train splits, then switch on the mode.  `--train` trains with
the reference's side effects (captions, sample grids, checkpoints, resume) whatever TRAIN.FLAG says; `--eval is|fid|imd` runs
eval_stagei.py's evaluator whatever EVAL.FLAG says (`--incep-batch` overrides EVAL.INCEP_BATCH_SIZE; `imd` is an addition the
reference does not have); `--visualize` runs the caption visualiser (visualize_stagei.py) with `--interp N` rounds of interpolation
sheets (the reference runs none).  EVAL.FLAG without `--eval` raises, and TRAIN.FLAG: False without `--train` / `--visualize` raises
instead of starting the visualiser, so that no run starts something the caller did not ask for.  `--synthetic` trains on the
on-device synthetic data set; `--steps` bounds the updates of this run.  Every argument error is raised before a directory is
created or anything touches the GPU.  The throughput loop of models/stackgan/run.py is unchanged."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd.utils.config import config_from_yaml  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EVAL_MODES = ('is', 'fid', 'imd')


def make_parser(default_cfg):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=default_cfg, help='Relative path to the config of the model')
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument('--train', action='store_true', help='train even if the yml says TRAIN.FLAG: False')
    mode.add_argument('--eval', choices=EVAL_MODES, default=None, help='Inception score, FID or Inception match distance of the '
                      'latest checkpoint (needs the pickled dataset and an Inception checkpoint in EVAL.INCEP_CHECKPOINT_DIR)')
    mode.add_argument('--visualize', action='store_true', help='run the caption visualiser on the latest checkpoint (needs the '
                      'pickled dataset)')
    ap.add_argument('--incep-batch', type=int, default=None, help='--eval: Inception batch size (default EVAL.INCEP_BATCH_SIZE)')
    ap.add_argument('--interp', type=int, default=0, help='--visualize: rounds of interpolation / captioned sheets (default 0)')
    ap.add_argument('--synthetic', action='store_true', help='--train: synthetic on-device dataset instead of cfg.DATASET_DIR')
    ap.add_argument('--steps', type=int, default=None, help='--train: stop after this many updates')
    ap.add_argument('--batch', type=int, default=None, help='override TRAIN.BATCH_SIZE')
    ap.add_argument('--graphs', type=int, default=1, help='1: replay the iteration from hipGraphs once it has run eagerly (default)')
    return ap


def check_mode(args, cfg, visualiser):
    """The mode errors, raised before any device work and before a directory is created."""
    if args.incep_batch is not None and (not args.eval or args.incep_batch <= 0):
        raise ValueError('--incep-batch takes a positive batch size and needs --eval (got %r)' % args.incep_batch)
    if args.steps is not None and args.steps <= 0:
        raise ValueError('--steps takes a positive number of updates (got %r)' % args.steps)
    if args.interp < 0 or (args.interp and not args.visualize):
        raise ValueError('--interp takes a non-negative number of rounds and needs --visualize (got %r)' % args.interp)
    if args.eval:
        if args.synthetic:
            raise ValueError('--eval needs the pickled dataset (embeddings are drawn from its test split); the --synthetic data '
                             'set has none')
        return
    if cfg.EVAL.FLAG:
        raise NotImplementedError('EVAL.FLAG: pass --eval is, --eval fid or --eval imd to run the evaluation')
    if args.visualize:
        if args.synthetic:
            raise ValueError('--visualize needs the pickled dataset (the neighbour search reads its uint8 image store); the '
                             '--synthetic data set has none')
        return
    if not (cfg.TRAIN.FLAG or args.train):
        raise NotImplementedError('TRAIN.FLAG is False: the reference would start its caption visualiser (%s); pass --visualize '
                                  'for it, --train / TRAIN.FLAG: True to train or --eval to evaluate' % visualiser)


def make_dirs(cfg):
    for d in (cfg.CHECKPOINT_DIR, cfg.SAMPLE_DIR, cfg.LOGS_DIR):
        if not os.path.exists(d):
            os.makedirs(d)


def run_eval(ev, mode):
    return {'is': ev.evaluate_inception, 'fid': ev.evaluate_fid, 'imd': ev.evaluate_imd}[mode]()


def main(argv=None):
    args = make_parser(os.path.join(HERE, 'cfg', 'birds.yml')).parse_args(argv)
    print(args.cfg)
    cfg = config_from_yaml(args.cfg)
    if args.batch:
        cfg.TRAIN.BATCH_SIZE = args.batch
    check_mode(args, cfg, 'visualize_stagei.py')
    make_dirs(cfg)

    from t2i_amd.models.stackgan.stageI.model import ConditionalGan
    from t2i_amd.models.wgancls.run import load_dataset
    if args.eval:
        from t2i_amd.models.stackgan.stageI.eval_stagei import StageIEval
        stage_i = ConditionalGan(cfg, build_model=False)     # the evaluator creates and restores the generator's variables only
        dataset = load_dataset(cfg, stage_i.device)
        return run_eval(StageIEval(sess=None, model=stage_i, dataset=dataset, cfg=cfg, incep_batch_size=args.incep_batch), args.eval)
    if args.visualize:
        from t2i_amd.models.stackgan.stageI.visualize_stagei import StageIVisualizer
        stage_i = ConditionalGan(cfg, build_model=False)     # the visualiser creates and restores the generator's variables only
        dataset = load_dataset(cfg, stage_i.device)
        return StageIVisualizer(sess=None, model=stage_i, dataset=dataset, cfg=cfg).visualize(interp=args.interp)
    from t2i_amd.models.stackgan.stageI.trainer import ConditionalGanTrainer
    stage_i = ConditionalGan(cfg)
    dataset = load_dataset(cfg, stage_i.device, synthetic=args.synthetic)
    trainer = ConditionalGanTrainer(sess=None, model=stage_i, dataset=dataset, cfg=cfg)
    trainer.train(max_updates=args.steps, side_effects=True, graphs=bool(args.graphs))
    return trainer


if __name__ == '__main__':
    main()
