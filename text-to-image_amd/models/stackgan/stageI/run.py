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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd.models.cli import check_mode, make_dirs, make_parser, run_eval, subsets_of  # noqa: E402
from t2i_amd.utils.config import config_from_yaml  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

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
        return run_eval(StageIEval(sess=None, model=stage_i, dataset=dataset, cfg=cfg, incep_batch_size=args.incep_batch), args.eval, args.msssim_pairs, args.prdc_k, subsets_of(args))
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
