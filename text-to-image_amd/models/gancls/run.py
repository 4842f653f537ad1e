"""Entry point of the GAN-CLS model — reference models/gancls/run.py:19-71.

    python -m t2i_amd.models.gancls.run --cfg <yaml> [--train | --eval is|fid|imd [--incep-batch N] | --visualize [--interp N]]
                                        [--synthetic] [--steps N] [--batch B] [--graphs 0|1]

As the reference's main(): read the config, create CHECKPOINT_DIR / SAMPLE_DIR / LOGS_DIR, load `TextDataset(DATASET_DIR, 64)`
with its test and train splits, then switch on the mode.  The modes are explicit, as in the sibling entry points: `--train`
trains with the reference's side effects (sampled captions, 8 x 8 grids, checkpoints, resume) whatever TRAIN.FLAG says;
`--eval is|fid|imd` runs eval_gancls.py's evaluator whatever EVAL.FLAG says (`--incep-batch` overrides EVAL.INCEP_BATCH_SIZE;
`fid` and `imd` are additions to the reference's run.py, which only starts the Inception score); `--visualize` runs the caption
visualiser (visualize_gancls.py) with `--interp N` rounds of interpolation sheets (the reference runs none).  EVAL.FLAG without
`--eval` raises, and TRAIN.FLAG: False without `--train` / `--visualize` raises instead of starting the visualiser, so that no run of
the shipped yml starts something the caller did not ask for.  `--synthetic` trains on the on-device synthetic data set; `--steps`
bounds the updates of this run.  Every argument error is raised before anything touches the GPU or the file system."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd.models.cli import check_mode, make_dirs, make_parser, run_eval, subsets_of  # noqa: E402
from t2i_amd.utils.config import config_from_yaml  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

def main(argv=None):
    args = make_parser(os.path.join(HERE, 'cfg', 'flowers.yml')).parse_args(argv)
    print(args.cfg)
    cfg = config_from_yaml(args.cfg)
    if args.batch:
        cfg.TRAIN.BATCH_SIZE = args.batch
    check_mode(args, cfg, 'visualize_gancls.py')
    make_dirs(cfg)

    from t2i_amd.models.gancls.model import GanCls
    from t2i_amd.models.wgancls.run import load_dataset
    if args.eval:
        from t2i_amd.models.gancls.eval_gancls import GanClsEval
        gancls = GanCls(cfg, build_model=False)          # the evaluator creates and restores the generator's variables only
        dataset = load_dataset(cfg, gancls.device)
        return run_eval(GanClsEval(sess=None, model=gancls, dataset=dataset, cfg=cfg, incep_batch_size=args.incep_batch), args.eval, args.msssim_pairs, args.prdc_k, subsets_of(args))
    if args.visualize:
        from t2i_amd.models.gancls.visualize_gancls import GanClsVisualizer
        gancls = GanCls(cfg, build_model=False)          # the visualiser creates and restores the generator's variables only
        dataset = load_dataset(cfg, gancls.device)
        return GanClsVisualizer(sess=None, model=gancls, dataset=dataset, config=cfg).visualize(interp=args.interp)
    from t2i_amd.models.gancls.trainer import GanClsTrainer
    gancls = GanCls(cfg)
    dataset = load_dataset(cfg, gancls.device, synthetic=args.synthetic)
    trainer = GanClsTrainer(sess=None, model=gancls, dataset=dataset, cfg=cfg)
    trainer.train(max_updates=args.steps, side_effects=True, graphs=bool(args.graphs))
    return trainer


if __name__ == '__main__':
    main()
