"""Entry point of StackGAN Stage II — reference models/stackgan/stageII/run.py:22-88.

    python -m t2i_amd.models.stackgan.stageII.run --cfg_stage_I <stage-I yaml> --cfg <stage-II yaml>
                                                  [--train | --eval is|fid|imd [--incep-batch N] | --visualize [--interp N]]
                                                  [--synthetic] [--steps N] [--batch B] [--graphs 0|1]

The modes and argument rules of stageI/run.py, on `TextDataset(DATASET_DIR, 256)` (304images.pickle).  Training restores the
Stage-I generator from the Stage-I config's CHECKPOINT_DIR (a warning if there is none) and checkpoints the Stage-II networks;
the evaluators and the caption visualiser (visualize_stageii.py, the reference's visualize_stageiI.py) chain the Stage-I and
Stage-II generators.  TRAIN.FLAG: False without `--train` / `--visualize` raises in place of the visualiser."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd.models.cli import check_mode, make_dirs, make_parser, run_eval, subsets_of  # noqa: E402
from t2i_amd.utils.config import config_from_yaml  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
STAGE_I_CFG = os.path.join(os.path.dirname(HERE), 'stageI', 'cfg', 'birds.yml')


def main(argv=None):
    ap = make_parser(os.path.join(HERE, 'cfg', 'birds.yml'))
    ap.add_argument('--cfg_stage_I', default=STAGE_I_CFG, help='Relative path to the config of the Stage-I model')
    args = ap.parse_args(argv)
    print(args.cfg_stage_I, args.cfg)
    cfg_stage_i = config_from_yaml(args.cfg_stage_I)
    cfg = config_from_yaml(args.cfg)
    if args.batch:
        cfg.TRAIN.BATCH_SIZE = cfg_stage_i.TRAIN.BATCH_SIZE = args.batch
    check_mode(args, cfg, 'visualize_stageiI.py')
    make_dirs(cfg)

    from t2i_amd.models.stackgan.stageI.model import ConditionalGan as ConditionalGanStageI
    from t2i_amd.models.stackgan.stageII.model import ConditionalGan
    from t2i_amd.models.wgancls.run import load_dataset
    stage_i = ConditionalGanStageI(cfg_stage_i, build_model=False)
    if args.eval:
        from t2i_amd.models.stackgan.stageII.eval_stageii import StageIIEval
        stage_ii = ConditionalGan(stage_i, cfg, build_model=False)
        dataset = load_dataset(cfg, stage_ii.device)
        return run_eval(StageIIEval(sess=None, model=stage_ii, dataset=dataset, cfg=cfg, incep_batch_size=args.incep_batch), args.eval, args.msssim_pairs, args.prdc_k, subsets_of(args))
    if args.visualize:
        from t2i_amd.models.stackgan.stageII.visualize_stageii import StageIIVisualizer
        stage_ii = ConditionalGan(stage_i, cfg, build_model=False)
        dataset = load_dataset(cfg, stage_ii.device)
        return StageIIVisualizer(sess=None, model=stage_ii, dataset=dataset, cfg=cfg).visualize(interp=args.interp)
    from t2i_amd.models.stackgan.stageII.trainer import ConditionalGanTrainer
    stage_ii = ConditionalGan(stage_i, cfg)
    dataset = load_dataset(cfg, stage_ii.device, synthetic=args.synthetic)
    trainer = ConditionalGanTrainer(sess=None, model=stage_ii, dataset=dataset, cfg=cfg, cfg_stage_i=cfg_stage_i)
    trainer.train(max_updates=args.steps, side_effects=True, graphs=bool(args.graphs))
    return trainer


if __name__ == '__main__':
    main()
