"""Entry point of the InceptionV3 fine-tuning — reference models/inception/run_incep.py.

    python -m t2i_amd.models.inception.run_incep --cfg <yaml>

Reads the config, creates CHECKPOINT_DIR and LOGS_DIR, loads the dataset's TEST split at 299 x 299 (`TextDataset(DATASET_DIR,
299)`, `<dir>/test/360images.pickle`: its classes are the ones the GANs never see) and, with TRAIN.FLAG, runs
InceptionTrainer.train(); without it, does nothing, as the reference does."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import t2i_amd  # noqa: E402,F401
from t2i_amd.utils.config import config_from_yaml  # noqa: E402

DEFAULT_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cfg', 'flowers.yaml')


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=DEFAULT_CFG, help='Relative path to the config of the model [cfg/flowers.yaml]')
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    print(args.cfg)
    cfg = config_from_yaml(args.cfg)
    for d in (cfg.CHECKPOINT_DIR, cfg.LOGS_DIR):
        if not os.path.exists(d):
            os.makedirs(d)
    if not cfg.TRAIN.FLAG:
        return None
    import torch
    from t2i_amd.models.inception.trainer import InceptionTrainer
    from t2i_amd.preprocess.dataset import TextDataset
    device = torch.device('cuda', torch.cuda.current_device())
    dataset = TextDataset(cfg.DATASET_DIR, 299, device=device)
    # trained on the test split, whose classes are disjoint from the train split the GANs see
    dataset.test = dataset.get_data('%s/test' % cfg.DATASET_DIR)
    return InceptionTrainer(sess=None, dataset=dataset, cfg=cfg, device=device).train()


if __name__ == '__main__':
    main()
