"""Stage driver of the progressive-growing schedule — reference models/pggan/train_pggan.py:17-69: stages
1, 2t, 2, 3t, 3, ... (t = fade-in transition), batch 16 (8 from stage 6 on), 600000 images per stage, checkpoints
written under `<CHECKPOINT_DIR>/stage<k>/` and read from the previous stage's directory.  `--iters` bounds the iterations
per stage (the full 600000 // batch when omitted).  The model's options are options.py's flags (`--critic-norm`, `--critic-mbstd`,
`--g-ema`, `--equalized-lr`, `--critic-sn`, `--resample-filter`, `--style-dim`, `--modulated-conv`, `--pl-weight`, `--diffaug`, `--diffaug-p`, `--diffaug-adapt`, `--lr`).

Without `--cfg`, synthetic data stands in for the pickled datasets and everything goes under `--out`.  With `--cfg <yml>`
(models/pggan/cfg/flowers.yml, birds.yml) the entry runs on the real dataset as the reference does: `TextDataset(DATASET_DIR,
MODEL.SIZES[stage - 1])` per entry, checkpoints in CHECKPOINT_DIR/stage%d/, sample grids and TensorBoard events in SAMPLE_DIR
and LOGS_DIR under stage%d/ or stage_t%d/, `train(side_effects=True, summaries=True)`; each entry's last iteration also writes
a sample grid next to its last checkpoint.  Every argument error, every missing image store (the stage-size stores come from
`python -m t2i_amd.preprocess.stage_images`) and a missing checkpoint of the stage the first entry starts from are reported
before any device work."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))

import torch  # noqa: E402
import t2i_amd  # noqa: E402,F401
from t2i_amd import kernels as K  # noqa: E402
from t2i_amd.data import SyntheticTextDataset  # noqa: E402
from t2i_amd.models.pggan import options  # noqa: E402
from t2i_amd.models.pggan.eval_pggan import load_stage_dataset as real_dataset  # noqa: E402  (train_pggan.py:53-60)
from t2i_amd.models.pggan.pggan import PGGAN  # noqa: E402
from t2i_amd.utils.config import AttrDict  # noqa: E402
from t2i_amd.utils.saver import latest_checkpoint  # noqa: E402

STAGE = [1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8]            # train_pggan.py:19-20
PREV_STAGE = [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8]


def dataset_for(size, device):
    cfg = AttrDict({'MODEL': {'IMAGE_SHAPE': {'H': size, 'W': size, 'D': 3}, 'EMBED_DIM': 1024}})
    return SyntheticTextDataset(cfg, device)


def check_real_run(cfg, first, last, bench=False):
    """Raises before any device work if an entry's image store or the first entry's starting checkpoint is missing."""
    from t2i_amd.preprocess.dataset import FINAL_SIZE_TO_ORIG, TextDataset
    sizes = list(cfg.MODEL.SIZES)
    if len(sizes) < max(STAGE[first:last + 1]):
        raise ValueError('MODEL.SIZES has %d entries; stage %d needs %d' % (len(sizes), max(STAGE[first:last + 1]), max(STAGE[first:last + 1])))
    datadir = cfg.DATASET_DIR
    for i in range(first, last + 1):
        size = sizes[STAGE[i] - 1]
        if size not in FINAL_SIZE_TO_ORIG or size != 4 * 2 ** (STAGE[i] - 1):
            raise ValueError('MODEL.SIZES[%d] = %d: stage %d generates %dx%d images' % (STAGE[i] - 1, size, STAGE[i], 4 * 2 ** (STAGE[i] - 1),
                                                                                    4 * 2 ** (STAGE[i] - 1)))
        for split in ('train', 'test'):
            d = os.path.join(datadir, split)
            for name in (TextDataset.EMBEDDINGS, TextDataset.FILENAMES, TextDataset.CLASSES):
                if not os.path.isfile(os.path.join(d, name)):
                    raise FileNotFoundError('%s is missing (DATASET_DIR %r: the reference preprocessing writes it)' % (os.path.join(d, name), datadir))
            store = os.path.join(d, '%dimages.pickle' % FINAL_SIZE_TO_ORIG[size])
            if not os.path.isfile(store):
                raise FileNotFoundError('%s is missing (stage %d trains on %dx%d crops of it); derive the stage-size stores from '
                                        '600images.pickle with: python -m t2i_amd.preprocess.stage_images --dir %s' % (
                                            store, STAGE[i], size, size, datadir))
    if not bench and STAGE[first] != 1:
        rdir = os.path.join(cfg.CHECKPOINT_DIR, 'stage%d/' % PREV_STAGE[first])
        if latest_checkpoint(rdir) is None:
            raise FileNotFoundError('entry %d (stage %d%s) starts from the stage-%d checkpoint in %s, which does not exist; run the '
                                    'earlier entries first (--first %d)' % (first, STAGE[first], 't' if first % 2 else '',
                                                                             PREV_STAGE[first], rdir, max(first - 1, 0)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=None, help='config of the real-data run (models/pggan/cfg/flowers.yml); without it: synthetic data under --out')
    ap.add_argument('--out', default='./pggan_run/', help='output directory of the synthetic run (unused with --cfg)')
    ap.add_argument('--iters', type=int, default=None, help='iterations per stage (default: 600000 // batch as the reference)')
    ap.add_argument('--first', type=int, default=0, help='index into the 15-entry schedule to start from')
    ap.add_argument('--last', type=int, default=len(STAGE) - 1)
    ap.add_argument('--math', choices=['f32', 'bf16'], default='f32')
    options.add_trainer_arguments(ap)
    ap.add_argument('--eager', action='store_true', help='--bench: keep eager launches instead of hipGraph replay')
    ap.add_argument('--bench', action='store_true', help='time `--iters` iterations of each entry instead of training with side effects')
    args = ap.parse_args(argv)
    if not 0 <= args.first <= args.last < len(STAGE):
        ap.error('--first %d / --last %d: need 0 <= first <= last <= %d' % (args.first, args.last, len(STAGE) - 1))
    if args.iters is not None and args.iters < 1:
        ap.error('--iters must be positive')
    kw = options.kwargs_of(ap, args)
    cfg = None
    if args.cfg is not None:
        from t2i_amd.utils.config import config_from_yaml
        if not os.path.isfile(args.cfg):
            raise FileNotFoundError('--cfg %s does not exist' % args.cfg)
        cfg = config_from_yaml(args.cfg)
        check_real_run(cfg, args.first, args.last, args.bench)
    K.set_math(args.math)
    dev = torch.device('cuda')
    kw = options.run_sampler(args, kw, dev)
    records = []
    for i in range(args.first, args.last + 1):
        t = (i % 2 == 1)
        batch_size = 8 if STAGE[i] >= 6 else 16
        max_iters = 600000 // batch_size
        sub = ('stage_t%d/' if t else 'stage%d/') % STAGE[i]
        if cfg is None:
            wdir = os.path.join(args.out, 'checkpoints', 'stage%d/' % STAGE[i])
            rdir = os.path.join(args.out, 'checkpoints', 'stage%d/' % PREV_STAGE[i])
            sample_path, logs_dir = os.path.join(args.out, 'samples', sub), None
        else:
            wdir = os.path.join(cfg.CHECKPOINT_DIR, 'stage%d/' % STAGE[i])
            rdir = os.path.join(cfg.CHECKPOINT_DIR, 'stage%d/' % PREV_STAGE[i])
            sample_path, logs_dir = os.path.join(cfg.SAMPLE_DIR, sub), os.path.join(cfg.LOGS_DIR, sub)
        for d in (wdir, rdir, sample_path) + ((logs_dir,) if logs_dir else ()):
            os.makedirs(d, exist_ok=True)
        size = 4 * 2 ** (STAGE[i] - 1)
        pggan = PGGAN(batch_size=batch_size, steps=max_iters, check_dir_write=wdir, check_dir_read=rdir,
                      dataset=dataset_for(size, dev) if cfg is None else real_dataset(cfg, STAGE[i], dev), sample_path=sample_path,
                      log_dir=logs_dir, stage=STAGE[i], trans=t, device=dev, **kw)
        if args.bench:
            gen = torch.Generator(device=dev).manual_seed(0)
            feed = pggan.make_feed(gen)
            for k in range(3):
                if k == 2 and not args.eager:
                    pggan.enable_graphs(feed)
                pggan.iteration(1 + k, feed)
            torch.cuda.synchronize()
            n = args.iters or 10
            t0 = time.perf_counter()
            for k in range(n):
                pggan.iteration(4 + k, feed)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            print('pggan stage %d%s  %3dx%-3d batch %2d  %s  %.2f ms/iteration  %.1f images/s' % (
                STAGE[i], 't' if t else ' ', size, size, batch_size, args.math + (' eager' if args.eager else ' graphs'), dt * 1e3, batch_size / dt))
        elif cfg is None:
            pggan.train(max_steps=args.iters, side_effects=True)
        else:
            pggan.train(max_steps=args.iters, side_effects=True, summaries=True, final_sample=True)
            pggan.writer.close()
        records.append(dict(entry=i, stage=STAGE[i], trans=t, restored=pggan.restored, checkpoint_dir=wdir, sample_path=sample_path,
                            logs_dir=logs_dir))
        del pggan
        torch.cuda.empty_cache()
    return records


if __name__ == '__main__':
    main()
