"""Stage driver of the progressive-growing schedule — reference models/pggan/train_pggan.py:17-69: stages
1, 2t, 2, 3t, 3, ... (t = fade-in transition), batch 16 (8 from stage 6 on), 600000 images per stage, checkpoints
written under `<CHECKPOINT_DIR>/stage<k>/` and read from the previous stage's directory.  `--iters` bounds the iterations
per stage (the full 600000 // batch when omitted).  `--style-dim D [--mapping-layers N] [--no-style-noise]` trains the style-based
generator (PGGAN(style_dim=D)).

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
from t2i_amd.models import cli  # noqa: E402
from t2i_amd.models.pggan.pggan import PGGAN  # noqa: E402
from t2i_amd.utils.config import AttrDict  # noqa: E402

STAGE = [1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8]            # train_pggan.py:19-20
PREV_STAGE = [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8]


def dataset_for(size, device):
    cfg = AttrDict({'MODEL': {'IMAGE_SHAPE': {'H': size, 'W': size, 'D': 3}, 'EMBED_DIM': 1024}})
    return SyntheticTextDataset(cfg, device)


def _has_checkpoint(directory):
    """What utils/saver.load will find: a `checkpoint` state file naming an archive that exists."""
    import re
    state = os.path.join(directory, 'checkpoint')
    if not os.path.isfile(state):
        return False
    m = re.search(r'model_checkpoint_path: "([^"]+)"', open(state).read())
    return bool(m) and os.path.isfile(os.path.join(directory, m.group(1)))


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
        if not _has_checkpoint(rdir):
            raise FileNotFoundError('entry %d (stage %d%s) starts from the stage-%d checkpoint in %s, which does not exist; run the '
                                    'earlier entries first (--first %d)' % (first, STAGE[first], 't' if first % 2 else '',
                                                                             PREV_STAGE[first], rdir, max(first - 1, 0)))


def real_dataset(cfg, stage, device):
    """train_pggan.py:53-60: the stage's TextDataset with both splits read."""
    from t2i_amd.preprocess.dataset import TextDataset
    datadir = cfg.DATASET_DIR
    dataset = TextDataset(datadir, cfg.MODEL.SIZES[stage - 1], device=device)
    dataset.test = dataset.get_data('%s/test' % datadir)
    dataset.train = dataset.get_data('%s/train' % datadir)
    return dataset


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default=None, help='config of the real-data run (models/pggan/cfg/flowers.yml); without it: synthetic data under --out')
    ap.add_argument('--out', default='./pggan_run/', help='output directory of the synthetic run (unused with --cfg)')
    ap.add_argument('--iters', type=int, default=None, help='iterations per stage (default: 600000 // batch as the reference)')
    ap.add_argument('--first', type=int, default=0, help='index into the 15-entry schedule to start from')
    ap.add_argument('--last', type=int, default=len(STAGE) - 1)
    ap.add_argument('--math', choices=['f32', 'bf16'], default='f32')
    ap.add_argument('--critic-norm', choices=['layer', 'pixel'], default=None,
                    help="normalise the critic's 3x3 / 4x4 convolutions per sample (default: the reference's un-normalised critic)")
    ap.add_argument('--critic-mbstd', type=int, default=None, metavar='G',
                    help="minibatch standard deviation in front of the critic's last block, over groups of (the largest divisor of the "
                         "batch not above) G samples (default: none, the reference's critic)")
    ap.add_argument('--g-ema', type=float, default=None, metavar='D',
                    help="keep an exponential moving average of the generator's weights with decay D in (0, 1) (the paper: 0.999); checkpoints "
                         "carry it, a second sample grid train_ema_* is drawn from it, and eval / visualize read it with --ema "
                         "(default: none)")
    ap.add_argument('--equalized-lr', action='store_true',
                    help="the paper's equalized learning rate: kernels drawn from N(0, 2 / fan_in) and stepped by Adam as c * w-hat with "
                         "w-hat ~ N(0, 1), c = sqrt(2 / fan_in), through per-slot multipliers in the Adam launch (default: the reference's "
                         "He initialisation and plain Adam)")
    ap.add_argument('--critic-sn', action='store_true',
                    help="spectral normalisation of the critic's conv and dense kernels (Miyato et al. 2018): one power iteration per "
                         "critic step next to the Adam launch; checkpoints carry the raw weights, u, v and sigma (default: none)")
    cli.add_resample_filter_argument(ap, reader=False)
    cli.add_style_arguments(ap, reader=False)
    ap.add_argument('--diffaug', default=None, metavar='POLICY',
                    help="differentiable augmentation of every image the critic sees (Zhao et al. 2020): a comma-separated subset of "
                         "color,translation,cutout (default: none)")
    ap.add_argument('--diffaug-p', type=float, default=None, metavar='P',
                    help='apply each transform of --diffaug to an image with probability P in [0, 1]; the tables are then drawn on the '
                         'device inside the step (default: every transform on every image, tables drawn by the tensor library)')
    ap.add_argument('--diffaug-adapt', action='store_true',
                    help="steer that probability from the critic's outputs on real images (Karras et al. 2020, restated for a "
                         "Wasserstein critic; starts from --diffaug-p, or 0); checkpoints carry it")
    ap.add_argument('--diffaug-target', type=float, default=None, metavar='R', help='--diffaug-adapt: the statistic to hold, in (-1, 1) (default 0.6)')
    ap.add_argument('--diffaug-interval', type=int, default=None, metavar='N', help='--diffaug-adapt: critic steps per adjustment (default 4)')
    ap.add_argument('--diffaug-ramp', type=float, default=None, metavar='IMAGES',
                    help='--diffaug-adapt: real images over which the probability can move from 0 to 1 (default 500000)')
    ap.add_argument('--lr', type=float, default=None, metavar='L', help="Adam's step size (default: the reference's hard-coded 2e-6)")
    ap.add_argument('--eager', action='store_true', help='--bench: keep eager launches instead of hipGraph replay')
    ap.add_argument('--bench', action='store_true', help='time `--iters` iterations of each entry instead of training with side effects')
    args = ap.parse_args(argv)
    taps = cli.resample_filter_of(ap, args)
    style = cli.style_kwargs_of(ap, args)
    if not 0 <= args.first <= args.last < len(STAGE):
        ap.error('--first %d / --last %d: need 0 <= first <= last <= %d' % (args.first, args.last, len(STAGE) - 1))
    if args.iters is not None and args.iters < 1:
        ap.error('--iters must be positive')
    if args.g_ema is not None and not 0.0 < args.g_ema < 1.0:          # (NaN fails both comparisons)
        ap.error('--g-ema %r: the decay must lie in (0, 1)' % args.g_ema)
    if args.lr is not None and not (0.0 < args.lr < float('inf')):      # (NaN fails both comparisons)
        ap.error('--lr %r: the step size must be a finite number > 0' % args.lr)
    if args.diffaug is not None:
        from t2i_amd.utils.ops import diff_augment_policy
        try:
            diff_augment_policy(args.diffaug, '--diffaug')
        except ValueError as e:
            ap.error(str(e))
    if args.diffaug is None and (args.diffaug_p is not None or args.diffaug_adapt):
        ap.error('--diffaug-p / --diffaug-adapt need --diffaug (the policy they apply)')
    if args.diffaug_p is not None and not 0.0 <= args.diffaug_p <= 1.0:          # (NaN fails both comparisons)
        ap.error('--diffaug-p %r: the probability must lie in [0, 1]' % args.diffaug_p)
    if not args.diffaug_adapt and (args.diffaug_target is not None or args.diffaug_interval is not None or args.diffaug_ramp is not None):
        ap.error('--diffaug-target / --diffaug-interval / --diffaug-ramp are the numbers of --diffaug-adapt, which is not given')
    if args.diffaug_target is not None and not -1.0 < args.diffaug_target < 1.0:
        ap.error('--diffaug-target %r: the statistic lies in (-1, 1)' % args.diffaug_target)
    if args.diffaug_interval is not None and args.diffaug_interval < 1:
        ap.error('--diffaug-interval %r: need at least one critic step per adjustment' % args.diffaug_interval)
    if args.diffaug_ramp is not None and not (0.0 < args.diffaug_ramp < float('inf')):
        ap.error('--diffaug-ramp %r: the number of images must be positive and finite' % args.diffaug_ramp)
    cfg = None
    if args.cfg is not None:
        from t2i_amd.utils.config import config_from_yaml
        if not os.path.isfile(args.cfg):
            raise FileNotFoundError('--cfg %s does not exist' % args.cfg)
        cfg = config_from_yaml(args.cfg)
        check_real_run(cfg, args.first, args.last, args.bench)
    K.set_math(args.math)
    dev = torch.device('cuda')
    aug_sampler = None
    if args.diffaug_p is not None or args.diffaug_adapt:
        # one sampler for the run, handed to every entry's model: p and the call counter carry over from entry to entry
        from t2i_amd.utils.ops import DiffAugmentSampler
        numbers = {k: v for k, v in (('target', args.diffaug_target), ('interval', args.diffaug_interval), ('ramp_images', args.diffaug_ramp))
                   if v is not None}
        aug_sampler = DiffAugmentSampler(args.diffaug, p=0.0 if args.diffaug_p is None else args.diffaug_p, device=dev,
                                         adapt='midpoint' if args.diffaug_adapt else None, **numbers)
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
                      log_dir=logs_dir, stage=STAGE[i], trans=t, device=dev, critic_norm=args.critic_norm,
                      critic_mbstd=args.critic_mbstd, **({} if args.g_ema is None else {'g_ema': args.g_ema}),
                      **({'equalized_lr': True} if args.equalized_lr else {}), **({} if args.lr is None else {'adam_lr': args.lr}),
                      **({'critic_sn': True} if args.critic_sn else {}), **({} if taps is None else {'resample_filter': taps}),
                      **({} if args.diffaug is None else {'diffaug': args.diffaug}), **style,
                      **({} if aug_sampler is None else {'diffaug_sampler': aug_sampler, 'diffaug_adapt': args.diffaug_adapt}))
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
