"""What the entry points of GAN-CLS and the two StackGAN stages share: the argument parser, the mode rules (every argument error is
raised before a directory is created or anything touches the GPU), the output directories and the evaluation switch."""
import argparse
import os

EVAL_MODES = ('is', 'fid', 'imd', 'swd')
PAIR_MODES = ('msssim',)            # evaluations of pairs of generated images: evaluate_<mode>(pairs=...)
PAIRINGS = ('random', 'caption')
FEATURE_MODES = ('prdc',)           # evaluations of the two feature SETS: evaluate_<mode>(nearest_k=...)
KNN_MAX_K = 8                       # kernels.KNN_MAX_K (not imported: argument errors come before anything touches the device library)
DEFAULT_NEAREST_K = 5
SUBSET_MODES = ('mmd',)             # evaluations over random subsets of the two feature sets: evaluate_<mode>(num_subsets=..., max_subset_size=...)
MAX_SUBSETS = 10000                 # evaluation.mmd.MAX_SUBSETS (not imported, as above)
DEFAULT_SUBSETS = (100, 1000)       # subsets, rows per subset at most: the published KID protocol


class Parser(argparse.ArgumentParser):
    """parse_args also runs the checks that span two arguments, so that they end as argument errors (exit status 2)."""

    def parse_args(self, *args, **kwargs):
        parsed = super(Parser, self).parse_args(*args, **kwargs)
        check_pairs(self, parsed)
        check_nearest_k(self, parsed)
        check_subsets(self, parsed)
        return parsed


def make_parser(default_cfg):
    ap = Parser()
    ap.add_argument('--cfg', default=default_cfg, help='Relative path to the config of the model')
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument('--train', action='store_true', help='train even if the yml says TRAIN.FLAG: False')
    mode.add_argument('--eval', choices=EVAL_MODES + PAIR_MODES + FEATURE_MODES + SUBSET_MODES, default=None, help='Inception score, FID, '
                      'Inception match distance, sliced Wasserstein distance, multi-scale SSIM between generated pairs, precision / recall / '
                      'density / coverage or the Kernel Inception distance (KID: --eval mmd) of the latest checkpoint (needs the pickled '
                      'dataset and, except for swd and msssim, an Inception checkpoint in EVAL.INCEP_CHECKPOINT_DIR)')
    mode.add_argument('--visualize', action='store_true', help='run the caption visualiser on the latest checkpoint (needs the '
                      'pickled dataset)')
    ap.add_argument('--incep-batch', type=int, default=None, help='--eval: Inception batch size (default EVAL.INCEP_BATCH_SIZE)')
    add_pairs_argument(ap)
    add_nearest_k_argument(ap)
    add_subsets_arguments(ap)
    ap.add_argument('--interp', type=int, default=0, help='--visualize: rounds of interpolation / captioned sheets (default 0)')
    ap.add_argument('--synthetic', action='store_true', help='--train: synthetic on-device dataset instead of cfg.DATASET_DIR')
    ap.add_argument('--steps', type=int, default=None, help='--train: stop after this many updates')
    ap.add_argument('--batch', type=int, default=None, help='override TRAIN.BATCH_SIZE')
    ap.add_argument('--graphs', type=int, default=1, help='1: replay the iteration from hipGraphs once it has run eagerly (default)')
    return ap


def add_pairs_argument(ap):
    ap.add_argument('--msssim-pairs', choices=PAIRINGS, default=None, help='--eval msssim: random: image i of a batch against image '
                    'i + batch // 2 (the paper\'s protocol); caption: every image against a second image of the same caption and a '
                    'fresh z (default random)')


def check_pairs(ap, args):
    """--msssim-pairs without --eval msssim is an argument error."""
    if args.msssim_pairs is not None and args.eval not in PAIR_MODES:
        ap.error('--msssim-pairs needs --eval msssim')


def add_nearest_k_argument(ap):
    ap.add_argument('--prdc-k', type=int, default=None, help='--eval prdc: the k of the k-nearest-neighbour balls, 1..%d (default %d, '
                    'the prdc package\'s; 3 reproduces the precision and recall of Kynkaanniemi et al.)' % (KNN_MAX_K, DEFAULT_NEAREST_K))


def check_nearest_k(ap, args):
    """--prdc-k without --eval prdc, or outside 1..KNN_MAX_K, is an argument error."""
    if args.prdc_k is not None:
        if args.eval not in FEATURE_MODES:
            ap.error('--prdc-k needs --eval prdc')
        if not 1 <= args.prdc_k <= KNN_MAX_K:
            ap.error('--prdc-k must be in 1..%d' % KNN_MAX_K)


def add_subsets_arguments(ap):
    ap.add_argument('--mmd-subsets', type=int, default=None, help='--eval mmd (KID): the number of random subsets the estimate is '
                    'averaged over, 1..%d (default %d)' % (MAX_SUBSETS, DEFAULT_SUBSETS[0]))
    ap.add_argument('--mmd-subset-size', type=int, default=None, help='--eval mmd (KID): rows per subset, at least 2; the smaller set '
                    'caps it (default %d)' % DEFAULT_SUBSETS[1])


def check_subsets(ap, args):
    """--mmd-subsets or --mmd-subset-size without --eval mmd, or out of range, is an argument error."""
    for flag, value, lo, hi in (('--mmd-subsets', args.mmd_subsets, 1, MAX_SUBSETS), ('--mmd-subset-size', args.mmd_subset_size, 2, None)):
        if value is not None:
            if args.eval not in SUBSET_MODES:
                ap.error('%s needs --eval mmd' % flag)
            if value < lo or (hi is not None and value > hi):
                ap.error('%s must be %s' % (flag, 'in %d..%d' % (lo, hi) if hi is not None else 'at least %d' % lo))


def subsets_of(args):
    """-> run_eval's `subsets`: (--mmd-subsets, --mmd-subset-size), None where a flag was not given."""
    return (args.mmd_subsets, args.mmd_subset_size)


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


EVAL_METHODS = dict(zip(EVAL_MODES + PAIR_MODES + FEATURE_MODES + SUBSET_MODES,
                        ('evaluate_inception', 'evaluate_fid', 'evaluate_imd', 'evaluate_swd', 'evaluate_msssim', 'evaluate_prdc',
                         'evaluate_mmd')))


def run_eval(ev, mode, pairs=None, nearest_k=None, subsets=None):
    """The requested mode's method only, looked up by name; a pair mode takes the pairing (default random), a feature mode the k of
    its nearest-neighbour balls (default 5), a subset mode `subsets` = (number of subsets, rows per subset at most), None or a None
    entry standing for the default (100, 1000)."""
    fn = getattr(ev, EVAL_METHODS[mode])
    if mode in PAIR_MODES:
        return fn(pairs=pairs or PAIRINGS[0])
    if mode in FEATURE_MODES:
        return fn(nearest_k=nearest_k or DEFAULT_NEAREST_K)
    if mode in SUBSET_MODES:
        n, size = subsets or (None, None)
        return fn(num_subsets=n or DEFAULT_SUBSETS[0], max_subset_size=size or DEFAULT_SUBSETS[1])
    return fn()
