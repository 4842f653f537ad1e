"""PGGAN's options, said once: what each one does and which values it takes (`validated`, which the constructor calls), the flags of
the entry points that set them (`add_trainer_arguments`, `add_reader_arguments`, `kwargs_of`: the same checks, speaking of the flag), and
what a checkpoint says about the two options that change the generator's function (`checkpoint_architecture`).  None of them is in the
reference; every default is the reference's model, variables, launches and checkpoint files."""
import math
import re

import numpy as np

from ...utils.ops import DiffAugmentSampler, diff_augment_policy
from ...utils.saver import latest_checkpoint

W_AVG = 'g_net/mapping/w_avg'                   # PGGAN(style_dim=D): the running mean of the style vector, [D], not trainable
RESAMPLE_KEY = 'g_net/resample_filter'          # the checkpoint entry of PGGAN(resample_filter=...): the taps divided by their sum, float32
PL_MEAN_KEY = 'pl_reg/pl_mean'                  # the checkpoint entry of PGGAN(pl_weight=...): the moving average of the path length, a float32 scalar


def _number(v, ok):
    """A real number (no bool, no string) that `ok` accepts; NaN fails every comparison."""
    return isinstance(v, (int, float)) and not isinstance(v, bool) and bool(ok(v))


def _count(v):
    return isinstance(v, int) and not isinstance(v, bool) and v >= 1


def normalised_taps(resample_filter, name='resample_filter'):
    """None -> None; a sequence of 2..8 finite taps with a positive sum -> (the taps as floats, taps / sum as a float32 array: what a
    checkpoint carries); anything else is a ValueError."""
    if resample_filter is None:
        return None
    try:
        k = tuple(float(t) for t in resample_filter)
    except (TypeError, ValueError):
        k = ()
    if isinstance(resample_filter, str) or not 2 <= len(k) <= 8 or not all(math.isfinite(t) for t in k) or not math.fsum(k) > 0.0:
        raise ValueError('%s must be None or a sequence of 2..8 finite taps with a positive sum (the low-pass filter of the '
                         'up- and downsampling, e.g. (1, 3, 3, 1)), got %r' % (name, resample_filter))
    norm = (np.asarray(k, dtype=np.float64) / math.fsum(k)).astype(np.float32)
    if not np.isfinite(norm).all():
        raise ValueError('%s %r does not normalise to finite float32 taps' % (name, resample_filter))
    return k, norm


def validated(batch_size, critic_norm=None, critic_mbstd=None, g_ema=None, equalized_lr=False, adam_lr=None, diffaug=None, diffaug_p=None,
              diffaug_adapt=False, diffaug_sampler=None, critic_sn=False, resample_filter=None, style_dim=None, mapping_layers=4,
              style_noise=True, truncation_psi=None, modulated_conv=False, pl_weight=None, pl_interval=4, pl_shrink=2, pl_decay=0.01,
              data_parallel=False, label=str):
    """The optional keywords of PGGAN, checked -> {attribute: value} as the constructor keeps them (numbers cast to float, the taps also
    normalised, the group of critic_mbstd picked); a bad value is a ValueError that names the keyword through `label` (the identity; an
    entry point passes `flag`, and the same sentence speaks of `--diffaug-p`)."""
    L = label
    # style_dim=D: the style-based generator of Karras et al. 2019.  A mapping network `g_net/mapping` (pixel norm
    # of [z, c], then mapping_layers dense + lrelu layers) turns [z, c] into a style vector w, and every conv -> layer_norm(relu) pair of the
    # generator becomes conv -> utils.ops.style_block (per-pixel noise unless style_noise=False, relu, instance norm, an affine map of w:
    # csrc/t2i_style.hip).  `feed['style_noise_{d,g}_<k>']` carry the noise images (drawn when missing); truncation_psi makes the sampler use
    # w_avg + psi (w - w_avg), training never truncates; the readers refuse a checkpoint built otherwise.  Style mixing, a learned constant
    # input and bf16 tensors are out of scope.
    # modulated_conv=True (needs style_dim; Karras et al. 2020): every such conv -> style block pair becomes one
    # utils.ops.modulated_conv2d instead: the style scales the convolution's input channels, the filter is demodulated per sample, and bias,
    # noise and relu follow in one epilogue (csrc/t2i_modconv.hip); no instance norm.  Variables `ModConv[_k]/...` in place of `Conv[_k]/...`
    # and `StyleMod[_k]/...`; the readers refuse a checkpoint of the other kind.
    if style_dim is not None and not _count(style_dim):
        raise ValueError('%s must be None (the reference\'s generator) or an integer >= 1 (the width of the style vector w), got %r' % (L('style_dim'), style_dim))
    if not _count(mapping_layers):
        raise ValueError('%s must be an integer >= 1 (the dense layers of the mapping network), got %r' % (L('mapping_layers'), mapping_layers))
    if not isinstance(style_noise, bool):
        raise ValueError('%s must be True or False, got %r' % (L('style_noise'), style_noise))
    if truncation_psi is not None and not _number(truncation_psi, math.isfinite):
        raise ValueError('%s must be None or a finite number (the sampler uses w_avg + psi (w - w_avg)), got %r' % (L('truncation_psi'), truncation_psi))
    if style_dim is None and truncation_psi is not None:
        raise ValueError('%s needs %s (the style-based generator whose w it truncates), which is None' % (L('truncation_psi'), L('style_dim')))
    if not isinstance(modulated_conv, bool):
        raise ValueError('%s must be True or False, got %r' % (L('modulated_conv'), modulated_conv))
    if modulated_conv and style_dim is None:
        raise ValueError('%s needs %s (the style-based generator whose convolutions it modulates), which is None' % (L('modulated_conv'), L('style_dim')))
    # pl_weight=W (needs modulated_conv; Karras et al. 2020, section 3.2): path-length regularisation.  On every
    # pl_interval-th generator step a second generator pass over the first max(1, B // pl_shrink) rows is differentiated to w against a
    # random image y, and W pl_interval mean((|J| - a)^2) joins G_loss in the same Adam step; a, the moving average of |J| with decay
    # pl_decay, lives on the device and in checkpoints as PL_MEAN_KEY.  The other generator steps, and the generator's function, are unchanged.
    if pl_weight is not None and not _number(pl_weight, lambda v: math.isfinite(v) and v > 0.0):
        raise ValueError('%s must be None or a finite weight > 0 (of the path-length penalty in the generator loss), got %r' % (L('pl_weight'), pl_weight))
    if not _count(pl_interval):
        raise ValueError('%s must be an integer >= 1 (the penalty joins every such generator step), got %r' % (L('pl_interval'), pl_interval))
    if not _count(pl_shrink):
        raise ValueError('%s must be an integer >= 1 (the penalty is taken over batch // it samples), got %r' % (L('pl_shrink'), pl_shrink))
    if not _number(pl_decay, lambda v: 0.0 < v <= 1.0):
        raise ValueError('%s must be a number in (0, 1] (how far the mean path length moves towards a step\'s), got %r' % (L('pl_decay'), pl_decay))
    if pl_weight is not None and not modulated_conv:
        raise ValueError('%s needs %s (the path-length penalty differentiates the generator twice, and the AdaIN layers of the other '
                         'generators have no second derivative)' % (L('pl_weight'), L('modulated_conv')))
    if pl_weight is not None and data_parallel:
        raise ValueError('%s under data parallelism is not done (the penalty and its mean path length are formed per process)' % L('pl_weight'))
    # resample_filter=(1, 3, 3, 1): utils.ops.upsample_2d for the generator's nearest x2 `upscale` and utils.ops.downsample_2d for the critic's
    # 2x2 `pool`, in the blocks and in both fade-in branches (Karras et al. 2019, Zhang 2019): one launch of
    # csrc/t2i_resample.hip each, differentiable to any order.  This changes the generator's function, so checkpoints carry the normalised
    # taps as RESAMPLE_KEY and the readers refuse a checkpoint whose taps differ from the model's.
    taps = normalised_taps(resample_filter, L('resample_filter'))
    # critic_sn=True: every conv2d / fc kernel of the critic divided by an estimate of its largest singular value (Miyato et al. 2018;
    # DESIGN.md section 4.40).  optim.SpectralNorm keeps the raw weights the critic's Adam steps and advances one power iteration per step,
    # inside D_optimizer.apply(); the variables, the checkpoints and every reader hold the normalised weights.
    if not isinstance(critic_sn, bool):
        raise ValueError('%s must be True or False, got %r' % (L('critic_sn'), critic_sn))
    # diffaug='color,translation,cutout' (or a subset): every image the critic sees, real or generated, goes through the differentiable
    # augmentation T of Zhao et al. (utils.ops.diff_augment).  The generator is trained through T, both gradient
    # penalties are gradients of D o T, and the sampler, checkpoints, evaluators and summaries never see it; the parameter tables are
    # `feed['aug_d']` [4B, 9] (rows G | x | x_mismatch | x_hat) and `feed['aug_g']` [B, 9], drawn when missing.
    if diffaug is not None:
        try:
            diff_augment_policy(diffaug, 'diffaug')
        except ValueError:
            raise ValueError("%s must be None or a comma-separated, non-empty subset of 'color,translation,cutout' (the "
                             "differentiable augmentation in front of the critic), got %r" % (L('diffaug'), diffaug))
    # diffaug_p=P applies each transform with probability P; diffaug_adapt=True steers P from D(x) and D(G) at the end of the critic step
    # (DESIGN.md section 4.39).  Either one moves the draw of a missing table into the step, as one launch of a utils.ops.DiffAugmentSampler
    # (`diffaug_sampler`, or the model's own) that a captured graph holds; the critic step then also returns `Dx_logit`, `Dg_logit`, `aug_p`.
    if diffaug_p is not None and not _number(diffaug_p, lambda p: 0.0 <= p <= 1.0):
        raise ValueError('%s must be None or a probability in [0, 1] (each transform of diffaug is applied with it), got %r' % (L('diffaug_p'), diffaug_p))
    if not isinstance(diffaug_adapt, bool):
        raise ValueError('%s must be True or False, got %r' % (L('diffaug_adapt'), diffaug_adapt))
    if diffaug_sampler is not None and not isinstance(diffaug_sampler, DiffAugmentSampler):
        raise ValueError('%s must be None or a utils.ops.DiffAugmentSampler, got %r' % (L('diffaug_sampler'), diffaug_sampler))
    if diffaug is None and (diffaug_p is not None or diffaug_adapt or diffaug_sampler is not None):
        raise ValueError('%s, %s and %s need %s (the policy they apply), which is None' % (
            L('diffaug_p'), L('diffaug_adapt'), L('diffaug_sampler'), L('diffaug')))
    if diffaug_sampler is not None and diffaug_sampler.mask != diff_augment_policy(diffaug, 'diffaug'):
        raise ValueError('%s draws for the policy %r, %s is %r' % (L('diffaug_sampler'), diffaug_sampler.policy, L('diffaug'), diffaug))
    if diffaug_sampler is not None and diffaug_adapt and diffaug_sampler.adapt is None:
        raise ValueError('%s=True, but the %s that was passed has adapt=None' % (L('diffaug_adapt'), L('diffaug_sampler')))
    # adam_lr=L: Adam's step size for both optimizers (the reference hard-codes 2e-6)
    if adam_lr is not None and not _number(adam_lr, lambda lr: math.isfinite(lr) and lr > 0.0):
        raise ValueError("%s must be None (the reference's 2e-6) or a finite step size > 0, got %r" % (L('adam_lr'), adam_lr))
    # equalized_lr=True (the progressive-growing paper's equalized learning rate): every conv2d / fc kernel is drawn
    # from N(0, c^2), c = sqrt(2 / fan_in), not truncated, and both optimizers get the per-slot multipliers (c, c): Adam on w-hat ~ N(0, 1)
    # used as c * w-hat, restated on w = c * w-hat itself, so the convolutions, the checkpoints and the readers see plain weights.  The gain
    # is sqrt(2) for every layer: the paper's gain 1 on the last linear layers (to_rgb's 1x1, the critic's last dense) is deliberately left
    # out.  Biases and the layer-norm gamma / beta keep the multiplier 1.
    if not isinstance(equalized_lr, bool):
        raise ValueError('%s must be True or False, got %r' % (L('equalized_lr'), equalized_lr))
    # g_ema=D (the paper's `Gs`): an exponential moving average of the generator's weights, formed in the generator's Adam launch, that
    # checkpoints carry and `ema_weights()` / `--ema` sample from
    if g_ema is not None and not _number(g_ema, lambda d: 0.0 < d < 1.0):
        raise ValueError("%s must be None or a decay in (0, 1) (the moving average of the generator's weights), got %r" % (L('g_ema'), g_ema))
    # critic_norm='layer' | 'pixel': the critic's 3x3 / 4x4 convolutions normalised per sample (PGGAN._d_conv)
    if critic_norm not in (None, 'layer', 'pixel'):
        raise ValueError("%s must be None, 'layer' or 'pixel', got %r" % (L('critic_norm'), critic_norm))
    # critic_mbstd=G: the paper's minibatch standard deviation in front of the critic's last block.  The group is
    # the largest divisor of the batch not above G (and the kernels' 16), so that groups of contiguous rows never straddle the B-row parts
    # of the critic's 3B pass; per rank under data parallelism (batch_size is the local batch).
    if critic_mbstd is not None and not _count(critic_mbstd):
        raise ValueError('%s must be None or an integer >= 1 (the group size of the minibatch standard deviation), got %r' % (L('critic_mbstd'), critic_mbstd))
    if critic_mbstd is not None and not _count(batch_size):
        raise ValueError('%s needs an integer batch_size >= 1 to pick its group size from, got %r' % (L('critic_mbstd'), batch_size))
    group = None if critic_mbstd is None else max(g for g in range(1, min(critic_mbstd, 16) + 1) if batch_size % g == 0)
    return dict(style_dim=style_dim, mapping_layers=mapping_layers, style_noise=style_noise, modulated_conv=modulated_conv,
                pl_weight=None if pl_weight is None else float(pl_weight), pl_interval=pl_interval, pl_shrink=pl_shrink, pl_decay=float(pl_decay),
                truncation_psi=None if truncation_psi is None else float(truncation_psi),
                resample_filter=None if taps is None else taps[0],        # the taps as given; None: nearest x2 and the 2x2 mean
                resample_taps=None if taps is None else taps[1],          # ... divided by their sum, float32: what checkpoints carry
                critic_sn=critic_sn, diffaug=diffaug, diffaug_p=diffaug_p, diffaug_adapt=diffaug_adapt, aug_sampler=diffaug_sampler,
                adam_lr=0.000002 if adam_lr is None else float(adam_lr), equalized_lr=equalized_lr, g_ema=None if g_ema is None else float(g_ema),
                critic_norm=critic_norm, critic_mbstd=critic_mbstd, mbstd_group=group)


# ---- the entry points' flags ----------------------------------------------------------------------------------------------------
def flag(keyword):
    """The flag that sets a keyword of `validated`: --diffaug-p for diffaug_p."""
    return {'adam_lr': '--lr', 'style_noise': '--no-style-noise'}.get(keyword) or '--' + keyword.replace('_', '-')


def add_resample_filter_argument(ap, reader=True):
    ap.add_argument('--resample-filter', default=None, metavar='TAPS',
                    help="low-pass filtered resampling in both networks (Karras et al. 2019, Zhang 2019): comma-separated taps, 2..8 of "
                         "them, finite, with a positive sum, e.g. 1,3,3,1; they replace the generator's nearest x2 upscale and the critic's "
                         "2x2 average pool%s (default: the reference's resampling)"
                         % (' - give the taps the checkpoint was trained with: a mismatch is refused' if reader else
                            '; checkpoints carry the taps and the evaluators and visualisers must be given the same'))


def add_style_arguments(ap, reader=True):
    """PGGAN's style-based generator: --style-dim, --mapping-layers, --no-style-noise, --modulated-conv, and for the readers --truncation-psi."""
    ap.add_argument('--style-dim', type=int, default=None, metavar='D',
                    help="the style-based generator (Karras et al. 2019): a mapping network turns [z, c] into a style vector w of D units, and "
                         "every generator convolution is followed by per-pixel noise, instance norm and an affine map of w%s (default: the "
                         "reference's generator)" % (' - give what the checkpoint was trained with: a mismatch is refused' if reader else
                                                     '; the evaluators and visualisers must be given the same'))
    ap.add_argument('--mapping-layers', type=int, default=None, metavar='N', help='--style-dim: dense layers of the mapping network (default 4)')
    ap.add_argument('--no-style-noise', action='store_true', help='--style-dim: build the style blocks without the per-pixel noise and its strengths')
    ap.add_argument('--modulated-conv', action='store_true',
                    help='--style-dim: weight-demodulated convolutions (Karras et al. 2020) in place of convolution + instance norm + style%s'
                         % (' - give it exactly when the checkpoint was trained with it: a mismatch is refused' if reader else
                            '; the evaluators and visualisers must be given the same'))
    if reader:
        ap.add_argument('--truncation-psi', type=float, default=None, metavar='PSI',
                        help='--style-dim: sample from w_avg + PSI (w - w_avg), w_avg the running mean of w the checkpoint carries (default: w itself)')


def add_reader_arguments(ap):
    """The flags of the evaluator and the visualisers: the architecture the checkpoint was trained with."""
    add_resample_filter_argument(ap)
    add_style_arguments(ap)


def add_trainer_arguments(ap):
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
    add_resample_filter_argument(ap, reader=False)
    add_style_arguments(ap, reader=False)
    ap.add_argument('--pl-weight', type=float, default=None, metavar='W',
                    help='--modulated-conv: path-length regularisation of the generator (Karras et al. 2020) with weight W > 0 (the '
                         'publication: 2); checkpoints carry the mean path length; the readers need no flag (default: none)')
    ap.add_argument('--pl-interval', type=int, default=None, metavar='N', help='--pl-weight: the penalty joins every N-th generator step (default 4)')
    ap.add_argument('--pl-shrink', type=int, default=None, metavar='K', help='--pl-weight: the penalty is taken over batch // K samples (default 2)')
    ap.add_argument('--pl-decay', type=float, default=None, metavar='D',
                    help="--pl-weight: the mean path length moves by D in (0, 1] of its distance to each step's (default 0.01)")
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


def kwargs_of(ap, args):
    """The PGGAN constructor keywords of whichever of the flags above `ap` has and `args` gives ({} when none is given: every default
    stays the constructor's).  A flag that needs another one that is missing, and every value `validated` refuses, is an argument error
    (exit status 2) that names the flag: before a directory is made or a device is touched."""
    given = vars(args).get
    taps = given('resample_filter')
    if taps is not None:
        try:
            taps = tuple(float(t) for t in taps.split(','))
        except ValueError:
            pass                                    # (left a string, which `validated` refuses by its text)
    if given('style_dim') is None and (given('mapping_layers') is not None or given('no_style_noise') or given('truncation_psi') is not None):
        ap.error('--mapping-layers / --no-style-noise / --truncation-psi need --style-dim (the generator they configure)')
    if given('style_dim') is None and given('modulated_conv'):
        ap.error('--modulated-conv needs --style-dim (the generator whose convolutions it modulates)')
    if given('pl_weight') is None and any(given(k) is not None for k in ('pl_interval', 'pl_shrink', 'pl_decay')):
        ap.error('--pl-interval / --pl-shrink / --pl-decay are the numbers of --pl-weight, which is not given')
    if given('diffaug') is None and (given('diffaug_p') is not None or given('diffaug_adapt')):
        ap.error('--diffaug-p / --diffaug-adapt need --diffaug (the policy they apply)')
    # the numbers of the run's sampler (`run_sampler`), which are no keywords of the model
    target, interval, ramp = given('diffaug_target'), given('diffaug_interval'), given('diffaug_ramp')
    if not given('diffaug_adapt') and (target is not None or interval is not None or ramp is not None):
        ap.error('--diffaug-target / --diffaug-interval / --diffaug-ramp are the numbers of --diffaug-adapt, which is not given')
    if target is not None and not -1.0 < target < 1.0:
        ap.error('--diffaug-target %r: the statistic lies in (-1, 1)' % target)
    if interval is not None and interval < 1:
        ap.error('--diffaug-interval %r: need at least one critic step per adjustment' % interval)
    if ramp is not None and not (0.0 < ramp < float('inf')):
        ap.error('--diffaug-ramp %r: the number of images must be positive and finite' % ramp)
    kw = dict(critic_norm=given('critic_norm'), critic_mbstd=given('critic_mbstd'), g_ema=given('g_ema'), adam_lr=given('lr'), diffaug=given('diffaug'),
              diffaug_p=given('diffaug_p'), resample_filter=taps, style_dim=given('style_dim'), mapping_layers=given('mapping_layers'),
              truncation_psi=given('truncation_psi'), style_noise=False if given('no_style_noise') else None,
              pl_weight=given('pl_weight'), pl_interval=given('pl_interval'), pl_shrink=given('pl_shrink'), pl_decay=given('pl_decay'),
              **{k: True for k in ('equalized_lr', 'critic_sn', 'diffaug_adapt', 'modulated_conv') if given(k)})
    kw = {k: v for k, v in kw.items() if v is not None}
    try:
        validated(1, label=flag, **kw)              # (batch 1: the group of --critic-mbstd is picked per entry, by the constructor)
    except ValueError as e:
        ap.error(str(e))
    return kw


def resample_filter_of(ap, args):
    """--resample-filter as a tuple of floats (None when absent); anything but 2..8 finite taps with a positive sum is an argument error."""
    return kwargs_of(ap, args).get('resample_filter')


style_kwargs_of = kwargs_of                         # ({} without --style-dim, on a parser that has add_style_arguments' flags alone)


def run_sampler(args, kw, device):
    """--diffaug-p / --diffaug-adapt: one sampler for the run, handed to every entry's model in place of `diffaug_p`, so that p and the call
    counter carry over from entry to entry.  -> `kw` as the constructors take it."""
    if args.diffaug_p is None and not args.diffaug_adapt:
        return kw
    numbers = {k: v for k, v in (('target', args.diffaug_target), ('interval', args.diffaug_interval), ('ramp_images', args.diffaug_ramp))
               if v is not None}
    kw = {k: v for k, v in kw.items() if k != 'diffaug_p'}
    return dict(kw, diffaug_adapt=args.diffaug_adapt, diffaug_sampler=DiffAugmentSampler(
        args.diffaug, p=0.0 if args.diffaug_p is None else args.diffaug_p, device=device, adapt='midpoint' if args.diffaug_adapt else None, **numbers))


# ---- what a checkpoint says about the generator it holds ------------------------------------------------------------------------
def same_taps(a, b):
    """Whether two normalised tap arrays (or None: no filter) describe the same resampling."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a, dtype=np.float32).reshape(-1), np.asarray(b, dtype=np.float32).reshape(-1)
    return a.shape == b.shape and bool((a == b).all())


def describe_taps(norm):
    """The taps of a message: 'no filter (nearest x2, 2x2 mean)' or the normalised values."""
    if norm is None:
        return 'no filter (nearest x2 upscale, 2x2 mean pool)'
    return 'the normalised taps (%s)' % ', '.join('%.6g' % float(t) for t in norm)


def style_of_names(names):
    """(style_dim, mapping_layers, style_noise) of the generator whose variables are `names` ({name: shape}); (None, None, None) for the
    reference's generator."""
    if W_AVG not in names:
        return (None, None, None)
    layers = sum(1 for n in names if re.match(r'^g_net/mapping/dense(_\d+)?/kernel$', n))
    return (int(names[W_AVG][0]), layers, any(n.endswith('/noise_strength') for n in names))


def describe_style(sig):
    """A (style_dim, mapping_layers, style_noise) triple in the flags' words."""
    if sig[0] is None:
        return "the reference's generator (no --style-dim)"
    return 'a style-based generator (--style-dim %d --mapping-layers %d%s)' % (sig[0], sig[1], '' if sig[2] else ' --no-style-noise')


def modulated_of_names(names):
    """Whether the generator whose variables are `names` has weight-demodulated convolutions (PGGAN(modulated_conv=True)): the bit beside
    style_of_names' triple."""
    return any('/ModConv' in n for n in names)


def describe_modulated(on):
    return 'weight-demodulated convolutions (--modulated-conv)' if on else 'convolution + AdaIN layers (no --modulated-conv)'


def checkpoint_architecture(directory):
    """What the newest checkpoint of `directory` (utils.saver.latest_checkpoint) says about its generator, in one open: ({name: shape} of
    the mapping-network, style-block and modulated-convolution entries, which style_of_names and modulated_of_names read; the RESAMPLE_KEY entry or None).  None without a checkpoint."""
    path = latest_checkpoint(directory)
    if path is None:
        return None
    with np.load(path) as z:
        names = {k: tuple(z[k].shape) for k in z.files if k.startswith('g_net/mapping/') or '/StyleMod' in k or '/ModConv' in k}
        return names, (z[RESAMPLE_KEY] if RESAMPLE_KEY in z.files else None)
