"""PGGAN — the reference's conditional progressive-growing GAN (reference models/pggan/pggan.py:12-394) on libt2i_hip.so
kernels.

Same class, constructor arguments and method names as the reference.  One `PGGAN` object = one (stage, trans) of the
schedule in train_pggan.py:17-69: output size 4 * 2^(stage-1); with `trans` the new resolution is faded in with
alpha = iter / steps next to the up-scaled previous `to_rgb` (generator) / the pooled-input `from_rgb` (critic).
The losses reuse the hot path's WGAN-GP machinery (gradient penalty through a double-differentiable critic); new
here: per-sample layer norm (generator only), 2x2 average pool and nearest x2 upscale (a pair of adjoint kernels, closed
under differentiation — the critic is differentiated twice), the fade-in mix.  The keywords from `critic_norm` on are
not in the reference; every default is the reference's model, and options.py describes each one where it checks it.
Reference specifics kept: penalty coefficient 200, no kt term, G = -D_fake + 5 KL, Adam(2e-6, beta1=0, beta2=0.99)
(pggan.py:104-110; `adam_lr` replaces the step size; the `learning_rate` placeholder is fed but unused), eps of x_hat
drawn in-graph (pggan.py:68 overrides the placeholder),
`to_rgb` = k2 s1 SAME 9-channel relu conv + 1x1, every kernel He-initialised by utils/ops.py's defaults.
`fmap_base` / `fmap_max` / the three sizes generalise the hard-coded 1024 / 512 / 128 / 1024 / 128 (defaults = the
reference's) so that the golden step can be tiny.
alpha: the reference assigns `alpha_tra = iter / steps` under a control dependency of D_optim only (pggan.py:76-77,112);
whether the critic step's own forward sees the new or the previous value is a TF scheduling race.  Here alpha is set
from `iter` BEFORE the critic step and kept for the generator step and the sampler — the assign-first order."""
import contextlib
import math
import sys
import time

import torch

from ... import autograd as A
from ... import kernels as K
from ... import optim
from ... import scope as S
from ...graphs import DGSchedule, StepGraphs
from ...utils.saver import Saver, load, save
from ...utils.ops import (DiffAugmentSampler, concat_tile, conv2d, diff_augment, diff_augment_params, downsample_2d, fc, layer_norm, lerp,
                          lrelu_act, minibatch_stddev_stat, modulated_conv2d, pixel_norm, pool, relu, style_block, upsample_2d, upscale)
from .options import PL_MEAN_KEY, RESAMPLE_KEY, W_AVG, checkpoint_architecture, describe_taps, same_taps, validated
from .options import normalised_taps, style_of_names  # noqa: F401  (importable from here, as before)

W_AVG_DECAY = 0.995
STYLE_NOISE_CUT = 6.0                           # the style noise is kernels.trunc_normal_'s inverse-CDF draw cut at +-6 sigma: a standard normal to 24 bits


class PGGAN(object):
    def __init__(self, batch_size, steps, check_dir_write, check_dir_read, dataset, sample_path, log_dir, stage, trans,
                 build_model=True, device=None, seed=0, store=None, fmap_base=1024, fmap_max=512, z_dim=128, embed_dim=1024,
                 compr_embed_dim=128, dp=None, critic_norm=None, critic_mbstd=None, g_ema=None, equalized_lr=False, adam_lr=None,
                 diffaug=None, diffaug_p=None, diffaug_adapt=False, diffaug_sampler=None, critic_sn=False, resample_filter=None,
                 style_dim=None, mapping_layers=4, style_noise=True, truncation_psi=None, modulated_conv=False, pl_weight=None, pl_interval=4,
                 pl_shrink=2, pl_decay=0.01):
        # pl_weight, pl_interval, pl_shrink, pl_decay, style_dim, mapping_layers, style_noise, truncation_psi, modulated_conv, resample_filter, resample_taps, critic_sn, diffaug, diffaug_p, diffaug_adapt,
        # aug_sampler (the model's own is made below, on the store's device), adam_lr, equalized_lr, g_ema, critic_norm, critic_mbstd, mbstd_group
        vars(self).update(validated(
            batch_size, critic_norm=critic_norm, critic_mbstd=critic_mbstd, g_ema=g_ema, equalized_lr=equalized_lr, adam_lr=adam_lr, diffaug=diffaug,
            diffaug_p=diffaug_p, diffaug_adapt=diffaug_adapt, diffaug_sampler=diffaug_sampler, critic_sn=critic_sn, resample_filter=resample_filter,
            style_dim=style_dim, mapping_layers=mapping_layers, style_noise=style_noise, truncation_psi=truncation_psi,
            modulated_conv=modulated_conv, pl_weight=pl_weight, pl_interval=pl_interval, pl_shrink=pl_shrink, pl_decay=pl_decay,
            data_parallel=dp is not None))
        self._second_order = False                # the generator pass of the path-length penalty builds its modulated convolutions twice differentiable
        self._sn = None                           # where the style blocks take their noise from: (feed, 'd' | 'g'), a list of images, or None (drawn)
        self.resample_restored = None             # train(): the taps of the checkpoint the last restore read (None: it had none)
        self.critic_spectral = None
        self.spectral_synced = None               # train(): how many normalised kernels the last restore had to sync from their weights
        self.batch_size, self.steps = batch_size, steps
        self.check_dir_write, self.check_dir_read = check_dir_write, check_dir_read
        self.dataset, self.sample_path, self.log_dir = dataset, sample_path, log_dir
        self.stage, self.trans = stage, trans
        self.z_dim, self.embed_dim, self.compr_embed_dim = z_dim, embed_dim, compr_embed_dim
        self.fmap_base, self.fmap_max = fmap_base, fmap_max
        self.out_size = self.output_size = 4 * pow(2, stage - 1)
        self.channel = 3
        self.sample_num = 64
        self.lr = 0.00005
        self.lr_inp = self.lr
        self.store = S.set_default_store(store or S.VariableStore(device=device, seed=seed))
        self.device = self.store.device
        self.alpha_tra = 0.0                      # tf.Variable(0.0, trainable=False, name='alpha_tra')
        self._alpha_dev = torch.zeros(1, device=self.device)      # ... kept in device memory: graph-replayable fade-in
        # pl_weight: the moving average of the path length, a device scalar updated in place on due generator steps (graph-replayable, like w_avg)
        self.pl_mean = torch.zeros((), device=self.device) if self.pl_weight is not None else None
        self._graphs = None
        self.restored = None
        # data parallelism (BASELINE config 5 "DP=8"; the reference is single-device): an optional dp.DataParallel — replicas
        # at local batch `batch_size`, critic and generator gradients all-reduced over RCCL, bucketed and overlapped with the
        # backward when eager, exchanged between captured graph segments under replay (same contract as models/wgancls)
        self.dp = dp
        if self.aug_sampler is None and (diffaug_p is not None or diffaug_adapt):
            # device tables with probability p; adapting alone starts from p = 0 like the publication; under
            # data parallelism each rank draws its own stream and steers its own p, as each rank draws its own table without this
            self.aug_sampler = DiffAugmentSampler(diffaug, p=0.0 if diffaug_p is None else float(diffaug_p), seed=seed + (dp.rank if dp is not None else 0),
                                                  device=self.device, adapt='midpoint' if diffaug_adapt else None)
        if build_model:
            self.build_model()
            self.define_losses()

    # ---- graph ---------------------------------------------------------------------------------------------------------
    def build_model(self):
        """pggan.py:44-82: variable creation by a launch-free dry pass, generator first."""
        B, dev = self.batch_size, self.device
        with K.dry_run(), torch.no_grad():
            z = torch.empty(B, self.z_dim, device=dev)
            cond = torch.empty(B, self.embed_dim, device=dev)
            G, _, _ = self.generator(z, cond, stages=self.stage, t=self.trans)
            self.discriminator(G, cond, reuse=False, stages=self.stage, t=self.trans)
        self.d_vars = S.trainable_variables('d_net')
        self.g_vars = S.trainable_variables('g_net')
        self.d_arena = optim.Arena(self.d_vars)
        self.g_arena = optim.Arena(self.g_vars)
        self.d_arena.enable_sinks()
        self.g_arena.enable_sinks()

    def get_gradient_penalty(self, x, y):
        with A.input_grads_only():
            grad_y, = torch.autograd.grad(y.sum(), [x], create_graph=True)
        return self._penalty(grad_y)

    get_gradient_penalty2 = get_gradient_penalty

    @staticmethod
    def _penalty(grad_y):
        slopes = A.GpSlopesFn.apply(grad_y)
        return torch.mean(torch.clamp(slopes - 1.0, min=0.0) ** 2)

    def define_losses(self):
        """pggan.py:84-130 (the optimizers; the loss expressions are in d_losses / g_losses)."""
        self.gp_coeff, self.kl_coeff = 200.0, 5.0
        if self.critic_sn:
            # over the kernels kernel_scales selects: every 4-D `weights` and 2-D `kernel` of the critic; the same u on every rank
            self.critic_spectral = optim.SpectralNorm(self.d_arena, self.kernel_names(self.d_vars))
        self.D_optimizer = optim.AdamTF(self.d_arena, 0.0, 0.99, slot_scales=self.kernel_scales(self.d_vars),
                                        **({} if self.critic_spectral is None else {'spectral': self.critic_spectral}))
        self.G_optimizer = optim.AdamTF(self.g_arena, 0.0, 0.99, ema_decay=self.g_ema,       # (None: no shadow, the plain launch)
                                        slot_scales=self.kernel_scales(self.g_vars))
        self.schedule = DGSchedule(self.dp, self.d_losses, self.d_arena, self.D_optimizer, self.g_losses, self.g_arena, self.G_optimizer)

    @staticmethod
    def kernel_names(variables):
        """The conv2d (`weights` [kh, kw, Cin, f]) and fc (`kernel` [in, units]) kernels among `variables`."""
        return [n for n, v in variables.items() if (n.endswith('/weights') and v.dim() == 4) or (n.endswith('/kernel') and v.dim() == 2)]

    def kernel_scales(self, variables):
        """equalized_lr: name -> c = sqrt(2 / fan_in) for every conv2d (`weights` [kh, kw, Cin, f]) and fc (`kernel` [in, units])
        kernel among `variables`, the fan_in utils/ops.py initialises them with; None without the flag (the plain Adam launches)."""
        if not self.equalized_lr:
            return None
        scales = {}
        for n, v in variables.items():
            if n.endswith('/weights') and v.dim() == 4:
                scales[n] = math.sqrt(2.0 / (v.shape[0] * v.shape[1] * v.shape[2]))
            elif n.endswith('/kernel') and v.dim() == 2:
                scales[n] = math.sqrt(2.0 / v.shape[0])
                if n.startswith('g_net/mapping/'):          # the mapping network's learning-rate multiplier (Karras et al. 2019)
                    scales[n] = (scales[n], 0.01)
        return scales

    def _init(self, fan_in):
        """The kernel initialiser handed to conv2d / fc: None (their He default) or, with equalized_lr, N(0, 2 / fan_in)."""
        return S.normal_init(math.sqrt(2.0 / fan_in)) if self.equalized_lr else None

    def _conv2d(self, x, f, ks, **kw):
        return conv2d(x, f=f, ks=ks, init=self._init(ks[0] * ks[1] * x.shape[-1]), **kw)

    def _fc(self, x, units, **kw):
        return fc(x, units=units, init=self._init(x.shape[-1]), **kw)

    def _noise(self, feed, key, like):
        n = feed.get(key)
        if n is None:
            n = K.trunc_normal_(torch.empty_like(like))
        return n

    def _aug_table(self, feed, key, rows, size):
        """The fed parameter table of the differentiable augmentation ([rows, 9], utils.ops.diff_augment), or a fresh draw (under data
        parallelism each rank draws its own): by the sampler's kernel when there is one (a launch, capturable), else by the tensor library."""
        P = feed.get(key)
        if P is None and self.aug_sampler is not None:
            P = self.aug_sampler.draw(rows, size[0], size[1])
        elif P is None:
            P = diff_augment_params(rows, size[0], size[1], self.diffaug, device=self.device)
        return P

    def d_losses(self, feed):
        """What sess.run([D_optim, D_loss]) evaluates before the update (pggan.py:62-73,84-100).  Gradients -> d_arena."""
        x, xm, cond, z = feed['x'], feed['x_mismatch'], feed['cond'], feed['z']
        B, st, t = x.shape[0], self.stage, self.trans
        aug = self._aug_table(feed, 'aug_d', 4 * B, x.shape[1:3]) if self.aug_sampler is not None else None      # the first launch: the sampler's call k
        eps = feed.get('eps_graph')
        if eps is None:        # tf.random_uniform([B,1,1,1]) in the graph: the fed `epsilon` placeholder is shadowed
            eps = torch.rand(B, device=x.device)
        with torch.no_grad():
            self._ca = self._noise(feed, 'ca_noise_d', cond[:, :self.compr_embed_dim])
            self._sn = (feed, 'd')
            G, _, _ = self.generator(z, cond, stages=st, t=t, reuse=True)
            x_hat = K.interp(eps.reshape(B, 1, 1, 1).contiguous(), G, x)
        # D(G), D(x), D(x_mismatch) as one pass over 3B samples: without critic_mbstd the critic has no batch coupling; with it the
        # coupling is inside groups of contiguous rows whose size divides B, so no group straddles two of the three parts, and the
        # statistic of the 3B rows is bit for bit that of three B-row passes
        images = torch.cat([G, x, xm], 0)
        if self.diffaug is not None:
            # every image the critic sees goes through T: rows [G | x | x_mismatch | x_hat] of one table, the 3B
            # pass as one call (a sample's result does not depend on its batch); both penalties are gradients of D o T
            if aug is None:
                aug = self._aug_table(feed, 'aug_d', 4 * B, x.shape[1:3])
            images = diff_augment(images, aug[:3 * B], self.diffaug)
        logits = self.discriminator(images, torch.cat([cond, cond, cond], 0), reuse=True, stages=st, t=t).view(3, B)
        Dg_logit, Dx_logit, Dxmi_logit = logits[0], logits[1], logits[2]
        x_hat.requires_grad_(True)            # before T: the penalty differentiates the adjoint kernel, and its backward
        cond_inp = (cond + 0.0).requires_grad_(True)
        Dx_hat_logit = self.discriminator(x_hat if aug is None else diff_augment(x_hat, aug[3 * B:], self.diffaug), cond_inp, reuse=True,
                                          stages=st, t=t)
        with A.input_grads_only():
            gx, gc = torch.autograd.grad(Dx_hat_logit.sum(), [x_hat, cond_inp], create_graph=True)
        real_gp, real_gp2 = self._penalty(gx), self._penalty(gc)
        D_loss_real, D_loss_fake, D_loss_mismatch = Dx_logit.mean(), Dg_logit.mean(), Dxmi_logit.mean()
        wdist, wdist2 = D_loss_real - D_loss_fake, D_loss_real - D_loss_mismatch
        D_loss = -wdist - wdist2 + self.gp_coeff * (real_gp + real_gp2)
        self.schedule.backward(self.d_arena, [D_loss], None, self.d_vars.values())
        out = dict(D_loss=D_loss.detach(), wdist=wdist.detach(), wdist2=wdist2.detach(), real_gp=real_gp.detach(),
                   real_gp2=real_gp2.detach(), reg_loss=(Dxmi_logit.detach() ** 2).mean(), G=G, Dx_hat_logit=Dx_hat_logit.detach(),
                   D_loss_real=D_loss_real.detach(), D_loss_fake=D_loss_fake.detach(), D_loss_mismatch=D_loss_mismatch.detach())
        if self.aug_sampler is not None:
            # the controller sees D(x) and D(G) alone (x_mismatch and x_hat take no part): the last launch of the step; p stays on the device
            out.update(Dx_logit=Dx_logit.detach(), Dg_logit=Dg_logit.detach())
            if self.diffaug_adapt:
                self.aug_sampler.observe(out['Dx_logit'], out['Dg_logit'])
            out['aug_p'] = self.aug_sampler.p_tensor().clone()
        return out

    def g_losses(self, feed, pl=False):
        """pl (pl_weight only): this generator step is due for the path-length penalty (iteration: idx % pl_interval == 0)."""
        if pl:
            return self._g_losses_pl(feed)
        cond, z = feed['cond'], feed['z']
        aug = None
        if self.aug_sampler is not None:          # the first launch, as in d_losses: call k + 1
            aug = self._aug_table(feed, 'aug_g', z.shape[0], (self.out_size, self.out_size))
        self._ca = self._noise(feed, 'ca_noise_g', cond[:, :self.compr_embed_dim])
        self._sn = (feed, 'g')
        G, mean, log_sigma = self.generator(z, cond, stages=self.stage, t=self.trans, reuse=True)
        if self.style_dim is not None:            # the truncation's centre follows the batch mean of w: in place, no host value, capturable
            with torch.no_grad():
                self.store.vars[W_AVG].lerp_(self._w.detach().mean(0), 1.0 - W_AVG_DECAY)
        if self.diffaug is not None and aug is None:
            aug = self._aug_table(feed, 'aug_g', G.shape[0], G.shape[1:3])
        G_seen = G if self.diffaug is None else diff_augment(G, aug, self.diffaug)
        with self.store.frozen('d_net'):
            Dg_logit = self.discriminator(G_seen, cond, reuse=True, stages=self.stage, t=self.trans)
        G_kl_loss = self.kl_std_normal_loss(mean, log_sigma)
        G_loss = -Dg_logit.mean() + self.kl_coeff * G_kl_loss
        self.schedule.backward(self.g_arena, [G_loss], None, self.g_vars.values())
        return dict(G_loss=G_loss.detach(), G_kl_loss=G_kl_loss.detach(), G=G.detach(), D_loss_fake=Dg_logit.detach().mean())

    def pl_due(self, idx):
        """Whether generator step `idx` (the argument of iteration) carries the path-length penalty."""
        return self.pl_weight is not None and idx % self.pl_interval == 0

    def _g_losses_pl(self, feed):
        """g_losses on a due step of the path-length regulariser (Karras et al. 2020, section 3.2): the generator
        step as it is, plus a second generator pass over rows [:Bp], Bp = max(1, B // pl_shrink), of the same z, cond, conditioning noise and
        style-noise images (a sample's bits do not depend on its batch: the pass equals the main pass on those rows) with twice-differentiable
        modulated convolutions; J = d sum(G y) / dw under input_grads_only, L = |J| per sample, a' = a + pl_decay (mean(L) - a) written back
        to pl_mean in place, pen = mean((L - a')^2) with a' a constant, and one backward of G_loss + pl_weight pl_interval pen.  y is
        feed['pl_noise'] [Bp,H,W,3] (independent N(0,1) / sqrt(H W) values) or a fresh draw."""
        if self.pl_weight is None:
            raise ValueError('g_losses(pl=True) needs a model built with pl_weight')
        cond, z = feed['cond'], feed['z']
        B = z.shape[0]
        Bp = max(1, B // self.pl_shrink)
        aug = None
        if self.aug_sampler is not None:
            aug = self._aug_table(feed, 'aug_g', B, (self.out_size, self.out_size))
        self._ca = self._noise(feed, 'ca_noise_g', cond[:, :self.compr_embed_dim])
        noise = {}                                # both passes see the same style-noise images: the fed ones, or one draw
        for k, size in self.style_noise_keys():
            if k.startswith('style_noise_g_'):
                n = feed.get(k)
                noise[k] = n if n is not None else K.trunc_normal_(torch.empty((B, size, size), device=self.device), a=-STYLE_NOISE_CUT, b=STYLE_NOISE_CUT)
        self._sn = (noise, 'g')
        G, mean, log_sigma = self.generator(z, cond, stages=self.stage, t=self.trans, reuse=True)
        with torch.no_grad():
            self.store.vars[W_AVG].lerp_(self._w.detach().mean(0), 1.0 - W_AVG_DECAY)
        if self.diffaug is not None and aug is None:
            aug = self._aug_table(feed, 'aug_g', G.shape[0], G.shape[1:3])
        G_seen = G if self.diffaug is None else diff_augment(G, aug, self.diffaug)
        with self.store.frozen('d_net'):
            Dg_logit = self.discriminator(G_seen, cond, reuse=True, stages=self.stage, t=self.trans)
        G_kl_loss = self.kl_std_normal_loss(mean, log_sigma)
        G_loss = -Dg_logit.mean() + self.kl_coeff * G_kl_loss
        # ---- the regulariser
        y = feed.get('pl_noise')
        if y is None:
            y = self.draw_pl_noise(torch.empty((Bp, self.out_size, self.out_size, self.channel), device=self.device))
        if tuple(y.shape) != (Bp, self.out_size, self.out_size, self.channel):
            raise ValueError('pl_noise must be %s, got %s' % ((Bp, self.out_size, self.out_size, self.channel), tuple(y.shape)))
        self._ca = self._ca[:Bp].contiguous()
        self._sn = ({k: n[:Bp].contiguous() for k, n in noise.items()}, 'g')
        self._second_order = True
        try:
            Gp, _, _ = self.generator(z[:Bp].contiguous(), cond[:Bp].contiguous(), stages=self.stage, t=self.trans, reuse=True)
        finally:
            self._second_order = False
        w = self._w
        with A.input_grads_only():
            J, = torch.autograd.grad((Gp * y).sum(), [w], create_graph=True)
        length = torch.sqrt((J * J).sum(1))
        with torch.no_grad():
            self.pl_mean.add_(self.pl_decay * (length.detach().mean() - self.pl_mean))       # a' = a + decay (mean(L) - a), in place
        penalty = ((length - self.pl_mean.detach()) ** 2).mean()
        total = G_loss + (self.pl_weight * self.pl_interval) * penalty
        self.schedule.backward(self.g_arena, [total], None, self.g_vars.values())
        return dict(G_loss=G_loss.detach(), G_kl_loss=G_kl_loss.detach(), G=G.detach(), D_loss_fake=Dg_logit.detach().mean(),
                    pl_penalty=penalty.detach(), pl_length=length.detach().mean(), pl_mean=self.pl_mean.clone())

    @staticmethod
    def draw_pl_noise(out):
        """The regulariser's random image y, in place: independent standard normals (cut at +-6 sigma like the style noise) / sqrt(H W)."""
        K.trunc_normal_(out, a=-STYLE_NOISE_CUT, b=STYLE_NOISE_CUT)
        return out.mul_(1.0 / math.sqrt(out.shape[1] * out.shape[2]))

    def set_alpha(self, value):
        self.alpha_tra = float(value)
        self._alpha_dev.fill_(self.alpha_tra)

    def _d_body(self, feed):
        return self.schedule.step(self.schedule.d, feed)

    def _g_body(self, feed):
        return self.schedule.step(self.schedule.g, feed)

    def enable_graphs(self, feed):
        """Capture the two halves of the iteration into hipGraphs (call after one eager iteration), cut at the exchange under data
        parallelism (graphs.DGSchedule.capture).  alpha then lives in device memory, and the in-graph random draws of the reference
        (eps of x_hat, the conditioning noise) become static buffers that are re-drawn before every replay."""
        B, dev = feed['x'].shape[0], self.device
        feed = dict(feed)
        drawn = (('eps_graph', (B,)), ('ca_noise_d', (B, self.compr_embed_dim)), ('ca_noise_g', (B, self.compr_embed_dim)))
        if self.diffaug is not None and self.aug_sampler is None:      # the two parameter tables of the augmentation: static buffers, re-drawn like eps_graph
            drawn += (('aug_d', (4 * B, 9)), ('aug_g', (B, 9)))
        drawn += tuple((k, (B, size, size)) for k, size in self.style_noise_keys())      # one image per style block and step, re-drawn like ca_noise_*
        if self.pl_weight is not None:            # the regulariser's image y: a static buffer, re-drawn before every due replay
            drawn += (('pl_noise', (max(1, B // self.pl_shrink), self.out_size, self.out_size, self.channel)),)
        for k, shape in drawn:
            if feed.get(k) is None:
                feed[k] = torch.empty(shape, device=dev)
        # with a sampler the tables are drawn inside the captured bodies (one launch each); a table that is fed stays a static input
        fed = ('aug_d', 'aug_g') if self.aug_sampler is not None else ()
        self._graphs = StepGraphs(feed, ('x', 'x_mismatch', 'cond', 'z') + tuple(k for k, _ in drawn) + fed,
                                  filters=(self.d_arena.flat, self.g_arena.flat))
        self._redraw(feed)
        self._graphs.load(feed)
        # pl_weight: both forms of the generator half; iteration picks one by idx, on the host
        self.schedule.capture(self._graphs, g_forms=None if self.pl_weight is None else {'g': {}, 'g_pl': {'pl': True}})

    def _redraw(self, feed, pl=False):
        st = self._graphs.static
        if feed.get('eps_graph') is None or feed['eps_graph'] is st['eps_graph']:
            st['eps_graph'].uniform_(0.0, 1.0)
        for k in ('ca_noise_d', 'ca_noise_g'):
            if feed.get(k) is None or feed[k] is st[k]:
                K.trunc_normal_(st[k])
        for k, _ in self.style_noise_keys():
            if feed.get(k) is None or feed[k] is st[k]:
                K.trunc_normal_(st[k], a=-STYLE_NOISE_CUT, b=STYLE_NOISE_CUT)
        if self.diffaug is not None and self.aug_sampler is None:
            size = st['x'].shape[1:3]
            for k in ('aug_d', 'aug_g'):
                if feed.get(k) is None or feed[k] is st[k]:
                    diff_augment_params(st[k].shape[0], size[0], size[1], self.diffaug, out=st[k])
        if pl and (feed.get('pl_noise') is None or feed['pl_noise'] is st['pl_noise']):      # last, and on due steps only: the other draws keep their order
            self.draw_pl_noise(st['pl_noise'])

    def iteration(self, idx, feed):
        """One D update then one G update (pggan.py:196-197)."""
        self.set_alpha(float(idx) / float(self.steps))           # alpha_assign (see the module docstring)
        if self._graphs is not None:
            if self.aug_sampler is not None and any(feed.get(k) is not None and k not in self._graphs.static for k in ('aug_d', 'aug_g')):
                raise ValueError('a parameter table is fed, but the graphs were captured drawing it: feed aug_d / aug_g to enable_graphs too')
            self._redraw(feed, pl=self.pl_due(idx))
        if self.pl_due(idx):                      # the generator half with the path-length penalty: picked here, no host value enters a graph
            return self.schedule.run(feed, self.adam_lr, self.adam_lr, graphs=self._graphs, g_form=('g_pl', {'pl': True}))
        return self.schedule.run(feed, self.adam_lr, self.adam_lr, graphs=self._graphs)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the generator's variables hold the moving average and the shadow holds the weights; on exit they are
        exchanged back, bit for bit.  Both exchanges write filter memory behind the optimizer's back, so the arena's cached filter
        images are dropped both times.  Not inside a capture (the exchange is host-ordered work around the sampler, not a step)."""
        opt = getattr(self, 'G_optimizer', None)
        if opt is None or opt.ema is None:
            raise RuntimeError('this model keeps no moving average of the generator (g_ema=None)')
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ema_weights() cannot run inside a graph capture')
        flat, ema = self.g_arena.flat, opt.ema

        def exchange():
            with torch.no_grad():
                tmp = flat.clone()
                flat.copy_(ema)
                ema.copy_(tmp)
            K.filter_cache_invalidate(flat)
        exchange()
        try:
            yield self
        finally:
            exchange()

    def sampler(self, z_sample, cond_sample, noise=None, truncation_psi=None):
        """noise (style_dim only): one [B,S,S] image per style block, in order (style_noise_keys gives the sizes); None draws fresh
        ones.  truncation_psi (style_dim only; default: the constructor's): w_avg + psi (w - w_avg) in place of w."""
        if self.style_dim is None and (noise is not None or truncation_psi is not None):
            raise ValueError('noise and truncation_psi belong to the style-based generator (style_dim), which this model does not have')
        with torch.no_grad():
            self._ca = None
            self._sn = None if noise is None else list(noise)
            try:
                return self.generator(z_sample, cond_sample, reuse=True, stages=self.stage, t=self.trans, truncation_psi=truncation_psi)[0]
            finally:
                self._sn = None

    def style_noise_keys(self):
        """[(feed key, map extent)] of the style-noise images of one iteration: `style_noise_d_<k>` and `style_noise_g_<k>` for block k
        (two per conv stage, 4 x 4 upwards); empty without style_dim or with style_noise=False."""
        if self.style_dim is None or not self.style_noise:
            return []
        sizes = [4 * 2 ** i for i in range(self.stage) for _ in range(2)]
        return [('style_noise_%s_%d' % (tag, k), size) for tag in ('d', 'g') for k, size in enumerate(sizes)]

    # ---- networks ------------------------------------------------------------------------------------------------------
    def discriminator(self, inp, cond, stages, t, reuse=False):
        """-> logits [B]  (pggan.py:251-281)"""
        alpha_trans = self._alpha_dev
        act = lrelu_act()
        with S.variable_scope('d_net', reuse=reuse):
            x_iden = None
            if t:
                x_iden = self.from_rgb(self._down(inp), stages - 2)
            x = self.from_rgb(inp, stages - 1)
            for i in range(stages - 1, 0, -1):
                with S.variable_scope(self.get_conv_scope_name(i), reuse=reuse):
                    x = self._d_conv(x, self.get_dnf(i), (3, 3), 'SAME', act)
                    x = self._d_conv(x, self.get_dnf(i - 1), (3, 3), 'SAME', act)
                    x = self._down(x)
                if i == stages - 1 and t:
                    x = lerp(x_iden, x, alpha_trans)              # alpha * x + (1 - alpha) * x_iden
            with S.variable_scope(self.get_conv_scope_name(0), reuse=reuse):
                cond_compress = self._fc(cond, units=self.compr_embed_dim, act=act)
                if self.mbstd_group is not None:        # [features | tiled compressed cond | tiled stat], the stat channels last
                    cond_compress = torch.cat([cond_compress, minibatch_stddev_stat(x, self.mbstd_group, self.mbstd_features(x.shape[-1]))], 1)
                concat = self.concat_cond4(x, cond_compress)
                x_b1 = self._d_conv(concat, self.get_dnf(0), (3, 3), 'SAME', act)
                x_b1 = self._d_conv(x_b1, self.get_dnf(0), (4, 4), 'VALID', act)
                output_b1 = self._fc(x_b1.reshape(x_b1.shape[0], -1), units=1)      # dense on the [B,1,1,C] map
            return output_b1.reshape(-1)

    def _up(self, x):
        """x2: the reference's nearest-neighbour upscale, or with resample_filter the low-pass filtered upsample_2d."""
        return upscale(x, 2) if self.resample_filter is None else upsample_2d(x, self.resample_filter)

    def _down(self, x):
        """/2: the reference's 2x2 average pool, or with resample_filter the low-pass filtered downsample_2d."""
        return pool(x, 2) if self.resample_filter is None else downsample_2d(x, self.resample_filter)

    def _d_conv(self, x, f, ks, padding, act):
        """A 3x3 / 4x4 convolution of the critic.  critic_norm = None: conv + lrelu (the reference).  'layer' / 'pixel': the conv
        without activation, then the per-sample normalisation with the lrelu fused — the normalised critic of the WGAN-GP and PGGAN
        papers (batch norm would couple the samples under the per-sample penalty); both are differentiable twice."""
        if self.critic_norm is None:
            return self._conv2d(x, f=f, ks=ks, s=(1, 1), padding=padding, act=act)
        x = self._conv2d(x, f=f, ks=ks, s=(1, 1), padding=padding, act=None)
        return layer_norm(x, act=act) if self.critic_norm == 'layer' else pixel_norm(x, act=act)

    def generator(self, z_var, cond_inp, stages, t, reuse=False, cond_noise=True, truncation_psi=None):
        """-> (image NHWC, mean, log_sigma)  (pggan.py:283-316).  With style_dim (Karras et al. 2019) the dense
        4x4 trunk from [z, c] stays (no learned constant), the mapping network comes between it and the first convolution, and every
        conv -> layer_norm(relu) pair is a conv -> style block (_g_conv); to_rgb, the fade-in and _up are the reference's either way.
        truncation_psi (style_dim only; None: the constructor's) replaces w by w_avg + psi (w - w_avg); training never truncates
        (g_losses and d_losses pass None with the constructor's None)."""
        alpha_trans = self._alpha_dev
        stage0 = self.get_conv_scope_name(0)
        with S.variable_scope('g_net', reuse=reuse):
            with S.variable_scope(stage0, reuse=reuse):
                mean_lr, log_sigma_lr = self.generate_conditionals(cond_inp)
                cond = self.sample_normal_conditional(mean_lr, log_sigma_lr, cond_noise)
                zc = torch.cat([z_var, cond], 1)
                x = self._fc(zc, units=4 * 4 * self.get_nf(0))
                x = layer_norm(x)
                x = x.reshape(-1, 4, 4, self.get_nf(0))
                if self.style_dim is None:
                    x = self._g_conv(self._g_conv(x, self.get_nf(0)), self.get_nf(0))
            if self.style_dim is not None:
                self._mapping(zc, reuse, self.truncation_psi if truncation_psi is None else float(truncation_psi))
                with S.variable_scope(stage0, reuse=reuse):                # (re-entered: only Conv and StyleMod layers follow)
                    x = self._g_conv(self._g_conv(x, self.get_nf(0)), self.get_nf(0))
            x_iden = None
            for i in range(1, stages):
                if (i == stages - 1) and t:
                    x_iden = self.to_rgb(x, stages - 2)
                    x_iden = self._up(x_iden)
                with S.variable_scope(self.get_conv_scope_name(i), reuse=reuse):
                    x = self._up(x)
                    x = self._g_conv(self._g_conv(x, self.get_nf(i)), self.get_nf(i))
            x = self.to_rgb(x, stages - 1)
            if t:
                x = lerp(x_iden, x, alpha_trans)                  # (1 - alpha) * x_iden + alpha * x
            return x, mean_lr, log_sigma_lr

    def _mapping(self, zc, reuse, psi):
        """style_dim: the mapping network (scope g_net/mapping: pixel norm of [z, c], then mapping_layers dense + lrelu layers) -> self._w
        [B,D], and self._w_used, what the style blocks of this pass see: w, or with psi its truncation.  g_net/mapping/w_avg [D] (not
        trainable) follows the batch mean of w with decay 0.995 in g_losses; under data parallelism it is rank-local — every rank averages
        its own batches — and rank 0's is the one a checkpoint holds."""
        B = zc.shape[0]
        with S.variable_scope('mapping', reuse=reuse):
            w = pixel_norm(zc.reshape(B, 1, 1, zc.shape[1])).reshape(B, zc.shape[1])
            for _ in range(self.mapping_layers):
                w = self._fc(w, units=self.style_dim, act=lrelu_act())
            w_avg = self.store.get_variable('w_avg', (self.style_dim,), S.constant_init(0.0), trainable=False)
        self._w = w
        self._w_used = w if psi is None else torch.lerp(w_avg.expand_as(w), w, psi)       # psi = 1: w, psi = 0: w_avg, both exactly
        self._block = 0                                                   # the style blocks of the pass, counted by _g_conv

    def _g_conv(self, x, f):
        """A 3x3 convolution of the generator and what follows it: the reference's layer_norm(relu), or with style_dim style block k of
        the pass: per-pixel noise scaled per channel, relu, instance norm, the style's affine map.  With modulated_conv the pair is one
        weight-demodulated convolution: the style scales the input channels, then bias, the same noise and relu."""
        if self.modulated_conv:
            k, self._block = self._block, self._block + 1
            noise = self._style_noise_image(k, x)
            return modulated_conv2d(x, self._w_used, f, ks=(3, 3), noise=noise, act=relu, init=self._init(3 * 3 * x.shape[-1]),
                                    style_init=self._init(self.style_dim), **({'second_order': True} if self._second_order else {}))
        x = self._conv2d(x, f=f, ks=(3, 3), s=(1, 1))
        if self.style_dim is None:
            return layer_norm(x, act=relu)
        k, self._block = self._block, self._block + 1
        return style_block(x, self._w_used, noise=self._style_noise_image(k, x), act=relu, init=self._init(self.style_dim))

    def _style_noise_image(self, k, x):
        """The noise image [B,H,W] of style block k: the feed's `style_noise_{d,g}_<k>`, the k-th of the sampler's list, or a fresh draw."""
        if not self.style_noise:
            return None
        src = self._sn
        n = None
        if isinstance(src, tuple):
            n = src[0].get('style_noise_%s_%d' % (src[1], k))
        elif src is not None:
            if k >= len(src):
                raise ValueError('the sampler was given %d noise images, style block %d needs one more' % (len(src), k))
            n = src[k]
        if n is None:
            n = K.trunc_normal_(torch.empty(x.shape[:3], device=x.device), a=-STYLE_NOISE_CUT, b=STYLE_NOISE_CUT)
        if tuple(n.shape) != tuple(x.shape[:3]):
            raise ValueError('the noise image of style block %d must be %s, got %s' % (k, tuple(x.shape[:3]), tuple(n.shape)))
        return n

    @staticmethod
    def mbstd_features(channels):
        """Statistic channels of the minibatch standard deviation: 4 where the 4x4 map has a multiple of 16 channels (the next
        convolution's input channels stay a multiple of four: the 16-byte conv kernels), else 1."""
        return 4 if channels % 16 == 0 else 1

    def concat_cond4(self, x, cond):
        return concat_tile(x, cond)

    def get_rgb_name(self, stage):
        return 'rgb_stage_%d' % stage

    def get_conv_scope_name(self, stage):
        return 'conv_stage_%d' % stage

    def get_dnf(self, stage):
        return min(self.fmap_base // (2 ** stage) * 2, self.fmap_max)

    def get_nf(self, stage):
        return min(self.fmap_base // (2 ** stage) * 4, self.fmap_max)

    def from_rgb(self, x, stage):
        with S.variable_scope(self.get_rgb_name(stage), reuse=S.default_store().reuse()):
            return self._conv2d(x, f=self.get_dnf(stage), ks=(1, 1), s=(1, 1), act=lrelu_act())

    def to_rgb(self, x, stage):
        with S.variable_scope(self.get_rgb_name(stage), reuse=S.default_store().reuse()):
            x = self._conv2d(x, f=9, ks=(2, 2), s=(1, 1), act=relu)
            return self._conv2d(x, f=3, ks=(1, 1), s=(1, 1))

    def generate_conditionals(self, embeddings, units=None):
        units = units or self.compr_embed_dim
        with K.f32_outputs():          # conditioning statistics stay fp32 in every storage mode
            return self._fc(embeddings, units, act=lrelu_act()), self._fc(embeddings, units, act=lrelu_act())

    def sample_normal_conditional(self, mean, log_sigma, cond_noise=True):
        if not cond_noise:
            return mean
        eps = getattr(self, '_ca', None)
        if eps is None or eps.shape != mean.shape:
            eps = K.trunc_normal_(torch.empty_like(mean))
        return mean + torch.exp(log_sigma) * eps

    def kl_std_normal_loss(self, mean, log_sigma):
        return torch.mean(-log_sigma + 0.5 * (-1.0 + torch.exp(2.0 * log_sigma) + mean * mean))

    def get_variables_up_to_stage(self, stages):
        """Names of the variables a stage's checkpoint holds (pggan.py:380-386): the stage's rgb layers + every conv stage
        below it, critic then generator."""
        d = list(self.store.global_variables('d_net/%s/' % self.get_rgb_name(stages - 1)))
        g = list(self.store.global_variables('g_net/%s/' % self.get_rgb_name(stages - 1)))
        for stage in range(stages):
            d += list(self.store.global_variables('d_net/%s/' % self.get_conv_scope_name(stage)))
            g += list(self.store.global_variables('g_net/%s/' % self.get_conv_scope_name(stage)))
        g += list(self.store.global_variables('g_net/mapping/'))       # (style_dim: the mapping network and w_avg, at every stage; else none)
        return d + g

    # ---- training loop (pggan.py:147-247) ---------------------------------------------------------------------------------
    def make_feed(self, gen):
        images, wrong_images, embed, _, _ = self.dataset.train.next_batch(self.batch_size, 4, wrong_img=True, embeddings=True)
        return {'x': images, 'x_mismatch': wrong_images, 'cond': embed,
                'z': torch.randn((self.batch_size, self.z_dim), generator=gen, device=self.device)}

    def define_summaries(self):
        """reference pggan.py:132-156,165: the FileWriter on log_dir (utils/summary.py: TensorBoard event files without TensorFlow)."""
        from ...utils.summary import FileWriter
        self.writer = FileWriter(self.log_dir)

    def write_summaries(self, idx, feed, out, sample_z=None):
        """The merged summary of reference pggan.py:132-156 at step idx (written every 20 steps, pggan.py:220-222): images `x` and
        `G_img`, histograms `z` / `z_sample`, and the twelve scalars under the reference's tags.  The reference evaluates them in a
        third sess.run after the two updates; here they are the values the iteration itself computed, as in models/wgancls."""
        from ...utils import summary as S
        d, g = out['d'], out['g']
        np_ = lambda t: t.detach().float().cpu().numpy()
        vals = [S.image('x', np_(feed['x'])), S.image('G_img', np_(g['G'])), S.histogram('z', np_(feed['z']))]
        if sample_z is not None:
            vals.append(S.histogram('z_sample', np_(sample_z)))
        vals += [S.scalar('G_loss_wass', -float(g['D_loss_fake'])), S.scalar('kl_loss', float(g['G_kl_loss'])), S.scalar('G_loss', float(g['G_loss']))]
        for tag, key in (('D_loss_real', 'D_loss_real'), ('D_loss_fake', 'D_loss_fake'), ('real_gp', 'real_gp'), ('D_loss', 'D_loss'),
                         ('reg_loss', 'reg_loss'), ('wdist', 'wdist'), ('wdist2', 'wdist2'), ('d_loss_mismatch', 'D_loss_mismatch'),
                         ('real_gp2', 'real_gp2')):
            vals.append(S.scalar(tag, float(d[key])))
        if 'pl_penalty' in g:                     # a due step of the path-length regulariser
            vals += [S.scalar('pl_penalty', float(g['pl_penalty'])), S.scalar('pl_length', float(g['pl_length'])), S.scalar('pl_mean', float(g['pl_mean']))]
        if self.aug_sampler is not None:          # the augmentation's probability after this step, and the controller's last statistic
            vals += [S.scalar('aug_p', float(d['aug_p'])), S.scalar('aug_r', self.aug_sampler.last_r)]
        self.writer.add_summary(vals, idx)
        self.writer.flush()

    def _savers(self):
        """(the saver of this stage's checkpoints, the saver that restores: the previous stage's variables for a transition, else the
        same one).  Each option's entries travel with every checkpoint and only with the option: without it the files are what they were."""
        shadows = [self.G_optimizer] if self.g_ema is not None else None      # both savers: a transition restores the previous stage's shadows too
        extra, loaded = {}, {}
        self._loaded = loaded                     # key -> what a restore read of it, for _after_restore
        if self.aug_sampler is not None:          # the sampler's sixteen state words; a checkpoint written without them leaves the sampler as it is
            extra['diffaug/state'] = (self.aug_sampler.state_dict, lambda w: (loaded.__setitem__('diffaug/state', w), self.aug_sampler.load_state_dict(w)))
        sn = self.critic_spectral
        for key in () if sn is None else [k for n in sn.names for k in sn.keys(n)]:
            # the raw weights, u, v and sigma of every normalised kernel; the variable itself is saved as the normalised weights every reader expects
            extra[key] = ((lambda key=key: sn.state_tensor(key).numpy()), (lambda a, key=key: loaded.__setitem__(key, a)))
        if self.pl_weight is not None:            # the mean path length, under a name outside g_net/ and d_net/: no reader's name checks see it
            extra[PL_MEAN_KEY] = ((lambda: self.pl_mean.detach().cpu().numpy()),
                                  lambda a: (loaded.__setitem__(PL_MEAN_KEY, a), self.pl_mean.copy_(torch.as_tensor(a, dtype=torch.float32).reshape(()))))
        if self.resample_filter is not None:
            # the normalised taps, so that a reader built with other taps, or none, can refuse the generator instead of sampling another
            # function from its weights (what a restore found is read from the file: _after_restore)
            extra[RESAMPLE_KEY] = ((lambda: self.resample_taps), lambda a: None)
        saver = Saver(self.store, var_list=self.get_variables_up_to_stage(self.stage), max_to_keep=2, shadows=shadows, extra=extra)
        if not self.trans:
            return saver, saver
        return saver, Saver(self.store, var_list=self.get_variables_up_to_stage(self.stage - 1), shadows=shadows, extra=extra)

    def _after_restore(self, src, log):
        """What a restore through `src` leaves to do: the taps the checkpoint was trained with, the spectral state, the sampler's words."""
        self.resample_restored = checkpoint_architecture(self.check_dir_read)[1]
        if not same_taps(self.resample_restored, self.resample_taps):
            # the trainer goes on (a stage may be grown with another filter on purpose); the readers refuse (eval_pggan.restore_generator)
            log('resample filter: the checkpoint in %s was trained with %s, this model resamples with %s' % (
                self.check_dir_read, describe_taps(self.resample_restored), describe_taps(self.resample_taps)))
        sn = self.critic_spectral
        if sn is not None:
            # a kernel that was restored and whose four keys the file holds is restored verbatim; every other one starts from the
            # weights it has now (a checkpoint trained without the flag, a variable new at this stage)
            whole = [n for n in sn.names if src._is_selected(n) and all(k in self._loaded for k in sn.keys(n))]
            sn.load_state_dict({k: self._loaded[k] for n in whole for k in sn.keys(n)})
            synced = [n for n in sn.names if n not in set(whole)]
            sn.sync(synced)
            self.spectral_synced = len(synced)
            log('spectral normalisation: %d of %d kernels restored with their state, %d synced from their weights' % (
                len(whole), len(sn.names), len(synced)))
        if self.pl_weight is not None:
            if PL_MEAN_KEY not in self._loaded:
                self.pl_mean.zero_()
                log('the checkpoint in %s carries no mean path length (it was trained without pl_weight): pl_mean starts at 0' % self.check_dir_read)
            else:
                log('path-length regularisation: pl_mean %.6f restored' % float(self.pl_mean))
        if self.aug_sampler is not None and 'diffaug/state' not in self._loaded:
            log('the checkpoint in %s carries no augmentation state: p stays %.6f, call counter %d' % (
                self.check_dir_read, self.aug_sampler.p, self.aug_sampler.counter))

    def train(self, max_steps=None, log=None, side_effects=False, summaries=False, final_sample=False):
        """Stage schedule semantics of pggan.py:147-247: a transition stage restores the previous stage's variables
        (`get_variables_up_to_stage(stage - 1)`) from check_dir_read, a stabilisation stage its own; new variables keep
        their fresh initialisation; checkpoints of `get_variables_up_to_stage(stage)` go to check_dir_write.  What was
        restored is kept in `self.restored` = (directory, step, variable names), None when nothing was.  final_sample: the
        last iteration, which writes the last checkpoint, also writes a sample grid (the reference only samples every 2000)."""
        from ...utils.utils import get_balanced_factorization, save_captions, save_images
        log = log or (lambda s: (sys.stdout.write(s + '\n'), sys.stdout.flush()))
        saver, src = self._savers()
        if side_effects and self.stage != 1:
            could_load, step = load(src, None, self.check_dir_read)
            if not could_load:
                raise RuntimeError('Could not load previous stage during transition' if self.trans else 'Could not load current stage')
            self.restored = (self.check_dir_read, step, list(src.var_list))
            self._after_restore(src, log)
        gen = torch.Generator(device=self.device).manual_seed(1234)
        if side_effects:
            sample_z = torch.randn((self.sample_num, self.z_dim), generator=gen, device=self.device)
            _, sample_cond, _, captions = self.dataset.test.next_batch_test(self.sample_num, 0, 1)
            sample_cond = sample_cond[0]
            save_captions(self.sample_path, captions)
        end = min(self.steps, max_steps) if max_steps is not None else self.steps
        t0 = time.time()
        out = None
        if summaries and self.log_dir:
            self.define_summaries()
        for idx in range(1, end):
            feed = self.make_feed(gen)
            out = self.iteration(idx, feed)
            if idx % 20 == 0 and getattr(self, 'writer', None) is not None:
                self.write_summaries(idx, feed, out, sample_z if side_effects else None)
            if idx % 20 == 0:
                epoch = idx // max(self.dataset.train.num_examples // self.batch_size, 1)
                log('Epoch: [%2d] [%4d] time: %4.4f, d_loss: %.8f, g_loss: %.8f' % (
                    epoch, idx, time.time() - t0, float(out['d']['D_loss']), float(out['g']['G_loss'])))
            if side_effects and (idx % 2000 == 0 or (final_sample and idx == end - 1)):
                samples = torch.clamp(self.sampler(sample_z, sample_cond), -1.0, 1.0)
                save_images(samples, get_balanced_factorization(samples.shape[0]), '{}train_{:02d}_{:04d}.png'.format(self.sample_path, 0, idx))
                if self.g_ema is not None:            # the same z and captions from the averaged generator
                    with self.ema_weights():
                        samples = torch.clamp(self.sampler(sample_z, sample_cond), -1.0, 1.0)
                    save_images(samples, get_balanced_factorization(samples.shape[0]), '{}train_ema_{:02d}_{:04d}.png'.format(self.sample_path, 0, idx))
            if side_effects and (idx % 2000 == 0 or idx == end - 1):      # end - 1 == steps - 1 unless max_steps truncates
                save(saver, None, self.check_dir_write, idx)
        return out
