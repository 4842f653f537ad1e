"""Full-size parity of the "next" rows against the float64 oracles, mask-pinned like
tests/test_step_b64_gpu.py: StackGAN Stage-II at its real 256x256 resolution and full width (GF=128, DF=64, critic up to
2048 channels), and a PGGAN transition stage at 64x64 (stage 5: the first stage with 256-channel layers next to the 512 ones).
Tolerances: PGGAN — SURVEY 8(c)'s (loss scalars 1e-5 relative, gradients max|d|/max|ref| <= 1e-4 per tensor).  Stage-II —
~60 conv + batch-norm layers in series at batch 2, statistics over as few as 32 values: loss scalars 1e-4, the tanh image
2e-4 absolute, gradients 2e-4 per tensor (measured: <= 5.8e-5 / 7e-5 / 1.1e-4; the loss on the generated image moves between
4.3e-5 and 5.8e-5 with nothing but the SUMMATION ORDER of the 128 -> 3 transposed conv — one, four or two passes over its
channels, t2i_tuning_set("thin_parts") — while the image error itself stays at 6.4-6.9e-5: rounding noise through batch
norms over two samples, so the scalar bound is the image's order of magnitude, not tighter; before the batch-norm statistics were made
stable — sum x^2 - (sum x)^2/n replaced by shifted chunk moments + Chan merging, DESIGN 4.6 — the same quantities sat at
8e-5 / 9e-4 / 7e-4 and the committed test allowed 8e-2).  Yardstick (round 3, /tmp run of the oracle in float32 on the
same step, un-pinned): torch-CPU float32 sits 1.0e-4 from float64 on the image and 4.4e-5 on D_synthetic_loss — the HIP path's
6.9e-5 / 5.8e-5 are the float32 floor of this model at batch 2, not a kernel property, which is why these bounds are not SURVEY
8(c)'s 1e-5 (PGGAN at the same 256x256 resolution, no batch norm over two samples, meets 1e-5: 6.2e-6 below).  Where a tensor's exact gradient is zero (biases in front of a
batch norm) the bound is absolute.  Batch sizes are the smallest that keep the
float64 oracle at ~30 s (2 and 4); the tiny-width golden steps (tests/test_stackgan.py, tests/test_pggan.py) stay as the
committed-fixture checks.

Round 3 adds the remaining full-width cases of the hot path's own variants and of the next rows: gancls at the reference's own
dimensions (models/gancls/cfg/flowers.yml: GF 128, DF 64, z 100; B = 64, the metric's batch, and B = 8, the yml's), StackGAN
Stage-I at full width (B = 16), and PGGAN stages 6 (128x128) and 7 in transition (256x256) at B = 2.  All at SURVEY 8(c)'s
tolerances (loss scalars 1e-5, gradients 1e-4 per tensor) unless a looser bound is stated next to the case with its reason."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from branches import flips, record_branches, split_sections

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(got, ref, scale=None):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    s = float(np.abs(ref).max()) if scale is None else scale
    return float(np.abs(got - ref).max() / max(s, 1e-30))


class Checker(object):
    def __init__(self):
        self.bad = []

    def __call__(self, name, err, tol):
        print('  %-44s %.2e  (tol %.0e)%s' % (name, err, tol, '' if err <= tol else '   <-- FAIL'))
        if not err <= tol:
            self.bad.append((name, err, tol))

    def grads(self, arena, names, ref, tol=1e-4, scales=None, may_cancel=()):
        """scales: per tensor, the magnitude of its gradient before the loss terms cancel (oracle d_step(term_scales=True)).  A
        tensor whose scale exceeds 4 max|ref| is a small difference of large terms and is bounded against the scale instead; such
        tensors must be named in `may_cancel` (the list cannot grow silently) and are printed."""
        self.cancelling = []
        for n in names:
            r = ref[n]
            rmax = float(r.abs().max())
            if rmax < 1e-9:
                self('grad ' + n + ' (exact zero: abs)', float(arena.grad_of(n).abs().max()), 1e-4)
            elif scales is not None and scales[n] > 4.0 * rmax:
                self.cancelling.append(n)
                print('  %-44s max|ref| %.3e is %.1e of its un-cancelled scale %.3e' % (n, rmax, rmax / scales[n], scales[n]))
                self('grad ' + n + ' (vs un-cancelled scale)', relerr(arena.grad_of(n), r, scale=scales[n]), tol)
                if n not in may_cancel:
                    self.bad.append((n, 'takes the un-cancelled-scale bound but is not in the pinned list', may_cancel))
            else:
                self('grad ' + n, relerr(arena.grad_of(n), r), tol)


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 64)))
    return torch.device('cuda')


def _rel_l2(got, ref):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().double().cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


# Stage-II in reduced precision (round 6): what bench.py's `next_rows[stackgan_stage2, bf16]` row runs is kernels.FWD_F32_BWD_BF16 on all three
# networks — every forward GEMM in fp32 math, every input- / filter-gradient GEMM in bf16 math — and that arithmetic is held to BASELINE.md's 2e-2
# on every loss and every gradient tensor below.  (The all-bf16 arithmetic the row ran before sits far outside it on this model — ~60 conv +
# batch-norm layers in series with statistics over two samples amplify the 2^-8 operand rounding: 2.3e-2 of the branches differ from the
# float64 oracle's own, the 256x256 image is 1.46e-1 off, critic gradients median 2.4e-1, generator gradients median 4.2e-1,
# profiles/r06_bf16_side_row_parity.txt — and CONFIG3_NET_MATH on the generators alone leaves the generator-step gradients at a median of 2.0e-2.)
STAGE2_COMPLIANT = dict(loss=2e-2, image=2e-2, d_grad=2e-2, g_grad=2e-2, flips=1e-4)       # kernels.FWD_F32_BWD_BF16 on all three networks


def _stage2_full_size(gpu, bf16):
    from oracle import torch_stackgan as SG, torch_step as T
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan as StageI
    from t2i_amd.models.stackgan.stageII.model import ConditionalGan as StageII
    from t2i_amd.models.stackgan.stageII.trainer import ConditionalGanTrainer
    from t2i_amd.utils.config import config_from_yaml
    B = 2
    base = os.path.join(ROOT, 'text-to-image_amd', 'models', 'stackgan')
    c1 = config_from_yaml(os.path.join(base, 'stageI', 'cfg', 'flowers.yml')); c1.TRAIN.BATCH_SIZE = B
    c2 = config_from_yaml(os.path.join(base, 'stageII', 'cfg', 'flowers.yml')); c2.TRAIN.BATCH_SIZE = B
    o1, o2 = SG.Cfg(batch=B), SG.Cfg(out_size=256, real_label=0.95, batch=B)
    P = OrderedDict((n, v.float().double()) for n, v in SG.init_variables(o2, 2, o1, seed=0).items())      # fp32-representable
    feed = {k: v.float().double() for k, v in SG.synthetic_feed(o2, 2, o1, seed=1).items()}
    compliant = bf16 == 'compliant'
    s1 = StageI(c1, build_model=False, device=gpu)
    m = StageII(s1, c2, build_model=False)
    if compliant:       # every forward GEMM of the three networks in fp32 math, every backward GEMM in bf16 math (kernels.FWD_F32_BWD_BF16)
        from t2i_amd import kernels as K
        s1.net_math = {'g_net': K.FWD_F32_BWD_BF16, 'd_net': K.FWD_F32_BWD_BF16}
        m.net_math = {'g_net': K.FWD_F32_BWD_BF16, 'd_net': K.FWD_F32_BWD_BF16}
    m.build_model()
    m.store.load({n: v.numpy() for n, v in P.items()})
    assert m.output_size == 256 and [n for n in m.store.vars] == list(P)
    f = {k: v.float().to(gpu) for k, v in feed.items()}
    hf = {'inputs': f['x'], 'wrong_inputs': f['x_mismatch'], 'phi_inputs': f['cond'], 'z': f['z']}
    hf.update({k: v for k, v in f.items() if k.startswith('ca_noise')})
    moving0 = {n: v.detach().clone() for n, v in m.store.vars.items() if 'moving' in n}
    tr = ConditionalGanTrainer(None, m, None, c2)
    # the critic passes of one sess.run stacked along the batch axis (see _cgan_steps); the generator step stacks its three critic
    # evaluations too (fake with the gradient | match | mismatch)
    plan = [('G',), ('Dfake', 'Dmatch', 'Dmis')]
    chk = Checker()
    env = STAGE2_COMPLIANT
    flip_tol = env['flips'] if bf16 else 1e-4

    def grads(arena, names, ref, tol, l1=None):
        if not bf16:
            return chk.grads(arena, names, ref, tol)
        worst, unc = [], []
        for n in names:                         # relative L2 per tensor (the yardstick of the config-3 test)
            got, r = arena.grad_of(n).detach().double().cpu().reshape(-1), ref[n].reshape(-1)
            s1_ = float(l1[n].norm()) if (l1 is not None and n in l1) else 0.0
            if s1_ > 4.0 * float(r.norm()):
                # a bias whose gradient is a small difference of large terms (zero in front of a batch norm, a border effect behind a zero-padded
                # convolution): the rounding error of sum g scales with sum |g| (oracle/torch_stackgan._BIAS_L1) — that is the yardstick, and the
                # exactly-zero ones are held to it too instead of being skipped
                unc.append((float((got - r).norm()) / s1_, n))
            elif float(r.abs().max()) >= 1e-9:
                worst.append((_rel_l2(arena.grad_of(n), ref[n]), n))
        worst.sort()
        print('  bf16 gradients, relative L2: median %.3e, worst %.3e (%s), then %s' % (
            worst[len(worst) // 2][0], worst[-1][0], worst[-1][1], ', '.join('%.2e %s' % w for w in worst[-4:-1][::-1])))
        chk('worst gradient (relative L2)', worst[-1][0], tol)
        if unc:
            unc.sort()
            print('  %d cancelling bias gradients against sum |g|: worst %.3e (%s)' % (len(unc), unc[-1][0], unc[-1][1]))
            chk('worst cancelling bias gradient (vs sum |g|)', unc[-1][0], tol)
    # ---- critic step
    rec = []
    with record_branches(rec):
        d = tr.d_losses(hf)
        torch.cuda.synchronize()
    own = T.SectionTape()
    with T.use_tape(own), T.forward_only():        # the oracle's own branches: forward passes only
        SG.d_step(P, o2, feed, 2, o1)
    masks = split_sections(rec, own.record, plan)
    fl, units = flips(own.record, masks)
    print('Stage-II critic step: %d of %d branches differ (%.2e)' % (fl, units, fl / units))
    assert fl <= flip_tol * units
    with T.use_tape(T.SectionTape(masks)):
        ref = SG.d_step(P, o2, feed, 2, o1, bias_l1=compliant)
    for k in ('D_loss', 'D_real_match_loss', 'D_real_mismatch_loss', 'D_synthetic_loss'):
        chk(k, abs(float(d[k]) - ref[k]) / max(abs(ref[k]), 1.0), env['loss'] if bf16 else 1e-4)
    if bf16:
        assert compliant and _rel_l2(d['G'], ref['G']) < 1e-4, 'the forward passes are meant to be fp32 here'
        chk('G (256x256 image, relative L2)', _rel_l2(d['G'], ref['G']), env['image'])
    else:
        chk('G (256x256 image, tanh output)', relerr(d['G'], ref['G'], scale=1.0), 2e-4)
    grads(m.d_arena, m.d_vars, ref['grads'], env['d_grad'] if bf16 else 2e-4, ref.get('bias_l1'))
    if compliant:
        worst = max(_rel_l2(m.d_arena.grad_of(n), ref['grads'][n]) for n in m.d_vars if n.endswith('weights'))
        assert worst > 1e-4, 'reduced precision is not in use in the backward GEMMs'

    with torch.no_grad():                      # undo the moving-average side effect of the probe pass
        for n, v in moving0.items():
            m.store.vars[n].copy_(v)
    # ---- generator step
    rec = []
    with record_branches(rec):
        g = tr.g_losses(hf)
        torch.cuda.synchronize()
    own = T.SectionTape()
    with T.use_tape(own), T.forward_only():        # the oracle's own branches: forward passes only
        SG.g_step(P, o2, feed, 2, o1)
    masks = split_sections(rec, own.record, plan)
    fl, units = flips(own.record, masks)
    print('Stage-II generator step: %d of %d branches differ (%.2e)' % (fl, units, fl / units))
    assert fl <= flip_tol * units
    with T.use_tape(T.SectionTape(masks)):
        gref = SG.g_step(P, o2, feed, 2, o1, bias_l1=compliant)
    for k in ('G_loss', 'G_gan_loss', 'G_kl_loss'):
        chk(k, abs(float(g[k]) - gref[k]) / max(abs(gref[k]), 1.0), env['loss'] if bf16 else 1e-4)
    grads(m.g_arena, m.g_vars, gref['grads'], env['g_grad'] if bf16 else 2e-4, gref.get('bias_l1'))
    assert not chk.bad, chk.bad


def test_stackgan_stage2_full_size(gpu):
    _stage2_full_size(gpu, bf16=False)


# The default sweep keeps every stage's shapes once (stages 1-4 in both forms where cheap, 6 stable, 7 in transition); the two middle cases
# (3 in transition, 4 stable, 5 in transition: 37 s of float64 CPU oracle between them, shapes the neighbours cover) run under T2I_FULL_SWEEP=1 — the GPU
# suite's wall clock is dominated by the CPU oracle (VERDICT r5 "next" 8).
_PGGAN_CASES = [(1, False, 16), (2, True, 16), (2, False, 16), (3, False, 8), (4, True, 8), (6, False, 2), (7, True, 2)]
if os.environ.get('T2I_FULL_SWEEP') == '1':
    _PGGAN_CASES += [(3, True, 16), (4, False, 8), (5, True, 4)]


@pytest.mark.parametrize('stage,trans,B', _PGGAN_CASES)
def test_pggan_stage_full_width(gpu, stage, trans, B):
    """reference models/pggan/pggan.py:251-316 (generator / critic of a stage), train_pggan.py:17-69 (the stage schedule: 1 = 4x4,
    2t / 2 = 8x8, 3t / 3 = 16x16, 4t / 4 = 32x32 — round 4: the low stages at full width and at the reference's batch 16 where the
    float64 oracle allows — 5t = 64x64 in transition, 6 = 128x128 stabilisation, 7t = 256x256 in transition; batch 16 -> 8 from
    stage 6 on, from stage 3 here the smallest batches that keep the float64 oracle below a minute)."""
    from oracle import torch_pggan as PG, torch_step as T
    from t2i_amd.models.pggan.pggan import PGGAN
    alpha = 0.3
    cfg = PG.Cfg(batch=B)
    P = OrderedDict((n, v.float().double()) for n, v in PG.init_variables(cfg, stage, trans, seed=0).items())
    feed = {k: v.float().double() for k, v in PG.synthetic_feed(cfg, stage, seed=1).items()}
    m = PGGAN(B, 100, None, None, None, None, None, stage, trans, device=gpu)
    m.store.load({n: v.numpy() for n, v in P.items()})
    m.set_alpha(alpha)
    f = {k: v.float().to(gpu) for k, v in feed.items()}
    hf = {'x': f['x'], 'x_mismatch': f['x_mismatch'], 'cond': f['cond'], 'z': f['z'], 'eps_graph': f['eps'].reshape(-1),
          'ca_noise_d': f['ca_noise_d'], 'ca_noise_g': f['ca_noise_g']}
    chk = Checker()
    rec = []
    with record_branches(rec):
        d = m.d_losses(hf)
        torch.cuda.synchronize()
    own = T.SectionTape()
    with T.use_tape(own), T.forward_only():        # the oracle's own branches: forward passes only
        PG.d_step(P, cfg, feed, stage, trans, alpha)
    masks = split_sections(rec, own.record, [('G',), ('Dg', 'Dx', 'Dxmi'), ('Dxh',)])
    fl, units = flips(own.record, masks)
    print('PGGAN stage %d%s critic step: %d of %d branches differ (%.2e)' % (stage, 't' if trans else '', fl, units, fl / units))
    assert fl <= 1e-4 * units
    with T.use_tape(T.SectionTape(masks)):
        ref = PG.d_step(P, cfg, feed, stage, trans, alpha)
    for k in ('D_loss', 'wdist', 'wdist2', 'real_gp', 'real_gp2'):
        chk(k, abs(float(d[k]) - ref[k]) / max(abs(ref[k]), 1.0), 1e-5)
    chk('G (%dx%d image)' % (m.output_size, m.output_size), relerr(d['G'], ref['G']), 1e-5)
    chk('D(x_hat)', relerr(d['Dx_hat_logit'], ref['Dx_hat']), 1e-5)
    chk.grads(m.d_arena, m.d_vars, ref['grads'])
    rec = []
    with record_branches(rec):
        g = m.g_losses(hf)
        torch.cuda.synchronize()
    own = T.SectionTape()
    with T.use_tape(own), T.forward_only():        # the oracle's own branches: forward passes only
        PG.g_step(P, cfg, feed, stage, trans, alpha)
    masks = split_sections(rec, own.record, [('G',), ('Dg',)])
    fl, units = flips(own.record, masks)
    print('PGGAN stage %d%s generator step: %d of %d branches differ (%.2e)' % (stage, 't' if trans else '', fl, units, fl / units))
    assert fl <= 1e-4 * units
    with T.use_tape(T.SectionTape(masks)):
        gref = PG.g_step(P, cfg, feed, stage, trans, alpha)
    for k in ('G_loss', 'G_kl_loss'):
        chk(k, abs(float(g[k]) - gref[k]) / max(abs(gref[k]), 1.0), 1e-5)
    chk.grads(m.g_arena, m.g_vars, gref['grads'])
    assert not chk.bad, chk.bad


def _cgan_steps(tag, tr, m, hf, d_oracle, g_oracle, loss_keys_d, loss_keys_g, chk, T, loss_tol=1e-5, grad_tol=1e-4, img_tol=1e-5,
                may_cancel=()):
    """Critic step then generator step of a sigmoid-CE conditional GAN (gancls, StackGAN Stage-I) against its float64 oracle,
    mask-pinned; d_oracle / g_oracle: callables that run the oracle step under whatever tape is installed."""
    moving0 = {n: v.detach().clone() for n, v in m.store.vars.items() if 'moving' in n}
    # the HIP passes in launch order (tests/branches.split_sections): gancls stacks the critic passes of one sess.run along the batch axis
    # (fake | match | mismatch in the critic step; the generator step stacks its three critic evaluations too: fake with the gradient |
    # match | mismatch)
    plan = [('G',), ('Dfake', 'Dmatch', 'Dmis')]
    rec = []
    with record_branches(rec):
        d = tr.d_losses(hf)
        torch.cuda.synchronize()
    own = T.SectionTape()
    with T.use_tape(own), T.forward_only():        # the oracle's own branches: forward passes only
        d_oracle()
    masks = split_sections(rec, own.record, plan)
    fl, units = flips(own.record, masks)
    print('%s critic step: %d of %d branches differ (%.2e)' % (tag, fl, units, fl / units))
    assert fl <= 1e-4 * units
    with T.use_tape(T.SectionTape(masks)):
        ref = d_oracle()
    for k in loss_keys_d:
        chk(k, abs(float(d[k]) - ref[k]) / max(abs(ref[k]), 1.0), loss_tol)
    chk('G (tanh output)', relerr(d['G'], ref['G'], scale=1.0), img_tol)
    chk.grads(m.d_arena, m.d_vars, ref['grads'], grad_tol, scales=ref.get('scales'), may_cancel=may_cancel)
    print('%s: critic tensors bounded against their un-cancelled scale: %s' % (tag, chk.cancelling))
    with torch.no_grad():                      # undo the moving-average side effect of the probe pass
        for n, v in moving0.items():
            m.store.vars[n].copy_(v)
    rec = []
    with record_branches(rec):
        g = tr.g_losses(hf)
        torch.cuda.synchronize()
    own = T.SectionTape()
    with T.use_tape(own), T.forward_only():        # the oracle's own branches: forward passes only
        g_oracle()
    masks = split_sections(rec, own.record, plan)
    fl, units = flips(own.record, masks)
    print('%s generator step: %d of %d branches differ (%.2e)' % (tag, fl, units, fl / units))
    assert fl <= 1e-4 * units
    with T.use_tape(T.SectionTape(masks)):
        gref = g_oracle()
    for k in loss_keys_g:
        chk(k, abs(float(g[k]) - gref[k]) / max(abs(gref[k]), 1.0), loss_tol)
    chk.grads(m.g_arena, m.g_vars, gref['grads'], grad_tol)


@pytest.mark.parametrize('B', [64, 8])
def test_gancls_full_width(gpu, B):
    """gancls at the reference's own dimensions (models/gancls/cfg/flowers.yml:9-19: z 100, GF 128, DF 64; model.py:54-192,
    trainer.py:19-51) — the second variant north_star names.  B = 64 is the metric's batch, B = 8 the yml's."""
    from oracle import torch_gancls as GC, torch_step as T
    from t2i_amd.models.gancls.model import GanCls
    from t2i_amd.models.gancls.trainer import GanClsTrainer
    from t2i_amd.utils.config import config_from_yaml
    cfg = config_from_yaml(os.path.join(ROOT, 'text-to-image_amd', 'models', 'gancls', 'cfg', 'flowers.yml'))
    cfg.TRAIN.BATCH_SIZE = B
    ocfg = GC.Cfg(batch=B)
    P = OrderedDict((n, v.float().double()) for n, v in GC.init_variables(ocfg, seed=0, dtype=torch.float64).items())
    feed = {k: v.float().double() for k, v in GC.synthetic_feed(ocfg, seed=1, dtype=torch.float64).items()}
    m = GanCls(cfg, device=gpu)
    assert [n for n in m.store.vars] == list(P) and (m.gf_dim, m.df_dim, m.z_dim) == (128, 64, 100)
    m.store.load({n: v.numpy() for n, v in P.items()})
    f = {k: v.float().to(gpu) for k, v in feed.items()}
    hf = {'inputs': f['x'], 'wrong_inputs': f['x_mismatch'], 'phi_inputs': f['cond'], 'z': f['z']}
    tr = GanClsTrainer(None, m, None, cfg)
    chk = Checker()
    # the logit bias (d_net/conv2d_8/bias): sum_i coef_i mean(sigmoid(l_i) - y_i), which on the B = 8 batch cancels to 4e-5 from
    # terms of 0.1-0.4 (torch-CPU float32 is 8e-3 from float64 there): the one tensor that may take the scale-relative bound
    _cgan_steps('gancls B=%d' % B, tr, m, hf, lambda: GC.d_step(P, ocfg, feed, term_scales=True), lambda: GC.g_step(P, ocfg, feed),
                ('D_loss', 'D_real_match_loss', 'D_real_mismatch_loss', 'D_synthetic_loss'), ('G_loss',), chk, T,
                may_cancel=('d_net/conv2d_8/bias',))
    assert not chk.bad, chk.bad


def test_stackgan_stage1_full_width(gpu):
    """StackGAN Stage-I at full width (reference models/stackgan/stageI/model.py:76-171, trainer.py:19-53; GF 128, DF 64,
    conditioning augmentation + KL), B = 16."""
    from oracle import torch_stackgan as SG, torch_step as T
    from t2i_amd.models.stackgan.stageI.model import ConditionalGan as StageI
    from t2i_amd.models.stackgan.stageI.trainer import ConditionalGanTrainer
    from t2i_amd.utils.config import config_from_yaml
    B = 16
    c1 = config_from_yaml(os.path.join(ROOT, 'text-to-image_amd', 'models', 'stackgan', 'stageI', 'cfg', 'flowers.yml'))
    c1.TRAIN.BATCH_SIZE = B
    o1 = SG.Cfg(batch=B)
    P = OrderedDict((n, v.float().double()) for n, v in SG.init_variables(o1, 1, seed=0).items())
    feed = {k: v.float().double() for k, v in SG.synthetic_feed(o1, 1, seed=1).items()}
    m = StageI(c1, device=gpu)
    assert [n for n in m.store.vars] == list(P)
    m.store.load({n: v.numpy() for n, v in P.items()})
    f = {k: v.float().to(gpu) for k, v in feed.items()}
    hf = {'inputs': f['x'], 'wrong_inputs': f['x_mismatch'], 'phi_inputs': f['cond'], 'z': f['z']}
    hf.update({k: v for k, v in f.items() if k.startswith('ca_noise')})
    tr = ConditionalGanTrainer(None, m, None, c1)
    chk = Checker()
    logit_bias = [n for n in m.d_vars if n.endswith('biases') or n.endswith('bias')][-1]      # see test_gancls_full_width
    _cgan_steps('Stage-I B=%d' % B, tr, m, hf, lambda: SG.d_step(P, o1, feed, 1, term_scales=True), lambda: SG.g_step(P, o1, feed, 1),
                ('D_loss', 'D_real_match_loss', 'D_real_mismatch_loss', 'D_synthetic_loss'), ('G_loss', 'G_gan_loss', 'G_kl_loss'), chk, T,
                may_cancel=(logit_bias,))
    assert not chk.bad, chk.bad


def test_stackgan_stage2_fwd_f32_bwd_bf16_within_2e2(gpu):
    """Stage-II with every forward GEMM of its three networks in fp32 math and every input- / filter-gradient GEMM in bf16 math
    (kernels.FWD_F32_BWD_BF16: bf16 operand images, fp32 accumulate): the same full-width step, mask-pinned, every loss and every gradient
    tensor of both steps within BASELINE.md's 2e-2 (relative L2 per tensor; biases whose gradient is a small difference of large terms against
    sum |g|, the exactly-zero ones included).  The forward being fp32, the image is exact and the pinning touches the fp32 tests' handful of units."""
    from t2i_amd import kernels as K
    K.set_math('bf16')
    try:
        _stage2_full_size(gpu, bf16='compliant')
    finally:
        K.set_storage('f32')
        K.set_math('f32')
        K.filter_cache_reset()
