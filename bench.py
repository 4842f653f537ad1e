#!/usr/bin/env python
"""bench.py — images/sec of one full wgancls iteration (critic step + kt, then generator step; reference
models/wgancls/trainer.py:97-102) at 64x64, batch 64 per GPU, fp32, synthetic inputs, random-init weights.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 64] [--dump-outputs DIR] [--full] [--no-cpu-baseline]
                    [--instrument inline|after|off]

A plain run sets up, runs W warm-up iterations, times ONE region of exactly K iterations, optionally writes what the last timed
iteration computed (--dump-outputs) and prints the line.  --full adds everything else the benchmark measures or checks: more timed
regions (median reported), the per-launch roofline pass, the config3_bf16 block, the b8_per_gpu / next_rows side rows, the CPU
baselines and, with N > 1, the data-parallel preflight and the exchange statistics.
N > 1 is launched by the driver as `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`
(one rank per GPU over RCCL); the batch is per GPU (weak scaling) and gradients are all-reduced (dp.py).
Rank 0 prints ONE JSON line.  See DESIGN.md §6 for how `roofline` and `cpu_baseline` are obtained.
"""
import argparse
import json
import os
import sys
import time

# multi-process GPU work on this stack needs dmabuf IPC (RCCL / cross-process tensors fail with the legacy mode); the boxes
# export it already — kept here so that a bare environment behaves the same
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# SURVEY.md §8(d) / BASELINE.md: algorithmic work per image (conv + dense MACs incl. padded taps, 2 FLOP/MAC)
G_FWD_MAC = 969478144
D_FWD_MAC = 694304768
NOMINAL_FLOP_PER_IMAGE = 2 * (4 * G_FWD_MAC + 17 * D_FWD_MAC)      # 31.362 GFLOP, the survey's nominal count
BF16_MATRIX_PEAK_TFLOPS = 2500.0                                   # dense bf16 MFMA peak (same guide)
FP32_MATRIX_PEAK_TFLOPS = 157.3                                    # MI355X_MICROARCH.md: 256 CU x 2.4 GHz x 256 FLOP/clk


def make_cfg(batch):
    from t2i_amd.utils.config import config_from_yaml
    cfg = config_from_yaml(os.path.join(ROOT, 'text-to-image_amd', 'models', 'wgancls', 'cfg', 'flowers.yml'))
    cfg.TRAIN.BATCH_SIZE = batch
    if os.environ.get('T2I_N_CRITIC'):          # diagnostics (tools/exchange_exactness.sh): critic-only iterations in between
        cfg.TRAIN.N_CRITIC = int(os.environ['T2I_N_CRITIC'])
    return cfg


def synthetic_feed(cfg, device, seed, with_noise=True):
    """BASELINE.md §2 inputs, generated on the device (resident in HBM before the timed region).
    with_noise=False: the feed carries no conditioning-augmentation noise, so the model draws it itself on every iteration —
    tf.truncated_normal is part of the reference's sess.run (models/wgancls/model.py:119); the timed region uses this form, the
    exactness checks (which need every rank and every run to see the same noise) the other."""
    g = torch.Generator(device=device).manual_seed(seed)
    B, m = cfg.TRAIN.BATCH_SIZE, cfg.MODEL
    shape = (B, m.IMAGE_SHAPE.H, m.IMAGE_SHAPE.W, m.IMAGE_SHAPE.D)
    tn = lambda: torch.nn.init.trunc_normal_(torch.empty(B, m.COMPRESSED_EMBED_DIM, device=device), 0.0, 1.0, -2.0, 2.0, generator=g)
    feed = {'x': torch.rand(shape, generator=g, device=device) * 2 - 1,
            'x_mismatch': torch.rand(shape, generator=g, device=device) * 2 - 1,
            'cond': torch.randn((B, m.EMBED_DIM), generator=g, device=device),
            'z': torch.randn((B, m.Z_DIM), generator=g, device=device),
            'epsilon': torch.rand((B, 1, 1, 1), generator=g, device=device),
            'ca_noise_d': tn(), 'ca_noise_g': tn(),
            'learning_rate_d': cfg.TRAIN.D_LR, 'learning_rate_g': cfg.TRAIN.G_LR}
    if not with_noise:
        del feed['ca_noise_d'], feed['ca_noise_g']
    return feed


class ConvTimer(object):
    """HIP-event pairs around every implicit-GEMM launch (torch.cuda.Event on the stream the kernels are launched
    on: kernels.py launches on torch's current stream).  Records (flops, start, end) per launch."""

    def __init__(self):
        self.records = []

    def begin(self, flops, algo='implicit_gemm'):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        self.records.append((flops, s, e, algo))
        return e

    def summary(self):
        from t2i_amd import kernels as K
        tot_ms = sum(s.elapsed_time(e) for _, s, e, _ in self.records)
        tot_flop = sum(f for f, _, _, _ in self.records)
        by_algo = {}
        for f, s, e, a in self.records:      # per algorithm: calls, time, direct-convolution FLOPs, FLOPs issued to the matrix cores
            r = by_algo.setdefault(a, [0, 0.0, 0.0, 0.0])
            r[0] += 1; r[1] += s.elapsed_time(e); r[2] += f; r[3] += f * K.ALGO_MAC_RATIO[K.ALGO_NAMES.index(a)]
        return dict(launches=len(self.records), ms=tot_ms, flop=tot_flop, by_algo=by_algo)


def effective_cpus():
    """Cores this process may really use: affinity mask, capped by the cgroup CPU quota (os.cpu_count() reports the
    host's 256 hardware threads inside a container that is allowed far fewer — 256 torch threads then thrash)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        with open('/sys/fs/cgroup/cpu.max') as f:
            quota, period = f.read().split()[:2]
        if quota != 'max':
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, 64))


def cpu_baseline_child(batch, budget_s=None):
    """Runs in a child process: the oracle (torch-CPU fp32 restatement of the identical D+G iteration) on the host cores."""
    from oracle import torch_step as T
    budget_s = budget_s if budget_s is not None else (15.0 if batch <= 16 else 18.0)
    threads = effective_cpus()
    torch.set_num_threads(threads)
    cfg = T.Cfg(batch=batch)
    P = T.init_variables(cfg, seed=0)
    feed = T.synthetic_feed(cfg, seed=1)
    tr = T.Trainer(cfg, P)
    t0 = time.time()
    tr.iteration(1, feed)                      # warm-up
    warm = time.time() - t0
    n, t0 = 0, time.time()
    while n < 12 and (n == 0 or (time.time() - t0) * (n + 1) / n < budget_s):     # ~10-15 s of CPU work on the GPU box's 16 cores
        tr.iteration(2 + n, feed)
        n += 1
        if n == 1 and warm > budget_s:
            break
    dt = (time.time() - t0) / n
    print(json.dumps({'value': batch / dt, 'unit': 'images/sec', 'cores': threads, 'kind': 'port',
                      'sample': '%d timed iteration(s) after 1 warm-up of the same fp32 D+G step at B=%d (%s), torch-CPU oracle' % (
                          n, batch, 'BASELINE.json configs[0], the reference\'s CPU-runnable case' if batch == 16 else
                          'the batch the metric is quoted on'),
                      'ms_per_step': dt * 1e3}))


def cpu_baseline(batch=16, timeout_s=180):
    """Bounded CPU baseline: a child process with a hard timeout, so a slow or oversubscribed host can never stall the
    default bench run (a first version used os.cpu_count()=256 threads inside a CPU-limited container: 275 s/iteration)."""
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--cpu-baseline-only', str(batch)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout_s, cwd=ROOT)
        line = [l for l in r.stdout.decode().splitlines() if l.startswith('{')][-1]
        return json.loads(line)
    except Exception as e:       # timeout / crash: say so instead of blocking or inventing a number
        return {'value': None, 'unit': 'images/sec', 'cores': effective_cpus(), 'kind': 'port',
                'sample': 'not measured: %s' % type(e).__name__}


BENCH_NOISE_SEED = 2                  # device generator seed of rank 0 (rank r: + r)
DUMP_WEIGHT_SAMPLE = 1 << 20          # weights written per arena by --dump-outputs (a fixed, seeded sample: 4 MB each)


def dump_outputs(path, out, model):
    """--dump-outputs: what the last timed iteration handed its caller — every tensor of the critic step's and the generator step's
    result dicts (loss scalars, G, D(x_hat), the gradient-penalty input gradients) — and the state it left behind: kt and a fixed,
    seeded sample of the updated critic and generator weights.  float32 .npy files, ~17 MB at B = 64."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    torch.cuda.synchronize()
    arrays = {}
    for part in ('d', 'g'):
        for k, v in sorted((out.get(part) or {}).items()):
            if torch.is_tensor(v):
                arrays['%s_%s' % (part, k)] = v.detach().float().cpu().numpy()
    arrays['kt'] = model.kt.detach().float().cpu().numpy()
    for name, arena in (('d_weights_sample', model.d_arena), ('g_weights_sample', model.g_arena)):
        n = arena.flat.numel()
        idx = np.sort(np.random.default_rng(0).choice(n, size=min(n, DUMP_WEIGHT_SAMPLE), replace=False))
        arrays[name] = arena.flat.detach()[torch.from_numpy(idx).to(arena.flat.device)].float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64 << 20, total
    for name, a in arrays.items():
        np.save(os.path.join(path, name + '.npy'), a)
    sys.stderr.write('[bench] wrote %d arrays (%.1f MB) to %s\n' % (len(arrays), total / 2.0 ** 20, path))


def _signature(model):
    return [model.d_arena.flat.clone(), model.g_arena.flat.clone(), model.D_optim.v.clone(), model.G_optim.v.clone(), model.kt.clone()]


def dp_preflight(cfg, device, make_dp, use_graphs, rank, world, batch, grad_dtype='f32', net_math=None):
    """Self-check of the N-rank exchange before anything is timed (first contact with a multi-GPU node must diagnose itself): every rank
    runs 4 iterations on IDENTICAL data through the data-parallel schedule that will be timed (2 eager iterations that learn the bucket
    counts, then the captured segments) with a single replica (no communicator) beside it IN LOCKSTEP — before every iteration the single
    replica takes the data-parallel model's weights, Adam state, kt and moving averages, then both run the iteration on the same feed.
    Averaging N identical gradients returns the gradient, so after every iteration the two gradient arenas must agree:
      * exactly where the sum is exact — fp32 buckets at N = 2 (x + x and its halving), bf16 buckets (fp32 accumulation,
        dp.DataParallel._exchange_bf16) at every power-of-two N against a replica that rounds its arena to bf16 once (dp.LocalRounding);
        there the weights, Adam state and kt after the four iterations must be bit-identical too;
      * otherwise (a ring sums 3x, 5x, ...: not representable) to the rounding of N additions: max |difference| <= 1e-5 (fp32 buckets) /
        1e-2 (bf16 buckets) of the critic arena's largest gradient per iteration, 5e-3 / 2e-2 for the generator's arena (see g_tol below).
    A bucket that is exchanged too early, twice, or not at all fails this by orders of magnitude, and the lockstep keeps the comparison
    about the EXCHANGE: round 6 found that the free-running form of this check (two runs of 4 iterations, weights compared at the end)
    reports a broken exchange for every N whose sum is inexact — 3, 6, 8 gloo ranks: 95 % of the weights more than 5 % of an Adam step
    apart, one of them 11 steps — because the model at initialisation amplifies a last-bit difference of the averaged gradient by an order of
    magnitude per iteration (Adam at beta1 = 0 on gradients that are small differences of large terms); N = 2 and 4, whose sums are exact,
    never showed it.  The weights are still compared after every iteration (how many sit more than 5 % of a step apart): reported, not fatal."""
    from t2i_amd import kernels as K
    from t2i_amd.dp import LocalRounding
    from t2i_amd.models.wgancls.model import WGanCls
    from t2i_amd.models.wgancls.trainer import WGanClsTrainer
    feed = synthetic_feed(cfg, device, seed=977)            # the same batch and noise on every rank
    lr = float(cfg.TRAIN.D_LR)

    def make(dp):
        model = WGanCls(cfg, device=device, seed=0, dp=dp)
        model.net_math = dict(net_math or {})
        model.pair_g = False          # the data-parallel schedules evaluate the generator twice per iteration: so does their single-replica reference
        return model, WGanClsTrainer(None, model, None, cfg)

    def state_of(m):
        return ({n: v.detach().clone() for n, v in m.store.vars.items()}, m.D_optim.v.clone(), m.G_optim.v.clone(), m.D_optim.t, m.G_optim.t, m.kt.clone())
    want_exact = (world == 2) if grad_dtype == 'f32' else (world & (world - 1)) == 0
    # the critic's arena is compared at the rounding of N additions; the generator's gradient of the same iteration is taken THROUGH the critic
    # the iteration has just updated, whose weights at rounding-level gradients (Adam: +-lr either way) already differ between the two — measured
    # 6e-6 .. 7e-5 of the arena's largest gradient with 3 and 8 gloo ranks — so its bound is the one a broken exchange still misses by two orders
    g_tol = (1e-5, 5e-3) if grad_dtype == 'f32' else (1e-2, 2e-2)
    # ---- the data-parallel model first: its state before every iteration, its averaged gradients and weights after (ONE model alive at a time)
    dp = make_dp()
    many, t_many = make(dp)
    dp.broadcast_variables(many.store)
    before, after = [], []
    for it in range(1, 5):
        with torch.no_grad():
            before.append(state_of(many))
        o2 = t_many.iteration(it, feed)
        if it == 2 and use_graphs:
            many.enable_graphs(feed)
        torch.cuda.synchronize()
        with torch.no_grad():                               # the data-parallel arena holds the SUM over ranks (Adam applies 1 / N)
            after.append((many.d_arena.grad * (1.0 / world), many.g_arena.grad * (1.0 / world), many.d_arena.flat.clone(), many.g_arena.flat.clone(),
                          many.kt.clone()))
    loss_dp = (float(o2['d']['D_loss']), float(o2['g']['G_loss']))
    sig_many = _signature(many)
    many._graphs = None
    del t_many, many
    # ---- the single replica, in lockstep: every iteration from the data-parallel model's state
    one, t_one = make(LocalRounding() if grad_dtype == 'bf16' else None)
    exact, finite, worst_g, worst_w, loose, kt_diff = True, True, [0.0, 0.0], 0.0, 0.0, 0.0
    for it in range(1, 5):
        vars_, dv, gv, dt_, gt_, kt_ = before[it - 1]
        with torch.no_grad():
            for n, v in vars_.items():
                one.store.vars[n].copy_(v)
            one.D_optim.v.copy_(dv); one.G_optim.v.copy_(gv)
            one.D_optim.t, one.G_optim.t = dt_, gt_
            one.kt.copy_(kt_)
        K.filter_cache_invalidate()                         # (cached filter transforms are keyed by the weights' addresses, which were just overwritten)
        o1 = t_one.iteration(it, feed)
        torch.cuda.synchronize()
        gd2, gg2, wd2, wg2, kt2 = after[it - 1]
        with torch.no_grad():
            for k_, (a1, g2, w2) in enumerate(((one.d_arena, gd2, wd2), (one.g_arena, gg2, wg2))):
                g1 = a1.grad
                finite = finite and bool(torch.isfinite(g2).all())
                exact = exact and torch.equal(g1, g2)
                worst_g[k_] = max(worst_g[k_], float((g1 - g2).abs().max()) / max(float(g1.abs().max()), 1e-30))
                d = (a1.flat - w2).abs()
                worst_w = max(worst_w, float(d.max()) / lr)
                loose = max(loose, float((d > 0.05 * lr).float().mean()))
            kt_diff = max(kt_diff, abs(float(one.kt) - float(kt2)))
    losses = [(float(o1['d']['D_loss']), float(o1['g']['G_loss'])), loss_dp]
    exact = exact and all(torch.equal(a, b) for a, b in zip(_signature(one), sig_many))
    finite = finite and all(bool(torch.isfinite(t).all()) for t in sig_many)
    kt_scale = max(abs(float(sig_many[4])), 1.0)
    del t_one, one, before, after
    report = {'ranks': world, 'iterations': 4, 'form': 'lockstep', 'gradient_buckets': grad_dtype, 'exact': bool(exact), 'exact_required': bool(want_exact),
              'max_gradient_diff_rel': {'critic': worst_g[0], 'generator': worst_g[1]}, 'gradient_tolerance': {'critic': g_tol[0], 'generator': g_tol[1]},
              'max_weight_diff_in_steps': worst_w,
              'frac_weights_off_by_5pct_of_a_step': loose, 'kt_diff': kt_diff, 'loss_single': losses[0], 'loss_dp': losses[1]}
    grads_ok = exact if want_exact else (worst_g[0] <= g_tol[0] and worst_g[1] <= g_tol[1])
    # (statistical part: measured 0.9e-3 / 1.3e-3 of the weights more than 5 % of a step apart with 8 / 3 gloo ranks — the ones whose gradient is at rounding level)
    ok = finite and grads_ok and (want_exact or (loose <= 1e-2 and kt_diff <= 1e-5 * kt_scale))
    report['ok'] = bool(ok)
    # What stops the run: what a BROKEN exchange produces — a non-finite value, or averaged gradients that are not the gradient by orders of
    # magnitude more than any summation order explains (a bucket exchanged too early, twice or not at all: O(1) of the arena's largest gradient;
    # the line is drawn at 1e-2 for the critic's arena, 1e-1 for the generator's).  Everything finer — a last-bit difference where exactness is
    # owed, a gradient outside the rounding bound, the statistical part (how many weights sit more than 5 % of a step from the single replica's
    # after one iteration from the same state) — has never met a real ring: the line then carries ok = false and the numbers, and the timing
    # goes ahead.  (Eight gloo ranks time-slicing ONE GPU — the pre-flight of this pre-flight — have produced a wrong gradient on a single
    # rank, 1.3e-3, and HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION aborts; two to four ranks, and one process per GPU, never have.)
    fatal = (not finite) or worst_g[0] > 1e-2 or worst_g[1] > 1e-1
    if os.environ.get('T2I_PREFLIGHT') == 'strict':          # every bound stops the run, the statistical one included
        fatal = fatal or not ok
    report['fatal'] = bool(fatal)
    if not ok:
        sys.stderr.write('[bench] data-parallel preflight, rank %d: %s\n' % (rank, report))
    flag = torch.tensor([1 if fatal else 0, 0 if ok else 1], device=device)
    torch.distributed.all_reduce(flag)
    report['ranks_outside_bounds'] = int(flag[1])
    report['ok'] = bool(ok) and int(flag[1]) == 0           # every rank's verdict, not this one's alone
    if int(flag[1]) != 0 and int(flag[0]) == 0 and rank == 0:
        sys.stderr.write('[bench] data-parallel preflight: outside its bounds on %d rank(s), not fatal (rank 0 saw %s)\n' % (int(flag[1]), report))
    if int(flag[0]) != 0:
        raise SystemExit('[bench] DATA-PARALLEL PREFLIGHT FAILED on rank %d of %d: on identical data the %d-rank exchange does not return the '
                         'single replica\'s gradients (%s).  The gradient exchange is broken on this node: not timing it.  '
                         '(T2I_PREFLIGHT=0 skips this check; T2I_DP_GRAPHS=0 selects the eager overlap schedule.)' % (rank, world, world, report))
    return report


def run_config(args, math, device, rank, local_rank, world, use_dp, make_dp, headline=True, g_mode='config3'):
    """g_mode (math 'bf16' only): 'config3' = the arithmetic whose parity test holds every tensor to 2e-2 (kernels.CONFIG3_NET_MATH: critic
    and the generator's backward GEMMs in bf16 math, the generator's forward GEMMs in fp32 math); 'all_bf16' = every GEMM in bf16 math
    (a labelled side row: outside the stated tolerance).
    Builds the model in arithmetic `math` ('f32' = BASELINE config 2, the metric; 'bf16' = config 3), warms it up, times it and
    (rank 0) attaches the roofline block.  Everything it creates is released before it returns, so that a second configuration
    can run in the same process (cached filter images of the first are dropped: their graphs are gone)."""
    import gc
    import math as _m
    from t2i_amd import autograd as A
    from t2i_amd import kernels as K
    from t2i_amd.models.wgancls.model import WGanCls
    from t2i_amd.models.wgancls.trainer import WGanClsTrainer
    K.set_storage('f32')
    K.set_math(math)
    storage = 'f32'
    if math == 'bf16' and args.storage == 'bf16':
        K.set_storage('bf16')           # config 3 end to end: activations and their gradients are bf16 tensors between the kernels
        storage = 'bf16'
    net_math = dict(K.CONFIG3_NET_MATH) if (math == 'bf16' and g_mode == 'config3') else {}
    cfg = make_cfg(args.batch)
    dp, grad_dtype = make_dp(math)
    use_graphs = not args.no_graphs and args.instrument != 'inline' and not (use_dp and os.environ.get('T2I_DP_GRAPHS') == '0')
    preflight = None
    # (a check, not part of the headline: on with --full, or with T2I_PREFLIGHT=1 / strict)
    if world > 1 and os.environ.get('T2I_PREFLIGHT', '1' if args.full else '0') != '0':
        preflight = dp_preflight(cfg, device, lambda: make_dp(math)[0], use_graphs, rank, world, args.batch, grad_dtype=grad_dtype, net_math=net_math)
        if rank == 0:
            sys.stderr.write('[bench] data-parallel preflight (%s) passed: %r\n' % (math, preflight))
    # the conditioning-augmentation noise the iteration draws comes from the device's torch generator, whose default seed differs from
    # process to process: seeded, so that the same arguments give the same inputs (and --dump-outputs the same outputs) in every run
    torch.cuda.manual_seed(BENCH_NOISE_SEED + rank)
    model = WGanCls(cfg, device=device, seed=0, dp=dp)
    model.net_math = net_math
    if dp is not None:
        dp.broadcast_variables(model.store)
    trainer = WGanClsTrainer(None, model, None, cfg)
    # T2I_SAME_DATA=1 (diagnostics): every rank sees rank 0's batch and noise, so the averaged gradients equal the local ones
    # and an N-rank run must end with EXACTLY the weights of a single process — a check of the exchange that, unlike the
    # replica comparison, also catches buckets that are exchanged consistently but too early
    same_data = os.environ.get('T2I_SAME_DATA') == '1'
    # the timed feed carries no conditioning noise: the two [B, 128] truncated-normal draws of an iteration happen inside it
    feed = synthetic_feed(cfg, device, seed=1 + (0 if same_data else rank), with_noise=os.environ.get('T2I_BENCH_FEED_NOISE') == '1')
    if same_data:
        torch.manual_seed(1234)
        torch.cuda.manual_seed_all(1234)

    def barrier():
        if use_dp:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # N > 1: the iteration is cut at its exchange steps and the collectives themselves are never captured.
    # T2I_DP_GRAPHS=0 keeps the data-parallel step eager (bucketed overlap, dp.py).
    if args.side_stream:
        A.enable_side_stream(True)
    if use_graphs:
        # set-up, before the W warm-up steps: eager iterations settle workspaces, kernel attributes, the filter cache's
        # buffers and (N > 1) the communicator, then the iteration is captured; warm-up and timed steps are replays
        for i in range(2):
            trainer.iteration(1 + i, feed)
        model.enable_graphs(feed)
        # the synthetic batch is resident in HBM; from here on it lives IN the captured graphs' input buffers (what a data pipeline
        # writing its batch in place does), so no per-step device-to-device copy of the inputs sits in front of a replay
        feed.update({k: v for k, v in model.static_inputs().items() if feed.get(k) is not None})   # noise the feed lacks is still re-drawn
    for i in range(args.warmup):
        trainer.iteration(3 + i, feed)
    timer = ConvTimer()
    it = 3 + args.warmup

    def timed_region(record=False):
        """EXACTLY --steps iterations between barrier + synchronize on both sides; max over ranks."""
        nonlocal it
        barrier()
        if record:
            K.set_conv_timer(timer)
        t0 = time.perf_counter()
        for i in range(args.steps):
            trainer.iteration(it, feed)
            it += 1
        barrier()
        dt_r = time.perf_counter() - t0
        K.set_conv_timer(None)
        if use_dp:
            t = torch.tensor([dt_r], device=device, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt_r = float(t)
        return dt_r

    # --repeats timed regions at least, and as many more as it takes to keep the GPU busy for --min-busy-s seconds in total (a
    # 20-step region lasts 0.3 s: the driver's once-a-second utilisation sampler saw an idle GPU in round 2); every region is
    # exactly --steps iterations, the MEDIAN region is reported and all are listed
    regions = [timed_region(record=(args.instrument == 'inline'))]
    want = max(1, args.repeats)
    if args.min_busy_s > 0 and regions[0] > 0:
        want = max(want, min(int(_m.ceil(args.min_busy_s / regions[0])), 64))
    if use_dp:                                  # every rank must run the same number of regions
        t = torch.tensor([want], device=device, dtype=torch.int64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        want = int(t)
    while len(regions) < want:
        regions.append(timed_region())
    dt = sorted(regions)[len(regions) // 2]     # median region
    if headline and rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, trainer.last, model)
    exchange = None
    inst_steps = args.steps
    if args.instrument == 'after':          # same workload, immediately after the timed region, with per-launch events
        inst_steps = min(args.steps, 3)
        saved_graphs, model._graphs = model._graphs, None      # per-launch events need eager launches
        A.enable_side_stream(False)                            # ... and one stream, so durations are per kernel
        # the eager instrumented pass must not be host-bound, or the idle time between a start event and the launches behind it
        # is booked as kernel time (bf16 mode: ~700 launches take the host 16 ms, the GPU 8): a spin kernel at the head of the
        # iteration lets the host run ahead, so the events bracket queued work only.  Its tick rate is calibrated first.
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); torch.cuda._sleep(1000000); e1.record(); torch.cuda.synchronize()
        ticks_per_ms = 1000000 / max(e0.elapsed_time(e1), 1e-3)
        headstart = int(float(os.environ.get('T2I_INSTRUMENT_HEADSTART_MS', '60')) * ticks_per_ms)
        K.set_conv_timer(timer)
        for i in range(inst_steps):
            torch.cuda._sleep(headstart)
            trainer.iteration(it + i, feed)
        torch.cuda.synchronize()
        K.set_conv_timer(None)
        model._graphs = saved_graphs

    if same_data and rank == 0:
        torch.cuda.synchronize()
        sys.stderr.write('[bench] signature after %d iterations: %r\n' % (model.global_step, [
            float(model.d_arena.flat.double().sum()), float(model.g_arena.flat.double().sum()), float(model.D_optim.v.double().sum()),
            float(model.G_optim.v.double().sum()), float(model.kt)]))
    if use_dp and os.environ.get('T2I_CHECK_SYNC') == '1':      # replicas must still hold identical weights, Adam state and kt
        sig = torch.stack([model.d_arena.flat.double().sum(), model.g_arena.flat.double().sum(), model.D_optim.v.double().sum(),
                           model.kt.double()])
        lo, hi = sig.clone(), sig.clone()
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        if not torch.equal(lo, hi):
            names = list(model.store.vars.keys())       # which variables: per-variable checksums, min/max over ranks
            per = torch.stack([model.store.vars[n].detach().double().sum() for n in names])
            plo, phi = per.clone(), per.clone()
            torch.distributed.all_reduce(plo, op=torch.distributed.ReduceOp.MIN)
            torch.distributed.all_reduce(phi, op=torch.distributed.ReduceOp.MAX)
            bad = [names[i] for i in range(len(names)) if plo[i] != phi[i]]
            raise SystemExit('replicas diverged: %s vs %s; variables that differ: %s' % (lo.tolist(), hi.tolist(), bad[:40]))
        if rank == 0:
            sys.stderr.write('[bench] replica sync check passed: %s\n' % sig.tolist())
    # the exchange itself, measured on 3 more iterations of the same schedule (events on the communication stream around every
    # collective, on the compute stream around every wait for them): bytes, ms in collectives, ms stalled, overlap fraction
    if use_dp and dp is not None and args.full:
        barrier()
        dp.begin_stats()
        for i in range(3):
            trainer.iteration(it, feed)
            it += 1
        barrier()
        exchange = dp.end_stats(3)
        ones = torch.ones(1, device=device)
        torch.distributed.all_reduce(ones)
        exchange['ranks_counted_by_all_reduce'] = int(ones.item())
        exchange['backend'] = str(torch.distributed.get_backend())
        if exchange['backend'] != 'nccl':
            exchange['note'] = ('test transport: gloo blocks the HOST inside each collective, so the compute stream is idle rather than stalled — '
                                'ms_compute_stream_stalled / overlap_fraction are meaningful with RCCL only')
    ms = dt / args.steps * 1e3
    value = args.batch * world * args.steps / dt
    schedule = getattr(model, 'dp_schedule', None)

    out = {'metric': 'images/sec (G+D step) at 64x64 batch=64', 'value': value, 'unit': 'images/sec', 'n_gpus': world,
           'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms, 'higher_is_better': True, 'scaling': 'weak',
           'vs_baseline': None, 'dtype': math, 'data': 'synthetic',
           'config': {'workload': 'wgancls 64x64 batch=%d/GPU ' % args.batch + ('fp32' if math == 'f32' else
                                  'bf16 MFMA, %s activation tensors, fp32 accumulate + master weights (BASELINE config 3)' % ('bf16' if storage == 'bf16' else 'fp32')) + ', synthetic images + random 1024-d text embeddings, '
                                  'D step (+kt) then G step, Adam(b1=0,b2=0.9)',
                      'global_batch': args.batch * world, 'parallelism': 'dp%d' % world,
                      'gradient_exchange': (grad_dtype + ' buckets over RCCL' + (' (fp32 accumulation)' if grad_dtype == 'bf16' else '')) if use_dp else None,
                      'launch': ('hipGraph replay (%s)' % ((schedule or 'graph segments + eager all-reduces') if use_dp else '1 graph/iteration')) if use_graphs else 'eager'},
           # SURVEY 8(d)'s nominal 31.362 GFLOP/image books 4 conv launches per critic layer whose operand is identically zero and
           # which are never launched; it is NOT a utilisation figure (roofline.frac is, from the launched convs' FLOPs)
           'survey_nominal_tflops_overcounts_zero_branches': NOMINAL_FLOP_PER_IMAGE * value / 1e12,
           'timing': {'regions': len(regions), 'steps_per_region': args.steps, 'statistic': 'median over regions (max over ranks per region)',
                      'gpu_busy_s': sum(regions), 'ms_per_step_by_region': [r / args.steps * 1e3 for r in regions]}}
    if preflight is not None:
        out['dp_preflight'] = preflight
        # top level, beside `value`: a reader of the line (or of its exit status, below) cannot miss a run that was timed although
        # the statistical part of the N > 2 fp32 bound was exceeded (T2I_PREFLIGHT=strict makes that fatal instead)
        out['dp_preflight_ok'] = bool(preflight.get('ok'))
    if exchange is not None:
        # rccl_ranks: how many ranks an all-reduce of ones over the communicator counted (== n_gpus or the line is not an N-GPU line)
        out['rccl_ranks'] = exchange['ranks_counted_by_all_reduce']
        out['gradient_exchange'] = exchange
    if math == 'bf16':
        out['arithmetic'] = ({'mode': 'config3', 'critic': 'bf16 MFMA on bf16 tensors (17 of the iteration\'s 21 network passes)',
                              'generator_backward': 'bf16 MFMA (input- and filter-gradient GEMMs), fp32 tensors with bf16 operand images',
                              'generator_forward': 'fp32 MFMA on fp32 tensors (2 passes per iteration)',
                              'why': 'DESIGN 4.16: every tensor of the step within BASELINE.md\'s 2e-2 (tests/test_step_b64_gpu.py[config3])'}
                             if g_mode == 'config3' else
                             {'mode': 'all_bf16', 'note': 'every GEMM of both networks in bf16 math: outside the 2e-2 tolerance (generator-step gradients '
                                                          'up to 1.07e-1), NOT a config-3 claim'})
    if rank == 0 and args.instrument != 'off':
        s = timer.summary()
        info = K.device_info(local_rank)
        achieved = s['flop'] / (s['ms'] * 1e-3) / 1e12 if s['ms'] > 0 else 0.0
        peak = FP32_MATRIX_PEAK_TFLOPS if math == 'f32' else BF16_MATRIX_PEAK_TFLOPS
        # HBM-side bytes per launch and MFMA pipe utilisation come from rocprofv3 PMC passes over this same command
        # (separate --pmc runs, tools/pmc_summary.py), NOT from this run: they are labelled "from_profile", carry the
        # profile's own launch count, and are dropped when that count is not this run's (another planner / algorithm mix)
        traffic, mfma_util, prof = None, None, None
        launches_per_step = s['launches'] / float(inst_steps)
        # the profile counts igemm_kernel dispatches; every conv entry-point call launches exactly one, except the small direct kernels
        igemm_per_step = launches_per_step - (s['by_algo'].get('direct_small', [0])[0] / float(inst_steps))
        suffix = '' if math == 'f32' else '_bf16'
        for cand in ('r06_pmc_igemm%s.json' % suffix, 'r05_pmc_igemm%s.json' % suffix, 'r04_pmc_igemm%s.json' % suffix, 'r03_pmc_igemm%s.json' % suffix, 'r02_pmc_igemm%s.json' % suffix, 'r01_pmc_igemm.json'):
            try:
                pmc = json.load(open(os.path.join(ROOT, 'profiles', cand)))
            except Exception:
                continue
            if pmc.get('math', 'f32') != math:
                continue
            prof = {'source': 'from_profile', 'file': 'profiles/' + cand, 'counters': 'FETCH_SIZE x2 + WRITE_SIZE; SQ_VALU_MFMA_BUSY_CYCLES',
                    'profile_igemm_launches_per_step': pmc.get('launches_per_iteration'), 'run_igemm_launches_per_step': igemm_per_step}
            # (bf16: the profile counts GEMM-kernel DISPATCHES — a pair launch is one, a staged boundary layer's generic GEMM is one more —
            # while this run counts entry-point CALLS: the two differ by a handful of launches for the same algorithm mix, hence 8 %)
            same = pmc.get('launches_per_iteration') is not None and abs(pmc['launches_per_iteration'] - igemm_per_step) <= (0.02 if math == 'f32' else 0.08) * igemm_per_step
            prof['counts_agree'] = bool(same)
            if same:
                traffic, mfma_util = pmc.get('traffic_bytes_per_launch'), pmc.get('mfma_util')
                # the GEMM kernels alone (rocprofv3 durations of the PMC pass) against the multiply-adds they actually issue
                # (round 2 credited them with the direct-convolution FLOPs of the Winograd layers: > 1 by construction)
                if pmc.get('igemm_ms_per_iteration_profiled'):
                    ex = sum(r[3] for a, r in s['by_algo'].items() if a != 'direct_small') / inst_steps
                    gk = ex / (pmc['igemm_ms_per_iteration_profiled'] * 1e-3) / 1e12
                    prof['gemm_kernels_only'] = {'ms_per_step': pmc['igemm_ms_per_iteration_profiled'], 'executed_tflops': gk,
                                                 'executed_frac': gk / peak,
                                                 'note': 'multiply-adds issued by the GEMM kernels / their profiled time (transforms, reductions and thin kernels excluded)'}
            break
        flop_per_step = s['flop'] / inst_steps
        driver_tflops = flop_per_step / (ms * 1e-3) / 1e12          # algorithmic FLOPs of the launched convs over the replayed step
        # compulsory HBM bytes of the same launches (Σ layer in+out per pass, 286 MB per generator pass and 161 MB per
        # critic pass at B = 64 in fp32, 4 generator-side and 15 critic-side passes are launched; half in bf16 storage)
        compulsory = (4 * 286e6 + 15 * 161e6) * (args.batch / 64.0) * (0.5 if storage == 'bf16' else 1.0)
        igemm_launches = prof['profile_igemm_launches_per_step'] if (prof and prof.get('counts_agree')) else None      # per-launch figures x the PROFILE's launch count = its per-step totals
        out['roofline'] = {
            'bound': 'mfma', 'kernel': 't2i::igemm_kernel<MODE,WMT,WNT,VEC> + t2i::bgemm_kernel<LAY> / bgemm9_kernel<LAY> (all conv/deconv/dense launches; the Winograd paths\' batched GEMMs run in bgemm_kernel, the fused nine-position form in bgemm9_kernel)'
                     if math == 'f32' else 't2i::igemm_hd_kernel<MODE,WMT,WNT> + t2i::igemm_hft_kernel (bf16 operands by LDS DMA) + the fp32 thin-layer kernels',
            'achieved': driver_tflops, 'peak': peak, 'unit': 'TFLOP/s',
            # round 4: `frac` is the driver-clock figure (algorithmic FLOPs of the launched convs / ms_per_step of the replayed
            # iteration, everything that is not a convolution included); the eager per-launch event sum is kept beside it
            'frac': driver_tflops / peak, 'frac_vs_driver_ms': driver_tflops / peak,
            'achieved_entry_points': achieved, 'frac_entry_points': achieved / peak,
            'traffic': traffic, 'traffic_source': prof, 'mfma_util': mfma_util,
            'traffic_per_step': (traffic * igemm_launches) if (traffic and igemm_launches) else None,
            'compulsory_bytes_per_step': compulsory,
            'traffic_over_compulsory': (traffic * igemm_launches / compulsory) if (traffic and igemm_launches) else None,
            'algorithmic_flop_per_launch': s['flop'] / max(s['launches'], 1),
            'launches_per_step': launches_per_step, 'igemm_ms_per_step': s['ms'] / inst_steps,
            'igemm_gflop_per_step': flop_per_step / 1e9, 'events': args.instrument,
            # `achieved` counts direct-convolution FLOPs; the Winograd paths issue 1/2.25 resp. 9/16 of them
            'executed_tflops': sum(r[3] for r in s['by_algo'].values()) / (s['ms'] * 1e-3) / 1e12 if s['ms'] > 0 else 0.0,
            'executed_frac': (sum(r[3] for r in s['by_algo'].values()) / (s['ms'] * 1e-3) / 1e12 / peak) if s['ms'] > 0 else 0.0,
            'note': 'frac = achieved / peak with achieved = direct-convolution FLOPs of the launched conv calls / ms_per_step (the replayed '
                    'iteration on the driver\'s clock); frac_entry_points = the same FLOPs / time inside the conv entry points (eager '
                    'instrumented pass; Winograd issues 1/2.25 resp. 9/16 of them); executed_frac = multiply-adds actually issued / peak over '
                    'the entry-point time; mfma_util = PMC pipe-busy fraction (from_profile); traffic = HBM-side bytes per GEMM launch '
                    '(from_profile), traffic_over_compulsory = per step against the minimum activation + weight bytes of the same launches',
            'by_algorithm': {a: {'calls_per_step': r[0] / float(inst_steps), 'ms_per_step': r[1] / inst_steps,
                                 'algorithmic_tflops': r[2] / (r[1] * 1e-3) / 1e12 if r[1] > 0 else 0.0}
                             for a, r in sorted(s['by_algo'].items())},
            'device': info}
    # release everything this configuration holds (graphs first: they point into the filter cache and the workspace)
    A.enable_side_stream(False)
    model._graphs = None
    del trainer, model, feed, dp
    gc.collect()
    torch.cuda.synchronize()
    K.filter_cache_reset()
    K.set_storage('f32')
    K.set_math('f32')
    torch.cuda.empty_cache()
    return out


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-run this command line as N ranks of ONE node, exactly the way the driver
    does it (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...).
    Rank 0's JSON line is the child's stdout, passed through untouched.  Returns the launcher's exit code."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < n and os.environ.get('T2I_SAME_DEVICE') != '1':
        sys.stderr.write('[bench] --gpus %d but %d GPU(s) visible here (T2I_SAME_DEVICE=1 T2I_DIST_BACKEND=gloo runs the N-rank path '
                         'on one device as a pre-flight)\n' % (n, have))
        return 2
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:       # a free port on the loopback interface
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stderr.write('[bench] launching %d ranks: %s\n' % (n, ' '.join(cmd)))
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', '4')
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64, help='per-GPU batch')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-graphs', action='store_true', help='keep the step eager (default: hipGraph replay on 1 GPU)')
    ap.add_argument('--full', action='store_true',
                    help='also measure and check everything beyond the headline (more timed regions, roofline pass, config3_bf16 block, '
                         'side rows, CPU baselines; N > 1: data-parallel preflight and exchange statistics)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed iteration computed as DIR/<name>.npy (float32)')
    ap.add_argument('--instrument', choices=['inline', 'after', 'off'], default=None,
                    help='where the per-launch HIP events for the roofline block are recorded (default: after with --full, off otherwise)')
    ap.add_argument('--math', choices=['f32', 'bf16'], default='f32',
                    help="conv arithmetic: f32 = BASELINE config 2 (the headline metric); bf16 = config 3 (bf16 MFMA "
                         "operands, fp32 accumulation and fp32 tensors) -- reported with dtype 'bf16', never the default")
    ap.add_argument('--storage', choices=['f32', 'bf16'], default=os.environ.get('T2I_STORAGE', 'bf16'),
                    help="with --math bf16 (and for the config3_bf16 block): 'bf16' = activation tensors are bf16 in HBM end to end "
                         "(ABI v6, default); 'f32' = fp32 tensors with bf16 operand images beside them (round 2)")
    ap.add_argument('--side-stream', type=int, default=int(os.environ.get('T2I_SIDE_STREAM', '0')),
                    help='1: sunk filter gradients run on a second HIP stream, concurrently with the bwd-data chain')
    ap.add_argument('--repeats', type=int, default=None,
                    help='timed regions of --steps iterations each, every one bracketed by barrier + synchronize; the MEDIAN is reported '
                         '(default: 3 with --full, 1 otherwise)')
    ap.add_argument('--min-busy-s', type=float, default=None,
                    help='keep adding timed regions (each exactly --steps iterations) until the GPU has been busy this long in total '
                         '(default: 3.0 with --full, 0 otherwise)')
    ap.add_argument('--no-config3', action='store_true', help='skip the config3_bf16 block (bf16 arithmetic) behind the fp32 headline')
    ap.add_argument('--no-side-rows', action='store_true', help='skip the b8_per_gpu and next_rows blocks')
    ap.add_argument('--side-budget-s', type=float, default=0.6, help='timed replay budget per side row')
    ap.add_argument('--cpu-baseline-only', type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.instrument is None:
        args.instrument = 'after' if args.full else 'off'
    if args.repeats is None:
        args.repeats = 3 if args.full else 1
    if args.min_busy_s is None:
        args.min_busy_s = 3.0 if args.full else 0.0
    if args.cpu_baseline_only:
        cpu_baseline_child(args.cpu_baseline_only)
        return

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(args.gpus))            # `python bench.py --gpus N` on its own: one rank per GPU through torch.distributed.run
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node %d (or unset WORLD_SIZE and let bench.py launch itself)'
                         % (args.gpus, world, args.gpus))
    # Pre-flight hooks for boxes with ONE GPU: T2I_SAME_DEVICE=1 puts every rank on device 0 and T2I_DIST_BACKEND=gloo
    # replaces RCCL (which refuses two ranks on one device), so the whole multi-process path — rendezvous, bucket order,
    # overlap hooks, barriers, max-over-ranks timing — runs for real, minus the xGMI transport.  Never set by the driver.
    if os.environ.get('T2I_SAME_DEVICE') == '1':
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device('cuda', local_rank)

    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K

    # T2I_FORCE_DP=1 exercises the data-parallel machinery (RCCL communicator, bucket hooks, side stream) on ONE rank
    use_dp = world > 1 or os.environ.get('T2I_FORCE_DP') == '1'
    if use_dp:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        os.environ.setdefault('RANK', '0')
        os.environ.setdefault('WORLD_SIZE', '1')
        backend = os.environ.get('T2I_DIST_BACKEND', 'nccl')
        import datetime
        tmo = datetime.timedelta(seconds=int(os.environ.get('T2I_DIST_TIMEOUT_S', '600')))   # a stuck collective aborts the run instead of hanging it
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=device, timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)

    K.filter_cache(os.environ.get('T2I_FILTER_CACHE', '1') != '0')     # transformed Winograd filters reused until Adam changes them
    bucket = int(os.environ.get('T2I_DP_BUCKET_MB', '32')) << 20

    def make_dp(math):
        if not use_dp:
            return None, None
        from t2i_amd.dp import DataParallel
        # gradient buckets: fp32 in place for the fp32 metric; bf16 on the wire (half the bytes per link), summed in fp32, for config 3
        gd = os.environ.get('T2I_DP_GRAD_DTYPE', 'bf16' if math == 'bf16' else 'f32')
        return DataParallel(bucket_bytes=bucket, grad_dtype=gd), gd

    out = run_config(args, args.math, device, rank, local_rank, world, use_dp, make_dp, headline=True)
    # BASELINE config 3 (bf16 MFMA operands, fp32 accumulate / master weights, bf16 gradient buckets under data parallelism) rides
    # on the SAME JSON line as a block of its own, so the driver's record holds it; the headline stays the fp32 metric.
    if args.full and args.math == 'f32' and not args.no_config3 and os.environ.get('T2I_BENCH_CONFIG3', '1') != '0':
        import copy
        a3 = copy.copy(args)
        a3.repeats = max(1, min(args.repeats, 3))
        c3 = run_config(a3, 'bf16', device, rank, local_rank, world, use_dp, make_dp, headline=False, g_mode='config3')
        side = None
        if os.environ.get('T2I_BENCH_ALL_BF16_ROW', '1') != '0':
            a3b = copy.copy(a3)
            a3b.repeats, a3b.min_busy_s, a3b.instrument = 1, 0.0, 'off'
            side = run_config(a3b, 'bf16', device, rank, local_rank, world, use_dp, make_dp, headline=False, g_mode='all_bf16')
        if rank == 0:
            keep = ('value', 'unit', 'ms_per_step', 'dtype', 'n_gpus', 'steps', 'warmup', 'config', 'arithmetic', 'timing', 'roofline', 'dp_preflight',
                    'rccl_ranks', 'gradient_exchange')
            blk = {k: c3[k] for k in keep if k in c3}
            blk['vs_fp32_line'] = c3['value'] / out['value'] if out.get('value') else None
            if side is not None:
                blk['all_bf16_side_row'] = {'value': side['value'], 'unit': side['unit'], 'ms_per_step': side['ms_per_step'],
                                            'vs_fp32_line': side['value'] / out['value'] if out.get('value') else None,
                                            'arithmetic': side.get('arithmetic'),
                                            'parity': 'NOT within BASELINE.md\'s 2e-2 (tests/test_step_b64_gpu.py[all_bf16] states its measured envelope: G 2.15e-2, '
                                                      'D(x_hat) 3.8e-2, generator-step gradients <= 1.07e-1): reported for the kernels\' sake, not as config 3'}
            blk['parity'] = {
                'test': 'tests/test_step_b64_gpu.py::test_config3_bf16_steps_mask_pinned[B64] (also [B16], [B8]; full width, in the form replayed here — one 2B-row '
                        'generator evaluation, the stacked critic step, the generator step on the leading half —, mask-pinned vs the float64 oracle, '
                        'plus G, D(x_hat) and every loss scalar against the UN-pinned oracle)',
                'stated_in_BASELINE_md': 'bf16-MFMA configuration: rel <= 2e-2 vs the fp32 oracle',
                'bounds_relative_l2': {'G': 2e-2, 'D(x_hat)': 2e-2, 'grad_x_hat': 2e-2, 'loss_scalars': 2e-2, 'critic_step_gradients': 2e-2,
                                       'generator_step_gradients': 2e-2},
                # measured on MI355X, round 5 (profiles/r05_config3_error_table.txt, tools/bf16_error_table.py --variants g_fwd_f32)
                'measured_relative_l2': {'G': 3.5e-6, 'D(x) activations, every layer': '<= 6.5e-3', 'D(x_hat) logit': 1.24e-2, 'grad_x_hat': 6.6e-3,
                                         'critic_step_gradients worst': 1.49e-2, 'loss_scalars worst': 7.0e-3,
                                         'generator_step_gradients worst / median': [1.04e-2, 8.4e-3]},
                'above_2e-2': None,
                # round 6 (profiles/r06_bf16_side_row_parity.txt): what the pinning touches, and the forward quantities without any pinning
                'pinned_branch_fraction': {'bound_asserted': 1.5e-3, 'critic_step': 5.44e-4, 'generator_step': 3.47e-4, 'fp32_generator_pass': 4.0e-7},
                'unpinned_forward_relative': {'G': 3.5e-6, 'D(x_hat)': 1.13e-2, 'loss_scalars worst': 3.3e-3, 'bound': 2e-2},
                'forward_error_yardstick': 'config 3: relative L2 per tensor.  The fp32 headline\'s G is held to max|G - ref| <= 1e-5 x max|pre-tanh logits| '
                                           '(logits reach |59|; against max|G| = 1 the same run measures <= 2.3e-5, tests/test_step_b64_gpu.py prints both)',
                'kernel_arithmetic': 'tests/test_kernels_gpu.py::test_bf16_operand_gemm_matches_rounded_oracle: 1e-5 / 1e-4 vs float64 on bf16-rounded operands'}
            out['config3_bf16'] = blk
    # SURVEY 8(d)'s strong-scaling share (global 64 = 8 per GPU = the yml's BATCH_SIZE) and the next rows (gancls, StackGAN, PGGAN):
    # short measured rows on the same line — images/s, algorithmic GFLOP/image, fraction of the matrix peak on the replayed clock
    if (args.full and rank == 0 and world == 1 and args.math == 'f32' and not args.no_config3 and not args.no_side_rows and args.instrument != 'off' and
            os.environ.get('T2I_BENCH_SIDE_ROWS', '1') != '0'):      # only on the full default line (diagnostic invocations skip them)
        from tools.next_rows import measure_rows
        b8 = measure_rows(['wgancls_b8'], 'f32', args.side_budget_s, device) + measure_rows(['wgancls_b8'], 'bf16', args.side_budget_s, device, args.storage)
        out['b8_per_gpu'] = {'what': 'wgancls at batch 8 per GPU (strong scaling of global batch 64 over 8 GPUs; models/wgancls/cfg/flowers.yml:24), '
                                     'hipGraph replay, noise drawn inside the iteration', 'f32': b8[0], 'bf16': b8[1]}
        rows = measure_rows(['gancls', 'stage1', 'stage2', 'pggan7'], 'f32', args.side_budget_s, device)
        rows += measure_rows(['stage2'], 'bf16', args.side_budget_s, device, 'f32')     # (fp32 activation tensors + bf16 operand images: the StackGAN graphs mix 3-channel joins into 64-multiples)
        out['next_rows'] = {'what': 'SURVEY 8(f) rows + the gancls variant at the reference\'s dimensions and batch sizes; algorithmic_gflop_per_image = '
                                    'direct-convolution FLOPs of the conv/deconv/dense calls one iteration launches / batch', 'rows': rows}
    if args.full and rank == 0 and not args.no_cpu_baseline and world == 1:      # the CPU leg is reported at N=1 only (the other ranks would idle in the final barrier)
        out['cpu_baseline'] = cpu_baseline(16)              # BASELINE configs[0]
        out['cpu_baseline_b64'] = cpu_baseline(64)          # and the batch the metric is quoted on
    if use_dp:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    # RCCL writes its version banner (NCCL_DEBUG=VERSION in this image) into the C stdio buffer, which would otherwise be
    # flushed at exit, AFTER the JSON line: flush it first so the JSON line is the last thing on stdout
    sys.stdout.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    if rank == 0:
        print(json.dumps(out))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
