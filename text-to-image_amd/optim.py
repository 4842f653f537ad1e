"""Flat parameter arenas + tf.train.AdamOptimizer semantics (reference models/wgancls/model.py:94-106).

All trainable variables of one optimizer live back-to-back in ONE device buffer (16-byte aligned slots), with
gradients, first and second moments in three more buffers of the same shape.  A step is then a single kernel launch
over ~29 M (critic) / ~23 M (generator) floats instead of one launch per tensor, and data-parallel gradient exchange
works on contiguous slices of the gradient arena (dp.py)."""
import math
import numbers
from collections import OrderedDict

import torch

from . import kernels as K


class Arena(object):
    def __init__(self, variables):
        """variables: OrderedDict name -> leaf tensor.  Re-points every variable's storage (and .grad) into the arena."""
        self.names = list(variables.keys())
        self.vars = variables
        self.offsets = OrderedDict()
        off = 0
        for n, v in variables.items():
            self.offsets[n] = (off, v.numel())
            off += (v.numel() + 3) // 4 * 4          # 16-byte slots: the kernels' float4 paths need aligned bases
        self.numel = off
        dev = next(iter(variables.values())).device
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for n, v in variables.items():
                o, k = self.offsets[n]
                self.flat[o:o + k].copy_(v.reshape(-1))
                v.data = self.flat[o:o + k].view(v.shape)
                v.grad = self.grad[o:o + k].view(v.shape)
        K.filter_cache_invalidate()                  # the variables moved (possibly onto recycled addresses)

    def zero_grad(self):
        # an optimizer that derives its first moment from this arena on demand (AdamTF with beta1 == 0) is about to lose its source:
        # let it form the moment first.  (Not inside a capture: a replayed iteration leaves the last step's gradients behind, so the
        # on-demand path stays valid between replays, and the host does not run here on replay anyway.)
        if self.before_zero and not (self.grad.is_cuda and torch.cuda.is_current_stream_capturing()):
            dead = False
            for ref in self.before_zero:           # weak references to the optimizers: a discarded optimizer is not kept alive by its arena
                opt = ref()
                if opt is None:
                    dead = True
                else:
                    opt._materialize_m()
            if dead:
                self.before_zero = tuple(r for r in self.before_zero if r() is not None)
        if self._store_first is not None:
            # the large filter slots are not zeroed: their first contribution of the step is a plain store (first_touch); one launch zeroes
            # the small slots between them
            K.zero_ranges(self.grad, self._small_ranges)
            self._touched = set()
            self._pending_check = True
        else:
            self.grad.zero_()

    before_zero = ()
    _store_first = None
    _pending_check = False

    def enable_sinks(self, store_first=True):
        """Let the filter-gradient GEMMs accumulate directly into this arena (autograd.SINKS).
        store_first: the slots of the large filters (>= 2^16 elements; conv / deconv / dense kernels) are
        never zero-filled — the first contribution a step writes into such a slot is a plain store (accumulate = 0 in the filter-gradient
        epilogue), later ones add.  Saves the fill (116 + 91 MB per wgancls iteration) and the epilogues' read of the slot.  A slot that
        receives NO contribution in a step would keep the previous step's gradient: finish_step() — called by the optimizer before it
        reads the arena — zeroes exactly those."""
        from . import autograd as A
        big = set()
        self._store_first, self._pending_check = None, False          # (a repeated call re-decides)
        if store_first and self.grad.is_cuda:
            big = {n for n, v in self.vars.items() if v.numel() >= (1 << 16) and v.dim() >= 2}
        import weakref
        me = weakref.ref(self)             # (the sink registry must not keep the arena — and through it the parameters — alive)

        def first_touch(name):
            a = me()
            return a._first_touch(name) if a is not None else False
        for n, v in self.vars.items():     # kernels, biases, BN gamma/beta: every gradient is summed in place by its kernel
            A.register_sink(v, self.grad_of(n).view(-1), (lambda name=n: first_touch(name)) if n in big else None)
        if big:
            self._store_first = big
            self._touched = set(big)           # until the first zero_grad every slot holds zeros already: accumulate
            runs, start = [], None
            for n in self.names:               # maximal runs of small slots (padding included), in arena order
                o, k = self.offsets[n]
                end = o + (k + 3) // 4 * 4
                if n in big:
                    if start is not None:
                        runs.append((start, o - start)); start = None
                else:
                    if start is None:
                        start = o
                    last_end = end
            if start is not None:
                runs.append((start, self.numel - start))
            self._small_ranges = torch.tensor(runs if runs else [[0, 0]], dtype=torch.int64, device=self.grad.device).reshape(-1, 2)

    def _first_touch(self, name):
        if name in self._touched:
            return False
        self._touched.add(name)
        return True

    def finish_step(self):
        """Before the optimizer (or a gradient exchange) reads the arena: large slots that received no contribution since zero_grad still
        hold the previous step's gradient — zero them (none on the models here: every filter gets its gradient every step)."""
        if self._store_first is not None and self._pending_check:
            for n in self._store_first - self._touched:
                self.grad_of(n).zero_()
                self._touched.add(n)
            self._pending_check = False

    def grad_of(self, name):
        o, k = self.offsets[name]
        return self.grad[o:o + k].view(self.vars[name].shape)


class SpectralNorm(object):
    """Spectral normalisation of named variables of an arena (Miyato et al., ICLR 2018).  A variable of shape
    [..., C] is the matrix M [R, C], C its last dimension.  The object owns `raw` (the weights the optimizer steps; a clone of
    arena.flat), per variable u [C], v [R] and sigma, and the slot table of csrc/t2i_spectral.hip; arena.flat holds W = raw / sigma
    for the named variables and raw for the others, so every reader of the arena sees normalised weights.
    u is drawn N(0, 1) from `seed` on the CPU and normalised — the same on every data-parallel rank (no rank offset).  Construction
    runs `warmup` power iterations, rewrites arena.flat and drops the cached filter images.
    normalize(iterations) and grad_() wrap the two entries; AdamTF(spectral=...) calls them around its launch.  sync(names) is for a
    restore behind the optimizer's back: raw <- flat for those slots, then `warmup` iterations from the u it has."""

    SUFFIXES = ('raw', 'u', 'v', 'sigma')

    def __init__(self, arena, names, seed=0, warmup=15):
        names = list(names)
        for n in names:
            if n not in arena.offsets:
                raise KeyError('SpectralNorm names %r, which is not a variable of this arena' % (n,))
            if arena.vars[n].dim() < 2:
                raise ValueError('SpectralNorm: %r has shape %s; a normalised variable has at least 2 dimensions' % (n, tuple(arena.vars[n].shape)))
        if len(set(names)) != len(names):
            raise ValueError('SpectralNorm: a variable is named twice')
        if not names:
            raise ValueError('SpectralNorm: no variable named')
        if isinstance(warmup, bool) or not isinstance(warmup, int) or warmup < 0:
            raise ValueError('SpectralNorm: warmup must be an integer >= 0, got %r' % (warmup,))
        self.arena, self.warmup, self.seed = arena, warmup, seed
        self.names = [n for n in arena.names if n in set(names)]          # arena order: the table ascends
        slots = []
        for n in self.names:
            o, k = arena.offsets[n]
            C = int(arena.vars[n].shape[-1])
            slots.append((o, k, k // max(C, 1), C))
        dev = arena.flat.device
        self.table = K.spectral_table(slots, arena.numel, dev)
        self.index = {n: i for i, n in enumerate(self.names)}
        gen = torch.Generator().manual_seed(int(seed))
        u = torch.zeros(self.table.nu, dtype=torch.float32)
        for row in self.table.host:
            C, uo = int(row[2]), int(row[3])
            d = torch.randn(C, generator=gen, dtype=torch.float32)
            u[uo:uo + C] = d / max(float(d.norm()), 1e-12)
        self.u = u.to(dev)
        self.v = torch.zeros(self.table.nv, dtype=torch.float32, device=dev)
        self.sigma = torch.ones(self.table.n_slots, dtype=torch.float32, device=dev)
        self.ws = torch.zeros(self.table.ws_floats, dtype=torch.float32, device=dev)
        self.raw = arena.flat.detach().clone()
        self.normalize(warmup)
        K.filter_cache_invalidate()

    def normalize(self, iterations=1, table=None):
        """`iterations` power iterations on raw, then arena.flat = raw / sigma (named slots) | raw (the others)."""
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 0:
            raise ValueError('SpectralNorm.normalize: iterations must be an integer >= 0, got %r' % (iterations,))
        table = self.table if table is None else table
        while True:
            k = min(iterations, K.SPECTRAL_MAX_ITERATIONS)
            K.spectral_normalize(self.arena.flat, self.raw, table, self.u, self.v, self.sigma, self.ws, iterations=k)
            iterations -= k
            if iterations == 0:
                return

    def grad_(self):
        """arena.grad, in place: dL/dW -> dL/draw inside the named slots, with the u, v, sigma that produced the current arena.flat."""
        K.spectral_grad_(self.arena.grad, self.arena.flat, self.table, self.u, self.v, self.sigma, self.ws)

    def sync(self, names=None):
        """After the arena's variables were written behind the optimizer's back (a restore): raw <- flat for the named slots (None:
        all of them) and for every variable that is not normalised (raw is all the state those have), then `warmup` iterations on the
        named slots from the u they have.  The other normalised slots keep raw, u, v and sigma bit for bit.  With a slot named,
        arena.flat is rewritten and the cached filter images are dropped."""
        names = list(self.names if names is None else names)
        for n in names:
            if n not in self.index:
                raise KeyError('SpectralNorm.sync names %r, which is not normalised here' % (n,))
        with torch.no_grad():
            for n in [n for n in self.arena.names if n not in self.index] + names:
                o, k = self.arena.offsets[n]
                self.raw[o:o + k].copy_(self.arena.flat[o:o + k])
            for n in names:
                self.sigma[self.index[n]] = 1.0
        if not names:
            return
        self.normalize(self.warmup, table=self.table.only([self.index[n] for n in names]))
        K.filter_cache_invalidate()

    def _views(self, n):
        i = self.index[n]
        o, k = self.arena.offsets[n]
        _, R, C, uo, vo = (int(x) for x in self.table.host[i][:5])
        return self.raw[o:o + k].view(self.arena.vars[n].shape), self.u[uo:uo + C], self.v[vo:vo + R], self.sigma[i:i + 1]

    @classmethod
    def keys(cls, name):
        """The four state keys of a variable: `<variable>/spectral_raw`, `_u`, `_v`, `_sigma`."""
        return tuple('%s/spectral_%s' % (name, s) for s in cls.SUFFIXES)

    def state_tensor(self, key):
        """One tensor of state_dict(), copied to the CPU on its own."""
        var, _, tail = key.rpartition('/spectral_')
        if var not in self.index or tail not in self.SUFFIXES:
            raise KeyError('SpectralNorm.state_tensor: %r is not a state key of a variable normalised here' % (key,))
        return self._views(var)[self.SUFFIXES.index(tail)].detach().cpu().clone()

    def state_dict(self):
        """key -> CPU tensor, for every normalised variable its raw weights, u, v and sigma ([1])."""
        out = OrderedDict()
        for n in self.names:
            for key, t in zip(self.keys(n), self._views(n)):
                out[key] = t.detach().cpu().clone()
        return out

    def load_state_dict(self, state):
        """Verbatim: the four tensors of every variable `state` holds are copied in; nothing is launched that changes them, and
        arena.flat is not touched (a checkpoint carries the normalised weights as the variable itself).  A variable with some of its
        four keys missing, or a key of a variable not normalised here, is a KeyError; a wrong shape a ValueError."""
        state = dict(state)
        named = set()
        for key in state:
            var, _, tail = key.rpartition('/spectral_')
            if var not in self.index or tail not in self.SUFFIXES:
                raise KeyError('SpectralNorm.load_state_dict: %r is not a state key of a variable normalised here' % (key,))
            named.add(var)
        with torch.no_grad():
            for n in self.names:
                if n not in named:
                    continue
                for key, t in zip(self.keys(n), self._views(n)):
                    if key not in state:
                        raise KeyError('SpectralNorm.load_state_dict: %s is missing (a variable is restored from all four of its keys)' % key)
                    src = torch.as_tensor(state[key]).to(torch.float32)
                    if src.numel() != t.numel() or (src.dim() > 1 and tuple(src.shape) != tuple(t.shape)):
                        raise ValueError('SpectralNorm.load_state_dict: %s has shape %s, expected %s' % (key, tuple(src.shape), tuple(t.shape)))
                for key, t in zip(self.keys(n), self._views(n)):
                    t.copy_(torch.as_tensor(state[key]).to(torch.float32).reshape(t.shape).to(t.device))


class AdamTF(object):
    """lr_t = lr*sqrt(1-b2^t)/(1-b1^t); m,v updates; w -= lr_t*m/(sqrt(v)+eps) — epsilon OUTSIDE the bias correction
    (SURVEY.md §8a M5).  With beta1=0, t=1 this is ~lr*sign(g).
    ema_decay (default None: no shadow, the plain update): a float in (0, 1) keeps `ema`, tf.train.ExponentialMovingAverage of the
    weights — a flat fp32 buffer of the arena's layout that starts as a copy of the weights (TF initialises a shadow to its
    variable's value) and is advanced by every step, in the update's own launch: ema -= (1 - decay) * (ema - w_new)
    (DESIGN.md section 4.30).
    slot_scales (default None: the plain launches, nothing allocated): a mapping variable name -> c or -> (grad_mult, lr_mult); the
    variable then steps with its gradient times grad_mult and its step size times lr_mult, in one launch over the arena
    (t2i_adam_tf_slots).  Variables not named keep (1, 1).  c for both is the equalized learning rate: Adam on
    w-hat ~ N(0, 1) used as w = c * w-hat, restated on w itself; (1, k) is a per-layer learning-rate multiplier.
    spectral (default None: today's code path and launches): a SpectralNorm over this arena.  apply() then (1) turns the gradients of
    the normalised slots into gradients of the raw weights, in place in arena.grad, (2) runs the same Adam launch on spectral.raw in
    place of arena.flat, (3) advances the power iteration by one step on the new raw and (4) rewrites arena.flat: six launches
    beyond Adam's.  AFTER apply() arena.grad HOLDS THE TRANSFORMED GRADIENT, so the on-demand first moment of
    beta1 == 0 is the moment of raw, the one the step used.  slot_scales combine with it (the multipliers act on the step of raw);
    ema_decay does not (ValueError: critic only)."""

    ema = None
    slot_end = slot_mult = slot_scales = None

    spectral = None

    def __init__(self, arena, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=None, slot_scales=None, spectral=None):
        if spectral is not None:
            if not isinstance(spectral, SpectralNorm) or spectral.arena is not arena:
                raise ValueError('spectral must be None or a SpectralNorm over this optimizer\'s arena, got %r' % (spectral,))
            if ema_decay is not None:
                raise ValueError('spectral and ema_decay do not combine: the moving average is the generator\'s, spectral normalisation the critic\'s')
            self.spectral = spectral
        if ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 < ema_decay < 1.0:
                raise ValueError('ema_decay must be None or a number in (0, 1), got %r' % (ema_decay,))
            ema_decay = float(ema_decay)
        self.arena, self.beta1, self.beta2, self.eps = arena, beta1, beta2, eps
        self.ema_decay = ema_decay
        if slot_scales is not None:
            self._build_slot_tables(slot_scales)
        if ema_decay is not None:
            self.ema = arena.flat.detach().clone()
            self.ema_decay_dev = torch.full((4,), ema_decay, dtype=torch.float32, device=arena.flat.device)   # [0] = the decay
        self._m = torch.zeros_like(arena.flat)
        self.v = torch.zeros_like(arena.flat)
        # beta1 == 0 (both wgancls optimizers, PGGAN): m_t = g_t * grad_scale whatever m_{t-1} was, so the step neither reads nor
        # writes it (4 bytes per parameter less of the 24 the update streams); `m` is formed from the gradient arena when somebody
        # asks for it — a checkpoint between two iterations — which is valid until the arena is zeroed for the next backward
        self.skip_m = beta1 == 0.0
        self._m_stale, self._last_scale = False, 1.0    # `_m` lags the last step (it is re-formed from the gradient arena on demand)
        self.t = 0
        self.lr_t_dev = torch.zeros(4, dtype=torch.float32, device=arena.flat.device)   # [0] = this step's lr_t
        if self.skip_m:
            import weakref
            arena.before_zero = tuple(arena.before_zero) + (weakref.ref(self),)

    def _build_slot_tables(self, slot_scales):
        """The two device tables of t2i_adam_tf_slots, once: slot_end[s] = the padded end of the arena's s-th variable (the next
        variable's offset; the arena's size for the last), slot_mult[s] = (grad_mult, lr_mult)."""
        arena = self.arena
        mults = OrderedDict((n, (1.0, 1.0)) for n in arena.names)
        for name, c in dict(slot_scales).items():
            if name not in mults:
                raise KeyError('slot_scales names %r, which is not a variable of this arena' % (name,))
            pair = tuple(c) if isinstance(c, (tuple, list)) else (c, c)
            if len(pair) != 2:
                raise ValueError('slot_scales[%r] must be a number or (grad_mult, lr_mult), got %r' % (name, c))
            for x in pair:
                if isinstance(x, bool) or not isinstance(x, numbers.Real) or not (math.isfinite(x) and x > 0.0):
                    raise ValueError('slot_scales[%r]: a multiplier must be a finite number > 0, got %r' % (name, x))
            mults[name] = (float(pair[0]), float(pair[1]))
        if len(mults) > K.ADAM_MAX_SLOTS:
            raise ValueError('slot_scales: the arena has %d variables, one launch takes at most %d slots' % (len(mults), K.ADAM_MAX_SLOTS))
        ends = [o + (k + 3) // 4 * 4 for o, k in arena.offsets.values()]
        assert ends[-1] == arena.numel
        dev = arena.flat.device
        self.slot_end = torch.tensor(ends, dtype=torch.int64, device=dev)
        self.slot_mult = torch.tensor([list(p) for p in mults.values()], dtype=torch.float32, device=dev)
        self.slot_scales = mults

    @property
    def m(self):
        """First moment.  With the beta1 == 0 fast path it is (re)built from the gradient arena on access (see __init__): the arena
        holds the last step's gradients until the next zero_grad, and an EAGER Arena.zero_grad forms a stale `m` before it clears
        them (_materialize_m), so a checkpoint taken after a stray zero_grad / backward still holds the last step's moment."""
        if self.skip_m and self._m_stale:
            with torch.no_grad():
                if self.slot_end is None:
                    torch.mul(self.arena.grad, self._last_scale, out=self._m)
                else:          # per slot what the launch would have written: g * fl32(grad_scale * grad_mult_s)
                    import numpy as np
                    start = 0
                    for end, (gm, _) in zip(self.slot_end.tolist(), self.slot_scales.values()):
                        gs = float(np.float32(self._last_scale) * np.float32(gm))
                        torch.mul(self.arena.grad[start:end], gs, out=self._m[start:end])
                        start = end
            self._m_stale = False
        return self._m

    @m.setter
    def m(self, value):
        """Assigning the first moment (a checkpoint restore, a test) keeps the assigned values until the next step."""
        with torch.no_grad():
            self._m.copy_(value)
        self._m_stale = False

    def _materialize_m(self):
        """Arena.zero_grad (eager) is about to clear the gradients the on-demand first moment is formed from."""
        if self.skip_m and self._m_stale:
            self.m

    def moments_loaded(self):
        """The caller has just written m (and t) from a checkpoint: keep those values until the next step."""
        self._m_stale = False

    def prepare(self, lr):
        """Host half of a step: advance t and publish lr_t to the device scalar (outside any captured graph)."""
        self.t += 1
        self._m_stale = self.skip_m          # every step (eager or replayed: this is its host half) leaves `_m` behind
        lr_t = lr * math.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
        self.lr_t_dev.fill_(lr_t)
        return lr_t

    def set_ema_decay(self, decay):
        """Publish a new decay to the device scalar the fused launch reads (a host call outside any captured graph, like prepare)."""
        if self.ema is None:
            raise RuntimeError('this optimizer keeps no moving average (ema_decay=None)')
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay <= 1.0:
            raise ValueError('the decay must be a number in [0, 1], got %r' % (decay,))
        self.ema_decay = float(decay)
        self.ema_decay_dev.fill_(self.ema_decay)

    def sync_ema(self, names=None):
        """ema <- weights for the named slots of the arena (None: every slot): a variable restored or re-initialised behind the
        optimizer's back starts its average from its new value."""
        if self.ema is None:
            raise RuntimeError('this optimizer keeps no moving average (ema_decay=None)')
        with torch.no_grad():
            if names is None:
                self.ema.copy_(self.arena.flat)
                return
            for n in names:
                o, k = self.arena.offsets[n]
                self.ema[o:o + k].copy_(self.arena.flat[o:o + k])

    def apply(self, grad_scale=1.0, refresh=None):
        """Device half: one kernel over the arena, step size read from the device scalar (graph-capturable).
        refresh: regenerate the cached filter images of this arena behind the update, in one launch
        (kernels.filter_cache_refresh).  Default: yes for eager launches; not inside a capture, whose successor graph starts
        with a refresh of everything — pass True where the same capture goes on to use these filters (the critic's update in
        a one-graph iteration)."""
        self.arena.finish_step()
        kw = dict(lr_t=0.0, beta1=self.beta1, beta2=self.beta2, eps=self.eps, grad_scale=grad_scale, lr_t_dev=self.lr_t_dev)
        if self.ema is not None:
            kw.update(ema=self.ema, ema_decay=self.ema_decay, ema_decay_dev=self.ema_decay_dev)
        if self.slot_end is not None:
            kw.update(slot_end=self.slot_end, slot_mult=self.slot_mult)
        launch = K.adam_tf_slots if self.slot_end is not None else K.adam_tf if self.ema is None else K.adam_tf_ema
        if self.spectral is not None:
            # dL/dW -> dL/draw in the gradient arena, Adam on the raw weights, one power iteration on the new raw, arena.flat rewritten
            self.spectral.grad_()
            launch(self.spectral.raw, self.arena.grad, None if self.skip_m else self._m, self.v, **kw)
            self.spectral.normalize(1)
        else:
            launch(self.arena.flat, self.arena.grad, None if self.skip_m else self._m, self.v, **kw)
        if self.skip_m:
            self._last_scale = float(grad_scale)
            self._m_stale = True             # (an eager zero_grad between prepare() and here has formed the PREVIOUS step's moment)
        if refresh is None:
            refresh = self.arena.flat.is_cuda and not torch.cuda.is_current_stream_capturing()
        if refresh and self.arena.flat.is_cuda:
            K.filter_cache_refresh(self.arena.flat)

    def step(self, lr, grad_scale=1.0):
        self.prepare(lr)
        self.apply(grad_scale)


class RMSPropTF(object):
    """tf.train.RMSPropOptimizer(lr, decay=0.9, momentum=0.0, epsilon=1e-10) over an Arena (reference
    models/inception/trainer.py): ms += (g^2 - ms)(1 - decay); mom = momentum * mom + lr g / sqrt(ms + eps); w -= mom, one launch
    (t2i_rmsprop_tf).  The `rms` slot starts at ONES (the TF 1.x initial value), `momentum` at zeros.  Checkpoints keep them under
    TF's slot names `<variable>/RMSProp` and `<variable>/RMSProp_1` (slots / slot_key: utils/saver.py)."""

    def __init__(self, arena, lr=5e-5, decay=0.9, momentum=0.0, eps=1e-10):
        self.arena, self.lr, self.decay, self.momentum, self.eps = arena, lr, decay, momentum, eps
        self.ms = torch.ones_like(arena.flat)
        self.mom = torch.zeros_like(arena.flat)

    def slots(self):
        """slot name -> flat buffer over the arena, in TF's slot order."""
        return OrderedDict([('RMSProp', self.ms), ('RMSProp_1', self.mom)])

    @staticmethod
    def slot_key(oname, var, slot):
        """TF names an optimizer slot after its variable alone (`InceptionV3/Logits/Conv2d_1c_1x1/weights/RMSProp`)."""
        return '%s/%s' % (var, slot)

    def step(self, lr=None):
        """One update of every variable of the arena from its gradient slot; the cached filter images of the arena are dropped."""
        self.arena.finish_step()
        K.rmsprop_tf(self.arena.flat, self.arena.grad, self.ms, self.mom, self.lr if lr is None else lr, self.decay, self.momentum, self.eps)
        if self.arena.flat.is_cuda:
            K.filter_cache_invalidate(self.arena.flat, external=False)
