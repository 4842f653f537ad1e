"""hipGraph capture of training-step bodies (HIP graphs instead of a tracing compiler).

A step body is a function of a dict of device tensors that issues only device work (kernels of libt2i_hip.so, the
Adam launch with its step size in device memory, tensor-library scalar math) — no host synchronisation, no allocation
that survives the call, no host-side random draws.  `StepGraphs` keeps one set of static input buffers, captures each
body once and replays it: at the reference's batch sizes (8 or 16) a GAN iteration is ~1000 launches of a few
microseconds each and is bound by the host's launch rate, not by the GPU.  Replay is bit-identical to the eager
launches (same kernels, same order).  `DGSchedule` is the D-then-G iteration those bodies make up, eager or replayed."""
import collections
import inspect
import weakref

import torch

from . import autograd as A
from . import kernels as K


def capture_mode(requested='global'):
    """The capture_error_mode a capture in this process should use.  As soon as a process group exists, its watchdog thread
    polls events on the HIP runtime at any time; in 'global' mode such a call from another thread while a capture is open is an
    error that tears the process down (seen once in the full GPU suite: a single-GPU capture after a data-parallel test in the same
    process).  'thread_local' confines the checks to the capturing thread, which is all these captures need."""
    if requested == 'global':
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                return 'thread_local'
        except Exception:          # noqa: BLE001 — a build without torch.distributed has no watchdog either
            pass
    return requested


class StepGraphs(object):
    def __init__(self, example_feed, keys, filters=()):
        """example_feed: name -> device tensor (shapes/dtypes of every later feed); keys: the entries the bodies read;
        filters: the tensors holding the convolution filters the bodies use (the optimizer arenas) — see capture(refresh=)."""
        self.filters = list(filters)
        self.static = {k: example_feed[k].clone() for k in keys if example_feed.get(k) is not None}
        self.graphs, self.outs, self._pool = {}, {}, None

    def load(self, feed):
        """Copy this iteration's inputs into the static buffers (device-to-device, outside the graphs)."""
        for k, buf in self.static.items():
            v = feed.get(k)
            if v is not None and v is not buf:
                buf.copy_(v, non_blocking=True)

    def capture(self, name, body, capture_error_mode='global', refresh=True):
        """body(static_feed) -> anything holding device tensors (kept alive and returned by replay).
        capture_error_mode='thread_local' when another thread touches the HIP runtime during the capture (the process
        group's watchdog under data parallelism).  refresh: start the graph with ONE batched regeneration of every cached filter
        image (kernels.filter_cache_refresh) — a graph must contain every transform it depends on, and filled lazily they are
        one small launch per filter; pass False for a segment that runs no convolution."""
        dev = next(iter(self.static.values())).device
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._pool, capture_error_mode=capture_mode(capture_error_mode)):
            if refresh:
                for t in self.filters:               # one batched launch per arena; the convs of this graph then find every
                    K.filter_cache_refresh(t)        # known image of these filters filled
            out = body(self.static)
        if self._pool is None:
            self._pool = g.pool()
        self.graphs[name], self.outs[name] = g, out
        return out

    def replay(self, name):
        self.graphs[name].replay()
        K.filter_cache_invalidate()                  # a replayed optimizer step rewrote filters behind the host's back
        return self.outs[name]


Half = collections.namedtuple('Half', 'losses arena optim')


def _unowned(f):
    """f, with a bound method held through a weak reference to its object.  The model owns its schedule; a strong reference back
    would close a cycle, and the model, its arenas and its captured graphs would then be freed by the cyclic collector at some
    later allocation instead of with their last reference — for instance inside another model's capture, where destroying a
    graph is an error that aborts the process."""
    if not inspect.ismethod(f):
        return f
    ref = weakref.WeakMethod(f)
    return lambda *a, **kw: ref()(*a, **kw)


class DGSchedule(object):
    """The step schedule of models/gancls, models/stackgan and models/pggan (models/wgancls keeps its own: kt, the cut backward):

        D half:  losses(feed) -> zero_grad -> [dp.arm] -> backward -> side_join | exchange | Adam
        G half:  the same on the generator's arena

    eager (step), captured whole, or — under data parallelism — captured and cut at the exchange: graphs 'd' | all-reduce of the
    gradient arena, issued eagerly | 'd_upd', then 'g' | all-reduce | 'g_upd': no collective is ever captured.  The model's
    losses(feed) end in self.backward(...); what a model draws or sets before a step is the model's business, before run()."""

    def __init__(self, dp, d_losses, d_arena, d_optim, g_losses, g_arena, g_optim):
        self.dp = dp                                 # a dp.DataParallel or None
        self.d, self.g = Half(_unowned(d_losses), d_arena, d_optim), Half(_unowned(g_losses), g_arena, g_optim)
        self.capturing = False                       # inside capture(): the exchanges are issued between the segments, not by armed hooks

    def backward(self, arena, roots, seeds, variables):
        """Gradients of `roots` (seeded by `seeds`, or None for scalar roots) with respect to `variables` -> arena."""
        arena.zero_grad()
        if self.dp is not None and not self.capturing:
            self.dp.arm(arena)                       # the bucketed all-reduce overlaps the rest of this backward
        torch.autograd.backward(roots, seeds, inputs=list(variables))
        A.side_join()

    def step(self, half, feed, refresh=None, **kw):
        """One eager half (self.d or self.g), graph-capturable without dp: Adam reads its step size from device memory."""
        out = half.losses(feed, **kw)
        scale = self.dp.allreduce_arena(half.arena) if self.dp is not None else 1.0
        half.optim.apply(grad_scale=scale, refresh=refresh)
        return out

    def capture(self, graphs, joint=None, g_forms=None):
        """Capture the iteration into `graphs` (a StepGraphs; call after one eager iteration).  Single process: 'dg' from `joint`, a
        body of both halves, if one is given, else 'd' and 'g'.  Data parallelism: the four cut segments, in thread-local capture
        mode because the process group's watchdog thread polls events meanwhile; the update segments run no convolution.
        g_forms (single process, no joint body): {graph name: keywords of the generator's losses} when the generator half has more than
        one form (PGGAN's path-length step); run(g_form=) says which one an iteration replays.  None: the one form 'g'."""
        if g_forms is not None and (self.dp is not None or joint is not None):
            raise ValueError('g_forms: several forms of the generator half are captured in a single process and without a joint body only')
        if self.dp is None:
            if joint is not None:
                graphs.capture('dg', joint)
            else:
                graphs.capture('d', lambda f: self.step(self.d, f))
                for name, kw in ({'g': {}} if g_forms is None else g_forms).items():
                    graphs.capture(name, lambda f, kw=kw: self.step(self.g, f, **kw))
            return
        scale = 1.0 / self.dp.world
        self.capturing = True
        try:
            graphs.capture('d', self.d.losses, capture_error_mode='thread_local')
            graphs.capture('d_upd', lambda f: self.d.optim.apply(grad_scale=scale), capture_error_mode='thread_local', refresh=False)
            graphs.capture('g', self.g.losses, capture_error_mode='thread_local')
            graphs.capture('g_upd', lambda f: self.g.optim.apply(grad_scale=scale), capture_error_mode='thread_local', refresh=False)
        finally:
            self.capturing = False

    def run(self, feed, lr_d, lr_g, graphs=None, joint=None, g_form=None):
        """One iteration -> {'d': ..., 'g': ...}: replayed from `graphs` if given, else eager (from `joint` if given).  prepare(lr)
        publishes each step size on the host, outside any graph: both up front for a one-body iteration, else before its half.
        g_form: (graph name, keywords of the generator's losses) of the form of the generator half this iteration takes (capture's
        g_forms); None: 'g' and no keywords."""
        g_name, g_kw = ('g', {}) if g_form is None else g_form
        if graphs is not None:
            graphs.load(feed)
        one_body = 'dg' in graphs.graphs if graphs is not None else joint is not None
        if one_body:
            self.d.optim.prepare(lr_d)
            self.g.optim.prepare(lr_g)
            d, g = joint(feed) if graphs is None else graphs.replay('dg')
            return {'d': d, 'g': g}
        out = {}
        for name, half, lr in (('d', self.d, lr_d), ('g', self.g, lr_g)):
            half.optim.prepare(lr)
            if graphs is None:
                out[name] = self.step(half, feed, **(g_kw if name == 'g' else {}))
                continue
            out[name] = graphs.replay(g_name if name == 'g' else name)
            if self.dp is not None:
                self.dp.allreduce_arena(half.arena)
                graphs.replay(name + '_upd')
        return out
