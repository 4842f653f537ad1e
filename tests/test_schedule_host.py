"""graphs.DGSchedule on the host: the order of calls of the D-then-G iteration — eager, captured and replayed, with and without
data parallelism — against recording fakes for dp, the arenas, the optimizers and the graphs object.  No kernel runs."""
import pytest
import torch


class Arena(object):
    def __init__(self, log, name):
        self.log, self.name = log, name

    def zero_grad(self):
        self.log.append((self.name, 'zero_grad'))


class Optim(object):
    def __init__(self, log, name):
        self.log, self.name = log, name

    def prepare(self, lr):
        self.log.append((self.name, 'prepare', lr))

    def apply(self, grad_scale=1.0, refresh=None):
        self.log.append((self.name, 'apply', grad_scale, refresh))


class DP(object):
    world = 4

    def __init__(self, log):
        self.log = log

    def arm(self, arena):
        self.log.append(('dp', 'arm', arena.name))

    def allreduce_arena(self, arena):
        self.log.append(('dp', 'allreduce', arena.name))
        return {'d_arena': 0.375, 'g_arena': 0.625}[arena.name]      # (distinct, so that the hand-over to apply() shows)


class Graphs(object):
    """StepGraphs' surface: capture runs the body once, replay returns what it returned."""

    def __init__(self, log):
        self.log, self.graphs, self.outs, self.static = log, {}, {}, {'feed': 'static'}

    def load(self, feed):
        self.log.append(('graphs', 'load', feed))

    def capture(self, name, body, capture_error_mode='global', refresh=True):
        self.log.append(('graphs', 'capture', name, capture_error_mode, refresh))
        self.graphs[name] = True
        self.outs[name] = body(self.static)

    def replay(self, name):
        self.log.append(('graphs', 'replay', name))
        return self.outs[name]


def make(dp=False, fail=None):
    """-> (schedule, log).  The two losses run the schedule's backward on a one-element graph whose hook logs the backward itself."""
    import t2i_amd  # noqa: F401
    from t2i_amd.graphs import DGSchedule
    log = []
    arenas = {k: Arena(log, k + '_arena') for k in 'dg'}
    optims = {k: Optim(log, k.upper()) for k in 'dg'}
    sched = []

    def losses(k):
        def f(feed, **kw):
            log.append((k + '_losses', feed, sched[0].capturing, kw))
            if fail == k:
                raise RuntimeError('the body failed')
            w = torch.ones(1, requires_grad=True)
            w.register_hook(lambda g: log.append((k, 'backward', float(g))))
            sched[0].backward(arenas[k], [w * 3.0], [torch.ones(1)], [w])
            return k + '_out'
        return f
    sched.append(DGSchedule(DP(log) if dp else None, losses('d'), arenas['d'], optims['d'], losses('g'), arenas['g'], optims['g']))
    return sched[0], log


def half(k, feed, capturing=False, armed=False, kw=None):
    """What one losses(feed) logs: the call, zero_grad, [arm], the backward."""
    return ([(k + '_losses', feed, capturing, kw or {}), (k + '_arena', 'zero_grad')] + ([('dp', 'arm', k + '_arena')] if armed else [])
            + [(k, 'backward', 3.0)])


def test_eager_without_dp():
    s, log = make()
    assert s.capturing is False
    assert s.run('feed', 1e-3, 2e-3) == {'d': 'd_out', 'g': 'g_out'}
    assert log == ([('D', 'prepare', 1e-3)] + half('d', 'feed') + [('D', 'apply', 1.0, None)]
                   + [('G', 'prepare', 2e-3)] + half('g', 'feed') + [('G', 'apply', 1.0, None)])


def test_eager_joint_body_prepares_both_first():
    s, log = make()

    def joint(feed):
        log.append(('joint', feed))
        return s.step(s.d, feed, refresh=True, keep=1), s.step(s.g, feed)
    assert s.run('feed', 1e-3, 2e-3, joint=joint) == {'d': 'd_out', 'g': 'g_out'}
    assert log == ([('D', 'prepare', 1e-3), ('G', 'prepare', 2e-3), ('joint', 'feed')] + half('d', 'feed', kw={'keep': 1}) + [('D', 'apply', 1.0, True)]
                   + half('g', 'feed') + [('G', 'apply', 1.0, None)])


def test_eager_with_dp_arms_before_the_backward_and_hands_the_scale_over():
    s, log = make(dp=True)
    s.run('feed', 1e-3, 1e-3)
    assert log == ([('D', 'prepare', 1e-3)] + half('d', 'feed', armed=True) + [('dp', 'allreduce', 'd_arena'), ('D', 'apply', 0.375, None)]
                   + [('G', 'prepare', 1e-3)] + half('g', 'feed', armed=True) + [('dp', 'allreduce', 'g_arena'), ('G', 'apply', 0.625, None)])
    assert sum(1 for e in log if e[:2] == ('dp', 'arm')) == 2


def test_capture_without_dp():
    s, log = make()
    g = Graphs(log)
    s.capture(g)
    assert [e[2:] for e in log if e[:2] == ('graphs', 'capture')] == [('d', 'global', True), ('g', 'global', True)]
    assert ('D', 'apply', 1.0, None) in log and ('G', 'apply', 1.0, None) in log
    s2, log2 = make()
    g2 = Graphs(log2)
    s2.capture(g2, joint=lambda f: (s2.step(s2.d, f), s2.step(s2.g, f)))
    assert list(g2.graphs) == ['dg'] and g2.outs['dg'] == ('d_out', 'g_out')
    del log2[:]
    assert s2.run('feed', 1e-3, 2e-3, graphs=g2) == {'d': 'd_out', 'g': 'g_out'}
    assert log2 == [('graphs', 'load', 'feed'), ('D', 'prepare', 1e-3), ('G', 'prepare', 2e-3), ('graphs', 'replay', 'dg')]


def test_capture_with_dp_cuts_each_half_at_its_exchange():
    s, log = make(dp=True)
    g = Graphs(log)
    s.capture(g)
    assert [e[2:] for e in log if e[:2] == ('graphs', 'capture')] == [
        ('d', 'thread_local', True), ('d_upd', 'thread_local', False), ('g', 'thread_local', True), ('g_upd', 'thread_local', False)]
    assert not [e for e in log if e[0] == 'dp']                                   # never armed, nothing exchanged inside a capture
    assert [e[2] for e in log if e[0] in ('d_losses', 'g_losses')] == [True, True]           # the flag inside each body ...
    assert s.capturing is False                                                   # ... and afterwards
    assert [e for e in log if e[1] == 'apply'] == [('D', 'apply', 0.25, None), ('G', 'apply', 0.25, None)]      # 1 / world, baked in
    assert log == ([('graphs', 'capture', 'd', 'thread_local', True)] + half('d', g.static, capturing=True)
                   + [('graphs', 'capture', 'd_upd', 'thread_local', False), ('D', 'apply', 0.25, None)]
                   + [('graphs', 'capture', 'g', 'thread_local', True)] + half('g', g.static, capturing=True)
                   + [('graphs', 'capture', 'g_upd', 'thread_local', False), ('G', 'apply', 0.25, None)])


@pytest.mark.parametrize('fail', ['d', 'g'])
def test_capture_clears_the_flag_when_a_body_raises(fail):
    s, log = make(dp=True, fail=fail)
    with pytest.raises(RuntimeError, match='the body failed'):
        s.capture(Graphs(log))
    assert [e[2] for e in log if e[0] == fail + '_losses'] == [True]
    assert s.capturing is False


def test_replay_with_dp_exchanges_between_the_segments():
    s, log = make(dp=True)
    g = Graphs(log)
    s.capture(g)
    del log[:]
    assert s.run('feed', 1e-3, 2e-3, graphs=g) == {'d': 'd_out', 'g': 'g_out'}
    assert log == [('graphs', 'load', 'feed'),
                   ('D', 'prepare', 1e-3), ('graphs', 'replay', 'd'), ('dp', 'allreduce', 'd_arena'), ('graphs', 'replay', 'd_upd'),
                   ('G', 'prepare', 2e-3), ('graphs', 'replay', 'g'), ('dp', 'allreduce', 'g_arena'), ('graphs', 'replay', 'g_upd')]


def test_a_model_that_keeps_its_schedule_is_freed_with_its_last_reference():
    """A model builds the schedule from its own bound methods and keeps it.  That must not close a reference cycle: a model left
    to the cyclic collector is freed at an arbitrary moment — inside a later capture, where destroying its graphs aborts."""
    import gc
    import weakref
    import t2i_amd  # noqa: F401
    from t2i_amd.graphs import DGSchedule

    class Model(object):
        def __init__(self):
            log = []
            self.schedule = DGSchedule(None, self.d_losses, Arena(log, 'd_arena'), Optim(log, 'D'), self.g_losses, Arena(log, 'g_arena'), Optim(log, 'G'))

        def d_losses(self, feed):
            return 'd_out'

        def g_losses(self, feed):
            return 'g_out'
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        m = Model()
        assert m.schedule.run('feed', 1e-3, 1e-3) == {'d': 'd_out', 'g': 'g_out'}
        r = weakref.ref(m)
        del m
        assert r() is None
    finally:
        if was_enabled:
            gc.enable()


def test_replay_without_dp():
    s, log = make()
    g = Graphs(log)
    s.capture(g)
    del log[:]
    s.run('feed', 1e-3, 2e-3, graphs=g)
    assert log == [('graphs', 'load', 'feed'), ('D', 'prepare', 1e-3), ('graphs', 'replay', 'd'), ('G', 'prepare', 2e-3), ('graphs', 'replay', 'g')]
