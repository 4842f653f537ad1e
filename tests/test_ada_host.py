"""The device-side parameter draw and the controller of p without a GPU: known answers of the Philox
restatement, the laws of the restated table and of the restated controller (tests/ada_cases.py), the two exports in header and binding
within ABI v13, every refusal of the entry points (host pointers: a call that passed validation would launch on them), of
DiffAugmentSampler, of PGGAN's new arguments and of the trainer's new flags."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import ada_cases as AC  # noqa: E402

NEW_EXPORTS = ('t2i_diff_augment_draw', 't2i_diffaug_observe')


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counter,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(counter, key, want):
    got = AC.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert ' '.join('%08x' % int(v) for v in got) == want


@pytest.mark.parametrize('H,W', AC.SIZES)
def test_laws_of_the_restated_table(H, W):
    n = 4096
    ident = np.array(AC.IDENTITY_ROW, np.float32)
    P, after = AC.draw(AC.make_state(seed=7, p=0.5, counter=3), n, H, W, 7)
    on = AC.gates(AC.make_state(seed=7, p=0.5, counter=3), n)
    assert P.dtype == np.float32 and P.shape == (n, 9) and AC.counter_of(after) == 4 and np.array_equal(after[4:], AC.make_state(7, 0.5)[4:])
    assert ((on.mean(0) > 0.4) & (on.mean(0) < 0.6)).all()
    col, tr, cut = on[:, 0], on[:, 1], on[:, 2]
    # gated off: the identity columns
    assert np.array_equal(P[~col, :3], np.tile(ident[:3], ((~col).sum(), 1)))
    assert not P[~tr, 3:5].any() and not P[~cut, 5:].any()
    # colour ranges, with most of each range reached
    b, s, c = P[col, 0], P[col, 1], P[col, 2]
    assert b.min() >= -0.5 and b.max() < 0.5 and b.min() < -0.45 and b.max() > 0.45
    assert s.min() >= 0.0 and s.max() < 2.0 and s.min() < 0.1 and s.max() > 1.9
    assert c.min() >= 0.5 and c.max() < 1.5 and c.min() < 0.55 and c.max() > 1.45
    assert np.array_equal(P[:, 3:], np.round(P[:, 3:]))
    for j, size in ((3, H), (4, W)):
        r = int(size / 8.0 + 0.5)
        assert sorted(set(P[tr, j].tolist())) == [float(v) for v in range(-r, r + 1)]             # |t| <= r, both ends (and all between) reached
    for j, size in ((5, H), (7, W)):
        ext = int(size / 2.0 + 0.5)
        lo, hi = P[cut, j], P[cut, j + 1]
        assert (lo >= 0).all() and (hi <= size).all() and (hi > lo).all()                          # clipped, never empty when applied
        assert int((hi - lo).max()) == ext and int((hi - lo).min()) == ext - ext // 2
        assert lo.min() == 0 and hi.max() == size
    # a policy that is absent keeps its identity columns whatever the gates say, and p = 0 / p = 1 never / always apply
    for mask, cols in ((AC.COLOR, (0, 1, 2)), (AC.TRANSLATION, (3, 4)), (AC.CUTOUT, (5, 6, 7, 8))):
        Q, _ = AC.draw(AC.make_state(seed=7, p=1.0, counter=3), n, H, W, mask)
        rest = [j for j in range(9) if j not in cols]
        assert np.array_equal(Q[:, rest], np.tile(ident[rest], (n, 1)))
        R, _ = AC.draw(AC.make_state(seed=7, p=0.5, counter=3), n, H, W, mask)
        assert np.array_equal(R[:, cols], P[:, cols])                                               # a block does not depend on the other policies
    assert np.array_equal(AC.draw(AC.make_state(7, 0.0, 3), n, H, W, 7)[0], np.tile(ident, (n, 1)))
    assert AC.gates(AC.make_state(7, 1.0, 3), n).all()


def test_the_stream_depends_on_seed_call_and_row_alone():
    a, s1 = AC.draw(AC.make_state(5, 1.0), 64, 16, 16, 7)
    b, _ = AC.draw(s1, 64, 16, 16, 7)
    assert not np.array_equal(a, b)
    assert np.array_equal(AC.draw(AC.make_state(5, 1.0, 1), 64, 16, 16, 7)[0], b)
    assert np.array_equal(AC.draw(AC.make_state(5, 1.0), 16, 16, 16, 7)[0], a[:16])               # row i does not depend on n
    assert not np.array_equal(AC.draw(AC.make_state(6, 1.0), 64, 16, 16, 7)[0], a)
    assert not np.array_equal(AC.draw(AC.make_state(5 + (1 << 32), 1.0), 64, 16, 16, 7)[0], a)     # the seed's high word is used
    assert not np.array_equal(AC.draw(AC.make_state(5, 1.0, 1 << 32), 64, 16, 16, 7)[0], a)        # and the counter's
    _, s = AC.draw(AC.make_state(5, 1.0, 0xffffffff), 4, 16, 16, 7)
    assert (int(s[2]), int(s[3])) == (0, 1)                                                         # the carry
    _, s = AC.draw(AC.make_state(5, 1.0, (1 << 64) - 1), 4, 16, 16, 7)
    assert (int(s[2]), int(s[3])) == (0, 0)


@pytest.mark.parametrize('seed', [0, 1, 1234])
@pytest.mark.parametrize('call', [0, 1])
def test_gate_fractions(seed, call):
    """each gate is Bernoulli(0.3) over 65536 rows: sigma = sqrt(0.3 * 0.7 / 65536) = 0.00179; the three fractions lie within 3 sigma"""
    n = 65536
    frac = AC.gates(AC.make_state(seed, 0.3, call), n).mean(0)
    sigma = math.sqrt(0.3 * 0.7 / n)
    print('seed %d call %d: %s sigma' % (seed, call, ((frac - 0.3) / sigma).round(2)))
    assert (np.abs(frac - 0.3) <= 3 * sigma).all()


def test_the_restated_controller():
    f = np.float32
    real_hi, real_lo = np.full(8, 2.0, f), np.full(8, -2.0, f)
    fake = np.zeros(8, f)
    s = AC.make_state(1, 0.25, counter=9)
    # the adjustment runs only on the interval-th call
    s1 = AC.observe(s, real_hi, None, AC.LOGIT, 0.6, 2, 64.0)
    assert AC.f32_of(s1[4]) == f(0.25) and AC.f32_of(s1[5]) == 8 and AC.f32_of(s1[6]) == 8 and s1[7] == 1 and s1[9] == 0 and AC.f32_of(s1[8]) == 0
    s2 = AC.observe(s1, real_hi, None, AC.LOGIT, 0.6, 2, 64.0)
    assert AC.f32_of(s2[4]) == f(0.5) and AC.f32_of(s2[8]) == 1.0 and s2[9] == 1 and not s2[5:8].any()            # r = 1 > 0.6: + 16 / 64
    assert np.array_equal(s2[:4], s[:4]) and not s2[10:].any()
    # r < target: p falls
    s3 = AC.observe(AC.observe(s2, real_lo, None, AC.LOGIT, 0.6, 2, 64.0), real_lo, None, AC.LOGIT, 0.6, 2, 64.0)
    assert AC.f32_of(s3[4]) == f(0.25) and AC.f32_of(s3[8]) == -1.0 and s3[9] == 2
    # r == target: p holds (6 of 8 above, 2 below: r = 0.5)
    half = np.array([1, 1, 1, 1, 1, 1, -1, -1], f)
    s4 = AC.observe(s3, half, None, AC.LOGIT, 0.5, 1, 64.0)
    assert AC.f32_of(s4[4]) == f(0.25) and AC.f32_of(s4[8]) == f(0.5) and s4[9] == 3
    # sign(0) = 0
    s5 = AC.observe(s4, np.array([0, 0, 1, -1], f), None, AC.LOGIT, 0.5, 2, 64.0)
    assert AC.f32_of(s5[5]) == 0 and AC.f32_of(s5[6]) == 4
    # the clamps
    lo = AC.observe(AC.make_state(1, 0.1), real_lo, None, AC.LOGIT, 0.6, 1, 16.0)
    hi = AC.observe(AC.make_state(1, 0.9), real_hi, None, AC.LOGIT, 0.6, 1, 16.0)
    assert AC.f32_of(lo[4]) == 0.0 and AC.f32_of(hi[4]) == 1.0
    # MIDPOINT: the threshold is the midpoint of the batch means, so a constant added to every logit changes nothing
    dr, df = AC.logits(65, 3, AC.MIDPOINT, shift=0.5)
    a = AC.observe(AC.make_state(), dr, df, AC.MIDPOINT, 0.6, 1, 1000.0)
    b = AC.observe(AC.make_state(), dr + f(64.0), df + f(64.0), AC.MIDPOINT, 0.6, 1, 1000.0)
    assert np.array_equal(a, b) and 0 < AC.f32_of(a[8]) < 1
    assert AC.theta_of(dr, df, AC.LOGIT) == 0.0 and AC.margin(dr, df, AC.MIDPOINT) > 1e-3


# ---- exports and refusals ------------------------------------------------------------------------------------------------------------
def test_the_two_exports_are_declared_and_the_abi_version_stays():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    from t2i_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 't2i_hip.h')).read()
    declared = set(re.findall(r'\b(t2i_[a-z0-9_]+)\s*\(', header))
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.lib.t2i_version() == 13 and _lib.ABI_VERSION == 13
    assert 't2i_diffaug_state' in header and re.search(r'T2I_ADA_LOGIT = 0, T2I_ADA_MIDPOINT = 1', header)
    assert (K.ADA_LOGIT, K.ADA_MIDPOINT) == (AC.LOGIT, AC.MIDPOINT)


def _host_buffers():
    state = (ctypes.c_uint32 * 32)()
    base = ctypes.addressof(state)
    base += (-base) % 16                                        # a 16-byte aligned host address inside the buffer
    table = (ctypes.c_float * 64)()
    logits = (ctypes.c_float * 64)()
    return (state, table, logits), ctypes.c_void_p(base), ctypes.cast(table, ctypes.c_void_p), ctypes.cast(logits, ctypes.c_void_p)


def test_the_draw_entry_refuses_bad_arguments_on_the_host():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    L = _lib.lib
    keep, st, tab, _ = _host_buffers()
    draw = lambda state=st, n=4, H=8, W=8, policy=7, out=tab: L.t2i_diff_augment_draw(state, n, H, W, policy, out, None)
    bad = [dict(state=None), dict(out=None), dict(state=ctypes.c_void_p(st.value + 4)), dict(state=ctypes.c_void_p(st.value + 8)),
           dict(out=ctypes.c_void_p(tab.value + 2)), dict(n=0), dict(n=-1), dict(n=65536), dict(H=0), dict(W=0), dict(H=32769), dict(W=32769),
           dict(policy=0), dict(policy=8), dict(policy=15), dict(policy=-1)]
    for kw in bad:
        assert draw(**kw) == -1, kw
        assert b't2i_diff_augment_draw' in L.t2i_last_error()
    assert not any(keep[0]) and not any(keep[1])                # nothing was written


def test_the_observe_entry_refuses_bad_arguments_on_the_host():
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    L = _lib.lib
    keep, st, _, lg = _host_buffers()

    def obs(state=st, d_real=lg, d_fake=lg, n=8, mode=AC.MIDPOINT, target=0.6, interval=4, ramp=500000.0):
        return L.t2i_diffaug_observe(state, d_real, d_fake, n, mode, target, interval, ramp, None)
    bad = [dict(state=None), dict(d_real=None), dict(d_fake=None), dict(d_real=None, mode=AC.LOGIT), dict(state=ctypes.c_void_p(st.value + 4)),
           dict(d_real=ctypes.c_void_p(lg.value + 2)), dict(n=0), dict(n=65536), dict(mode=2), dict(mode=-1), dict(interval=0), dict(interval=-3),
           dict(ramp=0.0), dict(ramp=-1.0), dict(ramp=float('inf')), dict(ramp=float('nan')), dict(target=1.0), dict(target=-1.0),
           dict(target=float('nan')), dict(target=2.5)]
    for kw in bad:
        assert obs(**kw) == -1, kw
        assert b't2i_diffaug_observe' in L.t2i_last_error()
    assert not any(keep[0])


def test_the_sampler_refuses_before_any_launch():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils.ops import DiffAugmentSampler as S
    for p in (-0.1, 1.5, float('nan'), '0.5', None, True):
        with pytest.raises(ValueError, match='DiffAugmentSampler.*p must'):
            S('color', p=p, device='cpu')
    for policy in ('colour', '', 'color,', 7, None):
        with pytest.raises(ValueError, match='DiffAugmentSampler.*policy'):
            S(policy, device='cpu')
    for adapt in ('ada', True, 0, 'LOGIT'):
        with pytest.raises(ValueError, match='DiffAugmentSampler.*adapt'):
            S('color', adapt=adapt, device='cpu')
    for kw in (dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5), dict(interval=0), dict(interval=2.0), dict(target=1.0), dict(target=float('nan')),
               dict(ramp_images=0), dict(ramp_images=float('inf'))):
        with pytest.raises(ValueError, match='DiffAugmentSampler'):
            S('color', device='cpu', **kw)
    s = S('color,cutout', p=0.25, seed=(3 << 32) | 9, device='cpu', adapt='midpoint')
    assert (s.target, s.interval, s.ramp_images) == (0.6, 4, 500000.0)                                # the publication's
    assert np.array_equal(s.state_dict(), AC.make_state((3 << 32) | 9, 0.25)) and s.state_dict().dtype == np.int64
    assert s.p == 0.25 and s.last_r == 0.0 and s.updates == 0 and s.counter == 0 and s.mask == 5
    for out in (torch.zeros(4, 8), torch.zeros(3, 9), torch.zeros(4, 9, dtype=torch.float64), torch.zeros(9, 4).t(), [0.0] * 36):
        with pytest.raises(ValueError, match='DiffAugmentSampler.draw.*out'):
            s.draw(4, 8, 8, out=out)
    for shape in ((0, 8, 8), (65536, 8, 8), (4, 0, 8), (4, 8, 32769)):
        with pytest.raises(ValueError, match='DiffAugmentSampler.draw'):
            s.draw(*shape)
    d = torch.zeros(8)
    for bad in (d.double(), d.reshape(2, 4), torch.zeros(16)[::2], [0.0] * 8, torch.zeros(0)):
        with pytest.raises(ValueError, match='DiffAugmentSampler.observe.*d_real'):
            s.observe(bad, d)
        with pytest.raises(ValueError, match='DiffAugmentSampler.observe.*d_fake'):
            s.observe(d, bad)
    with pytest.raises(ValueError, match='DiffAugmentSampler.observe'):
        s.observe(d)                                                                                   # 'midpoint' needs d_fake
    with pytest.raises(ValueError, match='DiffAugmentSampler.observe'):
        s.observe(d, torch.zeros(4))
    with pytest.raises(RuntimeError, match='no CPU path'):                                             # accepted calls have no fallback
        s.draw(4, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        s.observe(d, d)
    S('color', device='cpu').observe('anything')                                                       # adapt=None: nothing happens
    assert np.array_equal(s.state_dict(), AC.make_state((3 << 32) | 9, 0.25))
    # the words round-trip, and a bad array is refused
    words = AC.make_state(77, 0.5, counter=(1 << 32) + 5)
    words[5:10] = [AC.word_of(-3.0), AC.word_of(12.0), 3, AC.word_of(0.25), 0xffffffff]
    s.load_state_dict(words)
    assert np.array_equal(s.state_dict(), words) and s.counter == (1 << 32) + 5 and s.updates == 0xffffffff and s.last_r == 0.25
    for bad in (words[:15], words.astype(np.float64), np.full(16, -1), np.full(16, 1 << 32)):
        with pytest.raises(ValueError, match='load_state_dict'):
            s.load_state_dict(bad)


def _pggan(**kw):
    from t2i_amd.models.pggan.pggan import PGGAN
    return PGGAN(2, 100, None, None, None, None, None, 2, False, device='cpu', build_model=False, **kw)


def test_pggan_validates_the_new_arguments():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils.ops import DiffAugmentSampler as S
    for kw in (dict(diffaug_p=0.5), dict(diffaug_adapt=True), dict(diffaug_sampler=S('color', device='cpu'))):
        with pytest.raises(ValueError, match='diffaug'):
            _pggan(**kw)                                                                               # they need diffaug
    for p in (-0.5, 1.01, float('nan'), '1', True):
        with pytest.raises(ValueError, match='diffaug_p'):
            _pggan(diffaug='color', diffaug_p=p)
    for a in (1, 'midpoint', None):
        with pytest.raises(ValueError, match='diffaug_adapt'):
            _pggan(diffaug='color', diffaug_adapt=a)
    with pytest.raises(ValueError, match='diffaug_sampler'):
        _pggan(diffaug='color', diffaug_sampler='sampler')
    with pytest.raises(ValueError, match='diffaug_sampler'):
        _pggan(diffaug='color', diffaug_sampler=S('cutout', device='cpu'))                             # another policy
    with pytest.raises(ValueError, match='diffaug_adapt'):
        _pggan(diffaug='color', diffaug_adapt=True, diffaug_sampler=S('color', device='cpu'))          # a sampler that cannot adapt
    m = _pggan(diffaug='color')
    assert m.aug_sampler is None and m.diffaug_p is None and m.diffaug_adapt is False
    m = _pggan(diffaug='color', diffaug_p=0.5, seed=11)
    assert m.aug_sampler.p == 0.5 and m.aug_sampler.adapt is None and np.array_equal(m.aug_sampler.state_dict(), AC.make_state(11, 0.5))
    m = _pggan(diffaug='color', diffaug_adapt=True)
    assert m.aug_sampler.p == 0.0 and m.aug_sampler.adapt == 'midpoint'                                # the publication starts from 0
    own = S('translation,color', p=0.3, device='cpu', adapt='midpoint')
    assert _pggan(diffaug='color,translation', diffaug_adapt=True, diffaug_sampler=own).aug_sampler is own


def test_summaries_gain_the_two_scalars_only_with_a_sampler():
    import t2i_amd  # noqa: F401
    from t2i_amd.utils import summary as SM

    class Writer(object):
        def add_summary(self, vals, idx):
            self.vals = vals

        def flush(self):
            pass
    one = torch.tensor(1.0)
    d = dict({k: one for k in ('D_loss_real', 'D_loss_fake', 'real_gp', 'D_loss', 'reg_loss', 'wdist', 'wdist2', 'D_loss_mismatch', 'real_gp2')},
             aug_p=torch.tensor(0.25))
    out = {'d': d, 'g': {'G': torch.zeros(2, 8, 8, 3), 'D_loss_fake': one, 'G_kl_loss': one, 'G_loss': one}}
    feed = {'x': torch.zeros(2, 8, 8, 3), 'z': torch.zeros(2, 8)}
    got = {}
    for name, kw in (('plain', dict(diffaug='color')), ('sampler', dict(diffaug='color', diffaug_p=0.25))):
        m = _pggan(**kw)
        m.writer = Writer()
        m.write_summaries(20, feed, out)
        got[name] = m.writer.vals
    extra = [SM.scalar('aug_p', 0.25), SM.scalar('aug_r', 0.0)]
    assert got['sampler'] == got['plain'] + extra and not any(v in got['plain'] for v in extra)


@pytest.mark.parametrize('argv,word', [
    (['--diffaug-p', '0.5'], '--diffaug'), (['--diffaug-adapt'], '--diffaug'),
    (['--diffaug', 'color', '--diffaug-p', '1.5'], '--diffaug-p'), (['--diffaug', 'color', '--diffaug-p', '-0.1'], '--diffaug-p'),
    (['--diffaug', 'color', '--diffaug-p', 'nan'], '--diffaug-p'),
    (['--diffaug', 'color', '--diffaug-adapt', '--diffaug-target', '1.0'], '--diffaug-target'),
    (['--diffaug', 'color', '--diffaug-adapt', '--diffaug-interval', '0'], '--diffaug-interval'),
    (['--diffaug', 'color', '--diffaug-adapt', '--diffaug-ramp', '0'], '--diffaug-ramp'),
    (['--diffaug', 'color', '--diffaug-target', '0.5'], '--diffaug-adapt')])
def test_the_command_line_refuses(capsys, argv, word):
    import t2i_amd  # noqa: F401
    from t2i_amd.models.pggan import train_pggan
    with pytest.raises(SystemExit) as e:
        train_pggan.main(argv + ['--bench'])
    assert e.value.code == 2 and word in capsys.readouterr().err
