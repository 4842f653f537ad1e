"""The draw kernel and the controller kernel of DESIGN.md section 4.39 on the GPU against their numpy restatement (tests/ada_cases.py):
every table bit for bit — the workgroup's edge and the row loop, the four image sizes, each policy alone and all three, p = 0, 0.3 and
1 — the call counter with its carry, the words a kernel must leave alone, a captured draw replayed, and the controller's state after
single observations and after sequences: integers and the integer-valued accumulators exact, p and last_r within 1e-6."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import ada_cases as AC  # noqa: E402
import diffaug_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 64, 255, 256, 257, 1024)
RESERVED = [0x11111111 * (j - 9) for j in range(10, 16)]            # the kernels must leave words 10-15 alone, whatever they hold


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import t2i_amd  # noqa: F401
    from t2i_amd import kernels as K
    return K


def to_dev(words):
    return torch.from_numpy(np.asarray(words, np.int64).astype(np.uint32).view(np.int32).copy()).cuda()


def to_host(state):
    return state.cpu().numpy().view(np.uint32).astype(np.int64)


def full_state(seed, p, counter=0):
    """a state with every word a kernel must not write set to something recognisable"""
    s = AC.make_state(seed, p, counter)
    s[5:10] = [AC.word_of(-7.0), AC.word_of(40.0), 2, AC.word_of(0.125), 6]
    s[10:] = RESERVED
    return s


@pytest.mark.parametrize('policy', sorted(AC.POLICY_MASKS))
def test_the_drawn_table_is_the_restatement_bit_for_bit(policy):
    K = need_gpu()
    mask = AC.POLICY_MASKS[policy]
    cases = [(n, H, W, p) for n in ROWS for H, W in AC.SIZES for p in (0.0, 0.3, 1.0)]
    got = []
    for i, (n, H, W, p) in enumerate(cases):
        state = to_dev(full_state(seed=100 + i, p=p, counter=i))
        got.append((K.diff_augment_draw(state, torch.full((n, 9), 99.0, device='cuda'), H, W, mask), state))
    torch.cuda.synchronize()
    for i, ((n, H, W, p), (table, state)) in enumerate(zip(cases, got)):
        before = full_state(seed=100 + i, p=p, counter=i)
        want, after = AC.draw(before, n, H, W, mask)
        assert np.array_equal(table.cpu().numpy().view(np.uint32), want.view(np.uint32)), (n, H, W, p)
        assert np.array_equal(to_host(state), after), (n, H, W, p)             # the counter + 1; words 0, 1 and 4-15 unchanged
        if p == 0.0:
            assert np.array_equal(want, np.tile(np.array(AC.IDENTITY_ROW, np.float32), (n, 1)))


def test_consecutive_calls_and_the_carry():
    K = need_gpu()
    first = full_state(seed=(9 << 32) | 4, p=0.3, counter=0xfffffffe)
    state = to_dev(first)
    tables = [K.diff_augment_draw(state, torch.empty(257, 9, device='cuda'), 16, 16, 7).clone() for _ in range(3)]
    words = first
    for k, t in enumerate(tables):
        want, words = AC.draw(words, 257, 16, 16, 7)
        assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32)), k
    assert AC.counter_of(words) == 0x100000001 and np.array_equal(to_host(state), words)
    assert (int(words[2]), int(words[3])) == (1, 1)                               # 0xffffffff + 1 carried into word 3
    preset = full_state(seed=4, p=1.0, counter=0xffffffff)
    state = to_dev(preset)
    K.diff_augment_draw(state, torch.empty(3, 9, device='cuda'), 4, 4, 7)
    after = to_host(state)
    assert (int(after[2]), int(after[3])) == (0, 1) and np.array_equal(after[4:], preset[4:]) and np.array_equal(after[:2], preset[:2])


def test_at_p_zero_the_operator_returns_its_input():
    need_gpu()
    from t2i_amd.utils import ops
    s = ops.DiffAugmentSampler(DC.ALL, p=0.0, seed=3, device='cuda')
    x = DC.inputs((5, 16, 16, 3))[0].cuda()
    table = s.draw(5, 16, 16)
    assert torch.equal(table.cpu(), DC.identity_table(5))
    assert torch.equal(ops.diff_augment(x, table, DC.ALL), x)
    assert s.counter == 1 and s.p == 0.0


def test_a_captured_draw_advances_with_every_replay():
    """One stream, one kernel node: replay i draws call k + i into the static buffer."""
    K = need_gpu()
    first = full_state(seed=21, p=0.3, counter=5)
    state, out = to_dev(first), torch.zeros(64, 9, device='cuda')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.diff_augment_draw(state, out, 5, 7, 7)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(state), first) and not bool(out.any())          # capturing ran nothing
    words = first
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        want, words = AC.draw(words, 64, 5, 7, 7)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert AC.counter_of(words) == 7 and np.array_equal(to_host(state), words)


def check_controller(got, want, tag):
    """seed, counter, calls, updates, reserved words: equal; acc_sign, acc_n (integer-valued floats): equal; p, last_r: within 1e-6"""
    for j in (0, 1, 2, 3, 5, 6, 7, 9) + tuple(range(10, 16)):
        assert int(got[j]) == int(want[j]), (tag, j, int(got[j]), int(want[j]))
    for j in (4, 8):
        assert abs(float(AC.f32_of(got[j])) - float(AC.f32_of(want[j]))) <= 1e-6, (tag, j, AC.f32_of(got[j]), AC.f32_of(want[j]))


@pytest.mark.parametrize('mode', [AC.LOGIT, AC.MIDPOINT], ids=['logit', 'midpoint'])
@pytest.mark.parametrize('n', [1, 4, 63, 64, 65, 257, 1000])
def test_one_observation_matches_the_restatement(n, mode):
    K = need_gpu()
    d_real, d_fake = AC.logits(n, 40 + n, mode, shift=0.3)
    assert AC.margin(d_real, d_fake, mode) > 1e-3
    for interval, target in ((1, 0.6), (1, -0.6), (4, 0.6)):                      # an adjustment up or down, and the call before one
        before = full_state(seed=8, p=0.5, counter=77)                               # (two calls and 40 logits already accumulated)
        state = to_dev(before)
        K.diffaug_observe(state, torch.from_numpy(d_real).cuda(), None if mode == AC.LOGIT else torch.from_numpy(d_fake).cuda(), mode,
                          target, interval, 16.0 * n)
        want = AC.observe(before, d_real, d_fake, mode, target, interval, 16.0 * n)
        check_controller(to_host(state), want, (n, mode, interval, target))
        assert (int(want[7]) == 0) == (interval == 1)


SEQUENCES = {          # name -> (p at the start, shift of the logits, interval, what p does)
    'rising': (0.25, 2.0, 2, 'up'), 'falling': (0.75, 0.0, 2, 'down'), 'pinned at 0': (0.0, 0.0, 2, 'zero'), 'pinned at 1': (1.0, 2.0, 2, 'one'),
    'interval 1': (0.5, 2.0, 1, 'up')}


@pytest.mark.parametrize('name', sorted(SEQUENCES))
def test_a_sequence_of_observations_matches_the_restatement(name):
    K = need_gpu()
    p0, shift, interval, trend = SEQUENCES[name]
    n, target, ramp = 65, 0.6, 4.0 * 65 * interval
    words = full_state(seed=2, p=p0, counter=123)
    words[5:10] = 0
    state = to_dev(words)
    ps = [p0]
    for call in range(2 * interval + 1):
        d_real, d_fake = AC.logits(n, 1000 * call + 7, AC.MIDPOINT, shift=shift)
        assert AC.margin(d_real, d_fake, AC.MIDPOINT) > 1e-3
        K.diffaug_observe(state, torch.from_numpy(d_real).cuda(), torch.from_numpy(d_fake).cuda(), AC.MIDPOINT, target, interval, ramp)
        words = AC.observe(words, d_real, d_fake, AC.MIDPOINT, target, interval, ramp)
        check_controller(to_host(state), words, (name, call))
        ps.append(float(AC.f32_of(words[4])))
    assert int(words[9]) == (2 * interval + 1) // interval and int(words[7]) == (2 * interval + 1) % interval
    assert {'up': ps[-1] == p0 + 0.5, 'down': ps[-1] == p0 - 0.5, 'zero': ps[-1] == 0.0 and min(ps) == 0.0, 'one': ps[-1] == 1.0 and max(ps) == 1.0}[trend], ps


def test_the_sampler_class_drives_both_kernels():
    need_gpu()
    from t2i_amd.utils import ops
    s = ops.DiffAugmentSampler('color,cutout', p=0.5, seed=6, device='cuda', adapt='logit', target=0.0, interval=1, ramp_images=32)
    words = AC.make_state(6, 0.5)
    out = torch.empty(8, 9, device='cuda')
    assert s.draw(8, 16, 16, out=out) is out
    want, words = AC.draw(words, 8, 16, 16, AC.COLOR | AC.CUTOUT)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    d = np.array([1.5, 2.0, -0.5, 3.0, 1.0, 0.5, 2.5, 0.25], np.float32)           # r = 0.75 > 0: p + 8 / 32
    s.observe(torch.from_numpy(d).cuda())
    words = AC.observe(words, d, None, AC.LOGIT, 0.0, 1, 32.0)
    assert np.array_equal(s.state_dict(), words) and s.p == 0.75 and s.last_r == 0.75 and s.updates == 1 and s.counter == 1
    assert float(s.p_tensor()) == 0.75 and s.p_tensor().is_cuda
    t = ops.DiffAugmentSampler('color,cutout', device='cuda')
    t.load_state_dict(s.state_dict())
    assert torch.equal(t.draw(8, 16, 16), s.draw(8, 16, 16))
