"""The device-side parameter draw and the controller of its probability p (include/t2i_hip.h, t2i_diffaug_state)
restated in numpy: Philox4x32-10, the table of call k, and one observation of the controller.  Integers are computed in uint64 and
masked to 32 bits; every float of the table is float32 formed by the single rounding the header names, so the kernel's table is
reproduced bit for bit.  The controller's threshold is formed in float64 (the tests keep every logit 1e-3 away from it), its
accumulators and p in float32 like the kernel's.

The state is the sixteen words as an int64 array of values in [0, 2^32), which is what DiffAugmentSampler.state_dict() returns."""
import numpy as np

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
LOGIT, MIDPOINT = 0, 1
POLICY_MASKS = {'color': COLOR, 'translation': TRANSLATION, 'cutout': CUTOUT, 'color,translation,cutout': 7}
SIZES = ((4, 4), (5, 7), (16, 16), (256, 256))
IDENTITY_ROW = (0.0, 1.0, 1.0, 0, 0, 0, 0, 0, 0)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter [..., 4] and key [..., 2] (broadcast against each other), any integer dtype holding 32-bit words -> [..., 4] uint64"""
    c = [np.asarray(counter)[..., j].astype(np.uint64) & MASK for j in range(4)]
    k = [np.asarray(key)[..., j].astype(np.uint64) & MASK for j in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]               # < 2^64: no wrap
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(np.broadcast_arrays(*c), -1)


def u01(w):
    """float(w >> 8) * 2^-24: exact, in [0, 1)"""
    return (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def below(w, m):
    return ((w * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def f32_of(word):
    return np.array([word], np.uint32).view(np.float32)[0]


def word_of(value):
    return int(np.array([value], np.float32).view(np.uint32)[0])


def make_state(seed=0, p=1.0, counter=0):
    s = np.zeros(16, np.int64)
    s[0], s[1] = seed & 0xffffffff, seed >> 32
    s[2], s[3] = counter & 0xffffffff, counter >> 32
    s[4] = word_of(p)
    return s


def counter_of(state):
    return int(state[2]) | (int(state[3]) << 32)


def draw(state, n, H, W, mask):
    """-> (the table [n, 9] float32 of the call the state's counter names, the state after the call: the counter + 1, nothing else)"""
    state = np.asarray(state, np.int64)
    p = f32_of(state[4])
    rows = np.arange(n, dtype=np.uint64)
    key = np.array([state[0], state[1]], np.uint64)

    def block(j):
        ctr = np.stack([rows, np.full(n, j, np.uint64), np.full(n, state[2], np.uint64), np.full(n, state[3], np.uint64)], -1)
        w = philox4x32_10(ctr, key)
        return w, u01(w[:, 0]) < p

    P = np.tile(np.array(IDENTITY_ROW, np.float32), (n, 1))
    if mask & COLOR:
        w, on = block(0)
        P[on, 0] = (u01(w[:, 1]) - np.float32(0.5))[on]
        P[on, 1] = (np.float32(2.0) * u01(w[:, 2]))[on]
        P[on, 2] = (u01(w[:, 3]) + np.float32(0.5))[on]
    if mask & TRANSLATION:
        w, on = block(1)
        for col, size, word in ((3, H, 1), (4, W, 2)):
            r = int(size / 8.0 + 0.5)
            P[on, col] = (below(w[:, word], 2 * r + 1) - r)[on]
    if mask & CUTOUT:
        w, on = block(2)
        for col, size, word in ((5, H, 1), (7, W, 2)):
            ext = int(size / 2.0 + 0.5)
            off = below(w[:, word], size - ext % 2 + 1) - ext // 2
            P[on, col] = np.maximum(off, 0)[on]
            P[on, col + 1] = np.minimum(off + ext, size)[on]
    after = state.copy()
    k = (counter_of(state) + 1) & ((1 << 64) - 1)
    after[2], after[3] = k & 0xffffffff, k >> 32
    return P, after


def gates(state, n):
    """[n, 3] bool: which of colour, translation, cutout the call applies to each row"""
    p = f32_of(state[4])
    rows = np.arange(n, dtype=np.uint64)
    out = []
    for j in range(3):
        ctr = np.stack([rows, np.full(n, j, np.uint64), np.full(n, state[2], np.uint64), np.full(n, state[3], np.uint64)], -1)
        out.append(u01(philox4x32_10(ctr, np.array([state[0], state[1]], np.uint64))[:, 0]) < p)
    return np.stack(out, -1)


def theta_of(d_real, d_fake, mode):
    if mode == LOGIT:
        return 0.0
    return 0.5 * (float(np.mean(np.asarray(d_real, np.float64))) + float(np.mean(np.asarray(d_fake, np.float64))))


def margin(d_real, d_fake, mode):
    """min |d_real - theta| in float64: the tests keep it above 1e-3 so that no sign hangs on the rounding of theta"""
    return float(np.abs(np.asarray(d_real, np.float64) - theta_of(d_real, d_fake, mode)).min())


def observe(state, d_real, d_fake, mode, target, interval, ramp_images):
    """-> the state after one observation"""
    s = np.asarray(state, np.int64).copy()
    d = np.asarray(d_real, np.float64) - theta_of(d_real, d_fake, mode)
    f = np.float32
    acc_sign = f(f32_of(s[5]) + f(np.sign(d).sum()))
    acc_n = f(f32_of(s[6]) + f(len(d)))
    calls = int(s[7]) + 1
    if calls >= interval:
        r = f(acc_sign / acc_n)
        step = f(acc_n / f(ramp_images))
        p = f32_of(s[4])
        p = f(p + step) if r > f(target) else (f(p - step) if r < f(target) else p)
        p = min(max(p, f(0.0)), f(1.0))
        s[4], s[8], s[9] = word_of(p), word_of(r), (int(s[9]) + 1) & 0xffffffff
        acc_sign, acc_n, calls = f(0.0), f(0.0), 0
    s[5], s[6], s[7] = word_of(acc_sign), word_of(acc_n), calls
    return s


def logits(n, seed, mode, shift=0.0):
    """(d_real, d_fake) float32 [n] ~ N(shift, 1) and N(-shift, 1), re-drawn from the next seed until every |d_real - theta| > 1e-3"""
    for s in range(seed, seed + 1000):
        rs = np.random.RandomState(s)
        d_real = (rs.standard_normal(n) + shift).astype(np.float32)
        d_fake = (rs.standard_normal(n) - shift).astype(np.float32)
        if margin(d_real, d_fake, mode) > 1e-3:
            return d_real, d_fake
    raise AssertionError('no well-separated logits found')
