"""The eight direct kernels of csrc/t2i_thin.hip (thin deconv, tiny conv and its filter gradient, the three head kernels, the stem and
its filter gradient): one case table per family, seeded inputs and float64 references, for tests/test_thin_host.py and
tests/test_thin_gpu.py.

A case is (B, H, W, Cin, Cout, KH, KW, stride, padding) of the CONVOLUTION's descriptor (x [B,H,W,Cin] -> y [B,Ho,Wo,Cout], filter
[KH,KW,Cin,Cout]) with the entry points it drives ('fwd' | 'bwd_data' | 'bwd_filter'), the entry points that must reach a direct kernel
(`direct`), the word for the branch it is there for (`tag`, in the test id) and its switches.  The references are the tap loops of
oracle/np_ops.py in float64; tests/test_thin_host.py holds them to float64 torch convolutions and shows that each case tells a dropped
border tap, exchanged filter axes and exchanged H / W from the truth, so the GPU tests do not rest on one implementation or on cases
that cannot see the error they are there for."""
import collections
import functools
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_ops as O  # noqa: E402

FWD_TOL = 1e-5            # forward, input gradient, transposed conv (tests/test_kernels_gpu.py)
GRAD_TOL = 1e-4           # filter gradients
STEM_GRAD_TOL = 1e-5      # the stem's filter gradient keeps the bound of test_stem_filter_gradient
ENTRIES = ('fwd', 'bwd_data', 'bwd_filter')


class Case(collections.namedtuple('Case', 'family tag shape entries direct sw')):
    """sw: a tuple of (switch, value) pairs (hashable: the references are cached per case)"""
    __slots__ = ()

    def opt(self, key, default=None):
        return dict(self.sw).get(key, default)

    @property
    def id(self):
        B, H, W, Ci, Co, KH, KW, s, pad = self.shape
        k = 'k%d' % KH if KH == KW else 'k%dx%d' % (KH, KW)
        return '%s-%s-%dx%dx%dx%dx%d-%ss%d%s' % (self.family, self.tag, B, H, W, Ci, Co, k, s, pad[0])

    def tol(self, entry):
        if entry != 'bwd_filter':
            return FWD_TOL
        return STEM_GRAD_TOL if self.family == 'stem' else GRAD_TOL


def _case(family, tag, shape, entries=ENTRIES, direct=None, **sw):
    return Case(family, tag, tuple(shape), tuple(entries), tuple(entries if direct is None else direct), tuple(sorted(sw.items())))


def _k4s2(B, H, W, Ci, Co):
    return (B, H, W, Ci, Co, 4, 4, 2, 'SAME')


# ---- thin deconv: k4 s2 SAME, Cin 1..4 on the image side; the kernel runs as the input gradient ------------------------------------
# (B, H, W, Cin, Cout): H x W is the image.  LDS of one workgroup = (100 (CH + 4) + 16 Cin CH) 4 bytes, CH = Cout / passes.
THIN = [
    _case('thin', 'ci1_c4n5', _k4s2(2, 16, 16, 1, 20), ['bwd_data']),                    # CI = 1, parts collapses to 1, CH = 20
    _case('thin', 'ci2_c4n9', _k4s2(2, 16, 32, 2, 36), ['bwd_data']),                    # CI = 2, CH = 36
    _case('thin', 'cout16', _k4s2(1, 32, 16, 3, 16), ['bwd_data']),                      # the smallest Cout
    _case('thin', 'ch64_one_pass', _k4s2(2, 16, 16, 3, 64), ['bwd_data'], thin_parts=1),   # the CH == 64 fast path in one pass
    _case('thin', 'four_passes', _k4s2(2, 16, 16, 4, 128), ['bwd_data'], thin_parts=4),    # the generic loop, four passes of 32
    _case('thin', 'ch128_over48k', _k4s2(1, 16, 32, 3, 256), ['bwd_data']),              # CH = 128: 77 440 bytes, the attribute call
    _case('thin', 'ch256_fits', _k4s2(1, 16, 16, 3, 512), ['bwd_data']),                 # CH = 256: 153 152 bytes
    _case('thin', 'raised_to_4', _k4s2(1, 16, 16, 4, 512), ['bwd_data']),                # 169 536 bytes at two passes: four passes of 128
    _case('thin', 'no_split_508', _k4s2(1, 16, 16, 3, 508), ['bwd_data'], direct=[]),    # one pass only (508 % 8 != 0): 302 336 bytes, GEMM
    _case('thin', 'no_split_252', _k4s2(1, 16, 16, 4, 252), ['bwd_data'], direct=[]),    # one pass only: 166 912 bytes, GEMM
    _case('thin', 'no_split_356', _k4s2(1, 16, 16, 1, 356), ['bwd_data'], direct=[]),    # one pass only: 166 784 bytes, GEMM
]
THIN_MODES_CASE = _case('thin', 'modes', _k4s2(2, 16, 16, 3, 128), ['bwd_data'])
THIN_MODES = ('bias', 'tanh', 'bias_lrelu', 'dy_off', 'w_off')

# ---- tiny conv: Cin, Cout <= 4; forward and (stride 1) input gradient on tiny_conv_kernel --------------------------------------------
TINY = [
    _case('tiny', 'cin_ne_cout', (3, 5, 7, 2, 4, 3, 3, 1, 'SAME'), direct=['fwd', 'bwd_data'], variants=True),
    _case('tiny', 'cout1', (2, 6, 9, 4, 1, 3, 3, 1, 'SAME'), direct=['fwd', 'bwd_data']),
    _case('tiny', 'k1_valid', (2, 8, 8, 1, 3, 1, 1, 1, 'VALID'), direct=['fwd', 'bwd_data']),
    _case('tiny', 'k2_pad01', (2, 9, 11, 3, 3, 2, 2, 1, 'SAME')),                        # 3 -> 3, k <= 3: the filter gradient is tiny_bwdw
    _case('tiny', 'k4s2', (2, 8, 12, 3, 2, 4, 4, 2, 'SAME'), direct=['fwd']),            # stride 2: the input gradient is a GEMM
    _case('tiny', 'valid_4to4', (3, 7, 5, 4, 4, 3, 3, 1, 'VALID'), direct=['fwd', 'bwd_data']),
]
TINY_LARGE = _case('tiny', 'grid_stride', (1, 728, 1456, 3, 3, 3, 3, 1, 'SAME'), ['fwd', 'bwd_data'])   # 1 059 968 pixels > 4096 * 256

# ---- tiny filter gradient: 3 -> 3, k <= 3 ---------------------------------------------------------------------------------------------
TINY_BWDW = [
    _case('bwdw', 'k3s2', (2, 7, 9, 3, 3, 3, 3, 2, 'SAME'), ['bwd_filter']),
    _case('bwdw', 'k1x3', (2, 6, 6, 3, 3, 1, 3, 1, 'SAME'), ['bwd_filter']),
    _case('bwdw', 'k1_valid', (1, 5, 5, 3, 3, 1, 1, 1, 'VALID'), ['bwd_filter']),
    _case('bwdw', 'k2_pad01', (2, 9, 11, 3, 3, 2, 2, 1, 'SAME'), ['bwd_filter']),
    _case('bwdw', 'under_256_px', (1, 3, 4, 3, 3, 3, 3, 1, 'SAME'), ['bwd_filter']),
]

# ---- head: the whole map of a sample reduced to 1 x 1 x Cout <= 4 --------------------------------------------------------------------
HEAD = [
    _case('head', 'cout2', (7, 4, 4, 64, 2, 4, 4, 4, 'VALID'), variants=True),
    _case('head', 'cout3', (5, 4, 4, 32, 3, 4, 4, 4, 'VALID')),
    _case('head', 'b1_k256_cout4', (1, 4, 4, 16, 4, 4, 4, 4, 'VALID')),
    _case('head', 'k45', (6, 3, 3, 5, 1, 3, 3, 3, 'VALID')),                             # K % 4 != 0 and K < 64
    _case('head', 'misaligned', (9, 4, 4, 64, 1, 4, 4, 4, 'VALID'), offsets=True),       # x, then w, one float into a larger buffer
]

# ---- stem: 3 -> 64 | 128, k4 s2 SAME; forward and filter gradient -------------------------------------------------------------------
STEM_SHAPES = [((2, 10, 80), 'wo40_ragged_block'), ((1, 32, 18), 'h_ne_w'), ((3, 2, 2), 'one_pixel'), ((2, 16, 48), 'w48')]
STEM = [_case('stem', tag, _k4s2(B, H, W, 3, Co), ['fwd', 'bwd_filter'], bias_off=(i == 0))
        for i, ((B, H, W), tag) in enumerate(STEM_SHAPES) for Co in (64, 128)]

# ---- the pair entry in fp32 storage: one stem, one head and one 3 -> 3 shape --------------------------------------------------------
PAIR = [
    _case('pair', 'stem', _k4s2(2, 16, 48, 3, 128)),
    _case('pair', 'head', (7, 4, 4, 64, 2, 4, 4, 4, 'VALID')),
    _case('pair', 'tiny', (2, 9, 11, 3, 3, 3, 3, 1, 'SAME')),
]

ALL = THIN + [THIN_MODES_CASE] + TINY + [TINY_LARGE] + TINY_BWDW + HEAD + STEM + PAIR

# the models' own edge layers: (shape, entry points on a direct kernel)
MODEL_SHAPES = [
    (_k4s2(64, 64, 64, 3, 128), ENTRIES),                       # wgancls critic stem; its input gradient = the generator's out_deconv
    (_k4s2(64, 64, 64, 3, 64), ENTRIES),                        # gancls / StackGAN
    ((64, 64, 64, 3, 3, 3, 3, 1, 'SAME'), ENTRIES),             # the 3 -> 3 output conv
    ((64, 4, 4, 1024, 1, 4, 4, 4, 'VALID'), ENTRIES),           # the logit head
]

# thin deconv, default thin_parts = 2: (Cin, Cout) -> on the direct kernel?  The first Cout = 4 (mod 8) over 160 KiB per Cin and the
# last one under it; Cin = 4 at two passes: 496 is split again, 504 cannot be (504 % 16 != 0), 512 is.
THIN_LDS_EDGES = [(1, 348, True), (1, 356, False), (2, 300, True), (2, 308, False), (3, 268, True), (3, 276, False), (4, 244, True),
                  (4, 252, False), (4, 488, True), (4, 496, True), (4, 504, False), (4, 512, True), (3, 512, True), (3, 508, False)]


def ids(cases):
    return dict(ids=[c.id for c in cases])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def geometry(case):
    B, H, W, Ci, Co, KH, KW, s, pad = case.shape
    Ho, Wo, pt, pl = O.out_geometry(H, W, KH, KW, s, s, pad)
    return Ho, Wo, pt, pl


@functools.lru_cache(maxsize=None)
def inputs(case, integer=False):
    """float32 {x, w, b (bias over Cout), bi (bias over Cin: the transposed-conv form), dy, base (a filter-shaped accumulator)},
    seeded from the case.  integer: x, dy and w are integers in -3..3, so every partial sum of every entry point is an integer far below
    2^24 and float32 holds the result exactly in any summation order."""
    B, H, W, Ci, Co, KH, KW, s, pad = case.shape
    Ho, Wo, _, _ = geometry(case)
    rng = np.random.default_rng(zlib.crc32(repr((case, integer)).encode()))
    if integer:
        draw = lambda shape: rng.integers(-3, 4, shape).astype(np.float32)
        x, w, dy = draw((B, H, W, Ci)), draw((KH, KW, Ci, Co)), draw((B, Ho, Wo, Co))
    else:
        x = rng.standard_normal((B, H, W, Ci)).astype(np.float32)
        w = (rng.standard_normal((KH, KW, Ci, Co)) / np.sqrt(KH * KW * Ci)).astype(np.float32)
        dy = rng.standard_normal((B, Ho, Wo, Co)).astype(np.float32)
    out = dict(x=x, w=w, dy=dy, b=rng.standard_normal(Co).astype(np.float32), bi=rng.standard_normal(Ci).astype(np.float32),
               base=rng.standard_normal((KH, KW, Ci, Co)).astype(np.float32))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- references -----------------------------------------------------------------------------------------------------------------------
def exchange_io(w):
    """the filter read as [KH, KW, Cout, Cin] and transposed back to the HWIO shape: w'[kh, kw, ci, co] = flat[kh, kw][co * Cin + ci].
    With Cin == Cout this is the transpose of the two axes; with Cin == 1 or Cout == 1 it is the identity (both orders address the same
    memory, so no such error exists there)."""
    KH, KW, Ci, Co = w.shape
    return np.ascontiguousarray(w.reshape(KH, KW, Co, Ci).transpose(0, 1, 3, 2))


CORRUPTIONS = ('tap', 'io', 'hw')


def applies(case, corrupt):
    B, H, W, Ci, Co, KH, KW, s, pad = case.shape
    if corrupt == 'io':
        return Ci > 1 and Co > 1
    if corrupt == 'hw':
        return H != W
    return True


def border_tap(case):
    """(kh, kw) of the first tap that meets the image at all: (0, 0) everywhere but on the stem's 2 x 2 image, whose outer ring of the
    4 x 4 filter lies in the padding for its one output pixel (there the first of the four taps that remain)"""
    B, H, W, Ci, Co, KH, KW, s, pad = case.shape
    Ho, Wo, pt, pl = geometry(case)
    return next(iter(O._taps(H, W, KH, KW, s, s, Ho, Wo, pt, pl)))[:2]


def _refs(case, integer, corrupt, entries):
    B, H, W, Ci, Co, KH, KW, s, pad = case.shape
    Ho, Wo, _, _ = geometry(case)
    I = inputs(case, integer)
    x, w, dy = (I[k].astype(np.float64) for k in ('x', 'w', 'dy'))
    xs, ys = (B, H, W, Ci), (B, Ho, Wo, Co)
    tap = border_tap(case)
    if corrupt == 'tap':
        w = w.copy()
        w[tap] = 0.0                                    # a border tap of the filter is never applied
    elif corrupt == 'io':
        w = exchange_io(w)
    elif corrupt == 'hw':                               # every index is computed with H and W (Ho and Wo) exchanged, on the same memory
        assert KH == KW
        x, dy = x.reshape(B, W, H, Ci), dy.reshape(B, Wo, Ho, Co)
    out = {}
    if 'fwd' in entries:
        out['fwd'] = O.conv2d(x, w, None, (s, s), pad).reshape(ys)
    if 'bwd_data' in entries:
        out['bwd_data'] = O.conv2d_bwd_data(dy, w, x.shape, (s, s), pad).reshape(xs)
    if 'bwd_filter' in entries:
        dw = O.conv2d_bwd_filter(x, dy, w.shape, (s, s), pad)
        if corrupt == 'tap':
            dw[tap] = 0.0                               # ... or never written
        elif corrupt == 'io':
            dw = exchange_io(dw)
        out['bwd_filter'] = dw
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def refs(case, integer=False):
    """float64 {entry: reference} over the case's entry points, without bias or activation; computed once, read-only.
    fwd = conv(x, w), bwd_data = conv^T(dy, w), bwd_filter = x (*) dy."""
    return _refs(case, integer, None, case.entries)


def corrupted(case, corrupt):
    return _refs(case, False, corrupt, case.entries)


def act(a, name):
    return {'none': lambda v: v, 'lrelu': O.lrelu, 'tanh': np.tanh}[name](a)


def torch_refs(case, integer=False):
    """The same three quantities from float64 torch: conv2d on the explicitly padded input, and autograd of it."""
    import torch
    import torch.nn.functional as F
    B, H, W, Ci, Co, KH, KW, s, pad = case.shape
    I = inputs(case, integer)
    if pad == 'SAME':
        (_, pt, pb), (_, pl, pr) = O.same_pad(H, KH, s), O.same_pad(W, KW, s)
    else:
        pt = pb = pl = pr = 0
    xt = torch.from_numpy(I['x'].astype(np.float64)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.from_numpy(I['w'].astype(np.float64)).permute(3, 2, 0, 1).contiguous().requires_grad_(True)      # HWIO -> OIHW
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, stride=s)
    gt = torch.from_numpy(I['dy'].astype(np.float64)).permute(0, 3, 1, 2)
    dx, dw = torch.autograd.grad(y, [xt, wt], gt)
    return {'fwd': y.detach().permute(0, 2, 3, 1).numpy(), 'bwd_data': dx.permute(0, 2, 3, 1).numpy(),
            'bwd_filter': dw.permute(2, 3, 1, 0).numpy()}


def f32_yardstick(case, entry):
    """The error of the same operation evaluated in float32 by torch on the CPU against the float64 reference: it rounds the way a
    kernel must.  A case that states a bound of its own may state at most min(1e-4, 4 x this) (the factor covers another summation
    order); tests/test_thin_host.py holds every stated bound to that."""
    import torch
    import torch.nn.functional as F
    B, H, W, Ci, Co, KH, KW, s, pad = case.shape
    I = inputs(case)
    if pad == 'SAME':
        (_, pt, pb), (_, pl, pr) = O.same_pad(H, KH, s), O.same_pad(W, KW, s)
    else:
        pt = pb = pl = pr = 0
    xt = torch.from_numpy(I['x'].copy()).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.from_numpy(I['w'].copy()).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, stride=s)
    dx, dw = torch.autograd.grad(y, [xt, wt], torch.from_numpy(I['dy'].copy()).permute(0, 3, 1, 2))
    got = {'fwd': y.detach().permute(0, 2, 3, 1), 'bwd_data': dx.permute(0, 2, 3, 1), 'bwd_filter': dw.permute(2, 3, 1, 0)}[entry]
    return relerr(got.double().numpy(), _refs(case, False, None, (entry,))[entry])


# per-check bounds a case states for itself, with the measured value and the float32 yardstick beside it: {case id: {check: bound}}
STATED = {}


# ---- measuring ------------------------------------------------------------------------------------------------------------------------
def f64(t):
    return np.asarray(t, np.float64) if isinstance(t, np.ndarray) else t.detach().cpu().double().numpy()


def relerr(got, ref):
    """max-norm relative error"""
    got, ref = f64(got), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


class Bounds(object):
    """The checks of one case: each is held to the bound handed in with it unless the case states its own (STATED); all measured
    values are printed (pytest -s) and all failures are reported together."""

    def __init__(self, case):
        self.case, self.stated, self.bad, self.seen = case.id, dict(STATED.get(case.id, {})), [], []

    def check(self, name, err, tol):
        tol = self.stated.get(name, tol)
        self.seen.append((name, err, tol))
        if not err <= tol:
            self.bad.append((name, err, tol))

    def exact(self, name, got, ref):
        """bit equality with a float64 reference that float32 holds exactly"""
        got, ref = f64(got), np.asarray(ref, np.float64)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), 'the reference is not representable in float32'
        ok = got.shape == ref.shape and np.array_equal(got, ref)
        self.seen.append((name + ' exact', 0.0 if ok else float(np.abs(got - ref).max()), 0.0))
        if not ok:
            self.bad.append((name + ' exact', int((got != ref).sum()), 'wrong elements'))

    def same(self, name, ok):
        """bit equality of two results of the library"""
        self.seen.append((name + ' same bits', 0.0 if ok else 1.0, 0.0))
        if not ok:
            self.bad.append((name, 'bits differ'))

    def done(self):
        print('  case %s: %s' % (self.case, ', '.join('%s %.2e/%.0e' % t for t in self.seen)))
        unused = set(self.stated) - set(n for n, _, _ in self.seen)
        assert not unused, ('stated bounds for checks that do not exist', unused)
        assert not self.bad, (self.case, self.bad)
