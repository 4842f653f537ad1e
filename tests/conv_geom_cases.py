"""The three convolution entry points (t2i_conv2d_fwd, _bwd_data, _bwd_filter) over the geometry space the descriptor admits: one case
table per family, seeded inputs and float64 references, for tests/test_conv_geom_host.py and tests/test_conv_geom_gpu.py.

A case is (B, H, W, Cin, Cout, KH, KW, SH, SW, padding) of the CONVOLUTION's descriptor (x [B,H,W,Cin] -> y [B,Ho,Wo,Cout], filter
[KH,KW,Cin,Cout]) with the word for the row it belongs to (`tag`), its channel class (`cls`), the entry points it drives, the algorithm
K.conv_algo must report per entry point in fp32 math (`algo`) and, where its channels admit the bf16-operand kernels, in bf16 math
(`algo_h`; None: the case is not run in bf16 math), and its switches (`sw`, t2i_tuning_set keys).  The algorithm words are one letter per
entry point, in the order fwd, bwd_data, bwd_filter: G implicit_gemm, H implicit_gemm_bf16_operands, 3 winograd_f2x2_3x3,
2 winograd_f2x2_2x2.

References are the float64 tap loops of oracle/np_ops.py; tests/test_conv_geom_host.py holds them to float64 torch convolutions and shows
that every case tells the indexing errors below from the truth.

Integer inputs and exactness
----------------------------
x, w, dy and bias are drawn from {-2..2}.  Every one of these is a bf16 number, so the operand rounding of the bf16 math mode is the
identity on them.

Direct GEMMs (t2i_igemm.hip, t2i_igemm_h.hip): every product is an integer of magnitude <= 4 and every partial sum of any subset of the
K_red products of an output element, in any order, tile or split-K grouping, is an integer of magnitude <= 4 K_red; the bias and the
accumulate base add at most 2.  K_red = KH KW Cin (fwd), KH KW Cout (bwd_data, all phases together), B Ho Wo (bwd_filter).  With
4 K_red + 2 < 2^24 float32 holds every intermediate exactly: `direct_bound`.

Winograd forms (t2i_winograd.hip): every transform matrix has entries in {0, +-1, +-1/2} and absolute row sums <= 2, so a 2-D transform
multiplies the largest magnitude by at most 4.  F(2x2,3x3): the filter transform G g G^T has the only halves (two of them: values on the
1/4 grid, magnitude <= 4 * 2), the input transform B^T d B is integral (<= 4 * 2); their products, summed over the K_red channels of a
batched GEMM, lie on the 1/4 grid with magnitude <= 64 K_red, and the output transform A^T M A (<= 4x) keeps the grid: <= 256 K_red, that
is 1024 K_red in units of 1/4.  The filter gradient transforms x (<= 8) and dy (A dy A^T, <= 8) integrally, sums K_red = T tiles of
products (<= 64 T) and applies G^T P G (halves, <= 4x): the same 1024 K_red in units of 1/4.  F(2x2,2x2) (the k4 s2 form) has integral
transforms throughout with the same gains over K_red = 4 Cin (fwd), 4 Cout (bwd_data) or T (bwd_filter).  `winograd_bound` = 1024 K_red + 8
(bias or base, in quarter units) must stay below 2^24.  The OUTPUT of every form is an integer (it equals the direct sum), so RELU
keeps it and LRELU with alpha = 0.25 gives a multiple of 1/4 of magnitude < 2^22: exact.

So on these inputs the kernel must equal the float64 oracle bit for bit: tolerance zero, derived rather than measured."""
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

FWD_TOL = 1e-5            # forward (tests/test_kernels_gpu.py)
GRAD_TOL = 1e-4           # input and filter gradients, as test_conv_medium_vs_oracle holds them
ENTRIES = ('fwd', 'bwd_data', 'bwd_filter')
ALGO_WORDS = {'G': 'implicit_gemm', 'H': 'implicit_gemm_bf16_operands', '3': 'winograd_f2x2_3x3', '2': 'winograd_f2x2_2x2'}
LRELU_ALPHA = 0.25        # dyadic: exact on integers

# the library's defaults of every switch a case or a test may set (csrc/t2i_capi.hip tuning_mut)
SWITCH_DEFAULTS = {'winograd_minwork': 50000000, 'winograd_minc': 128, 'winograd_maxhw': 1024, 'winograd_k4s2_minwork': 160000000,
                   'winograd_k4s2_minitems': 400, 'force_tile': 0, 'force_splitk': 0, 'no_thin': 0}
# the work thresholds lifted (as the module fixture of tests/test_kernels_gpu.py does), so that the Winograd kernels run at test sizes
LIFT = dict(winograd_minwork=0, winograd_k4s2_minwork=0, winograd_k4s2_minitems=0)


class Case(collections.namedtuple('Case', 'family tag cls shape entries algo algo_h sw')):
    """sw: a tuple of (switch, value) pairs (hashable: the references are cached per case)"""
    __slots__ = ()

    def opt(self, key, default=None):
        return dict(self.sw).get(key, default)

    @property
    def switches(self):
        return {k: v for k, v in self.sw if k in SWITCH_DEFAULTS}

    @property
    def id(self):
        B, H, W, Ci, Co, KH, KW, SH, SW, pad = self.shape
        return '%s-%s-%s-%dx%dx%dx%dx%d-k%dx%ds%dx%d%s' % (self.family, self.tag, self.cls, B, H, W, Ci, Co, KH, KW, SH, SW, pad[0])

    @property
    def phases(self):
        return self.shape[7] * self.shape[8] > 1

    def algos(self, math):
        word = self.algo if math == 'f32' else self.algo_h
        return {e: ALGO_WORDS[word[ENTRIES.index(e)]] for e in self.entries}

    def tol(self, entry):
        return FWD_TOL if entry == 'fwd' else GRAD_TOL

    @property
    def key(self):
        return census_key(self.shape[1:])


def census_key(hw_shape):
    """(KH, KW, SH, SW, padding, H odd, W odd, Cin % 32 == 0, Cout % 32 == 0) of (H, W, Cin, Cout, KH, KW, SH, SW, padding)"""
    H, W, Ci, Co, KH, KW, SH, SW, pad = hw_shape
    return (KH, KW, SH, SW, pad, H % 2 == 1, W % 2 == 1, Ci % 32 == 0, Co % 32 == 0)


def h_word(shape):
    """what K.conv_algo must report in bf16 math, restated from csrc/t2i_capi.hip: no Winograd form; h_eligible (fwd: Cin, bwd_data:
    Cout a multiple of 64, KH and KW <= 15: the loader keeps a row's tap masks in 15 + 15 bits); h_filter_eligible (Cin % 64 == 0,
    Cout % 8 == 0, Wo % 4 == 0; no limit on the kernel: the filter gradient has no tap masks)"""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = shape
    Wo = O.out_geometry(H, W, KH, KW, SH, SW, pad)[1]
    taps = KH <= 15 and KW <= 15
    return ''.join('H' if ok else 'G' for ok in (Ci % 64 == 0 and taps, Co % 64 == 0 and taps, Ci % 64 == 0 and Co % 8 == 0 and Wo % 4 == 0))


def _case(family, tag, cls, shape, algo='GGG', algo_h=None, entries=ENTRIES, **sw):
    """algo_h: stated by the tables that are about the bf16 paths; elsewhere h_word's where any entry point reaches a bf16-operand
    kernel (the case is then run in bf16 math too), else None.  tests/test_conv_geom_host.py holds both to K.conv_algo."""
    if algo_h is None and 'H' in h_word(shape):
        algo_h = h_word(shape)
    return Case(family, tag, cls, tuple(shape), tuple(entries), algo, algo_h, tuple(sorted(sw.items())))


# ---- channel classes -----------------------------------------------------------------------------------------------------------------
# The class decides the address path of the fp32 GEMM (csrc/t2i_capi.hip): VAR 0 (scalar) unless the gathered tensor's channel count
# C (Cin for fwd, Cout for bwd_data) is a multiple of 4; VAR 1 (vector) then; VAR 2 (tap-uniform) when C % 32 == 0; with C % 64 == 0 and
# bf16 math the bf16-operand kernels.  (Cin, Cout) per class: both counts are in the class, so that fwd and bwd_data take the same path.
CLASSES = collections.OrderedDict([('v0', (6, 10)), ('v1', (8, 12)), ('v2', (32, 32)), ('h', (64, 64))])


# ---- geometry rows: (tag, B, H, W, KH, KW, SH, SW, padding, switches) ---------------------------------------------------------------
# Every row appears once per channel class.  No class is left out of a row: every geometry below admits all four.
GEOMETRY_ROWS = [
    ('k1x7', 2, 8, 8, 1, 7, 1, 1, 'SAME', {}),             # pad (0, 3)
    ('k7x1', 2, 5, 8, 7, 1, 1, 1, 'SAME', {}),             # pad (3, 0); the kernel is taller than the map
    ('k1x3', 3, 5, 8, 1, 3, 1, 1, 'SAME', {}),
    ('k3x1', 2, 8, 8, 3, 1, 1, 1, 'SAME', {}),
    ('k5', 2, 9, 9, 5, 5, 1, 1, 'SAME', {}),               # pad 2, odd map
    ('k3s2v', 2, 7, 9, 3, 3, 2, 2, 'VALID', {}),           # phases of 4C, 2C, 2C and C; every row and column used
    ('k3s2v', 2, 8, 10, 3, 3, 2, 2, 'VALID', {}),          # ... the last row and column unused: dx = 0 (or act(bias)) there
    ('k3s2s', 2, 8, 8, 3, 3, 2, 2, 'SAME', {}),            # pad_t 0: kh0 = ph
    ('k3s2s', 2, 7, 7, 3, 3, 2, 2, 'SAME', {}),            # pad_t 1: kh0 = (ph + 1) % 2
    ('k3s2v', 3, 15, 13, 3, 3, 2, 2, 'VALID', {}),         # 168 rows per phase: three 64-row blocks, the last ragged
    ('k3s2s', 2, 16, 14, 3, 3, 2, 2, 'SAME', {}),          # 112 rows per phase: two blocks
    ('k1s2', 2, 8, 6, 1, 1, 2, 2, 'SAME', {}),             # three of four phases empty (K = 0)
    ('k2s3', 2, 10, 10, 2, 2, 3, 3, 'VALID', {}),          # five of nine phases empty, unused last row and column
    ('k3s3', 2, 10, 10, 3, 3, 3, 3, 'VALID', {}),          # nine phases of one tap each, unused trailing row and column
    ('s2x1', 2, 8, 12, 3, 3, 2, 1, 'SAME', {}),            # rectangular stride
    ('s1x2', 2, 8, 12, 3, 3, 1, 2, 'SAME', {}),
    ('big_k', 3, 2, 2, 4, 4, 2, 2, 'SAME', {}),            # one output pixel, 4 of 16 taps inside
    ('big_k', 3, 1, 1, 3, 3, 1, 1, 'SAME', {}),            # only the centre tap
    ('big_k', 3, 2, 2, 3, 3, 1, 1, 'SAME', {}),            # four of nine taps per pixel
    ('big_k', 2, 4, 4, 7, 1, 1, 1, 'SAME', {}),
    ('k4s1', 2, 6, 10, 4, 4, 1, 1, 'SAME', {}),            # pad (1, 2) on a non-square map
    ('deconv_v', 2, 10, 8, 4, 4, 2, 2, 'VALID', {'deconv': (4, 3)}),      # conv2d_transpose of a 4 x 3 map: (H - 1) s + k = 10 x 8
    ('deconv_v', 2, 9, 7, 3, 3, 2, 2, 'VALID', {'deconv': (4, 3)}),       # ... 9 x 7
]
PHASE_TAGS = ('k3s2v', 'k3s2s', 'k1s2', 'k2s3', 'k3s3', 's2x1')           # repeated under force_tile x force_splitk with no_thin

GEOMETRY = []
for _tag, _B, _H, _W, _KH, _KW, _SH, _SW, _pad, _sw in GEOMETRY_ROWS:
    for _cls, (_ci, _co) in CLASSES.items():
        _shape = (_B, _H, _W, _ci, _co, _KH, _KW, _SH, _SW, _pad)
        GEOMETRY.append(_case('geom', _tag, _cls, _shape, 'GGG', **_sw))

# ---- h_filter_eligible: one case on each side of Cout % 8 == 0 and of Wo % 4 == 0 -------------------------------------------------
H_FILTER = [
    _case('hf', 'cout72', 'h', (2, 8, 8, 64, 72, 3, 3, 1, 1, 'SAME'), 'GGG', 'HGH'),       # Cout % 8 == 0 (and not % 64: bwd_data on the fp32-operand GEMM)
    _case('hf', 'cout68', 'h', (2, 8, 8, 64, 68, 3, 3, 1, 1, 'SAME'), 'GGG', 'HGG'),       # Cout % 8 != 0
    _case('hf', 'wo8', 'h', (2, 6, 8, 64, 128, 3, 3, 1, 1, 'SAME'), 'GGG', 'HHH'),         # Wo % 4 == 0
    _case('hf', 'wo6', 'h', (2, 8, 6, 64, 128, 3, 3, 1, 1, 'SAME'), 'GGG', 'HHG'),         # Wo % 4 != 0
]

# ---- pixel walk: the filter gradient's VAR 2 (32 % Wo == 0, channels % 4) and its neighbours ---------------------------------------
WALK = [
    _case('walk', 'wo1', 'v2', (2, 4, 1, 32, 32, 3, 3, 1, 1, 'SAME')),                     # 32 output rows per K-tile; K = 8 pixels in all
    _case('walk', 'wo2', 'v2', (2, 3, 2, 32, 64, 3, 3, 1, 1, 'SAME')),
    _case('walk', 'wo2_s2', 'v2', (3, 8, 4, 32, 32, 4, 4, 2, 2, 'SAME')),
    _case('walk', 'wo32', 'v2', (1, 2, 32, 32, 32, 3, 3, 1, 1, 'SAME')),                   # one output row per K-tile
    _case('walk', 'wo3_generic', 'v2', (2, 4, 3, 32, 32, 3, 3, 1, 1, 'SAME')),             # 32 % 3 != 0: the generic decode
    _case('walk', 'wo16', 'v2', (1, 5, 16, 32, 32, 3, 3, 1, 1, 'SAME')),                   # two rows per K-tile, Ho odd: a tile straddles images
]

# ---- the last kernel on the bf16 tap-mask path (15 + 15 mask bits) and the first one off it ----------------------------------------
K15 = [
    _case('k15', 'k1x15', 'h', (1, 4, 16, 64, 64, 1, 15, 1, 1, 'SAME'), 'GGG', 'HHH'),
    _case('k15', 'k15x1', 'h', (1, 16, 4, 64, 64, 15, 1, 1, 1, 'SAME'), 'GGG', 'HHH'),
    _case('k16', 'k1x16', 'h', (1, 4, 16, 64, 64, 1, 16, 1, 1, 'SAME'), 'GGG', 'GGH'),      # h_eligible refuses KW = 16; the filter gradient has no tap masks
    _case('k16', 'k16x1', 'h', (1, 16, 4, 64, 64, 16, 1, 1, 1, 'SAME'), 'GGG', 'GGH'),
]


def _k3(B, H, W, Ci, Co):
    return (B, H, W, Ci, Co, 3, 3, 1, 1, 'SAME')


def _k4s2(B, H, W, Ci, Co):
    return (B, H, W, Ci, Co, 4, 4, 2, 2, 'SAME')


# ---- Winograd F(2x2,3x3): per term of winograd_eligible / winograd_filter_eligible one case just inside and one just outside ---------
# (`pair`: the tag of the case's routing partner, the same geometry on the other side of the term)
WINO3 = [
    _case('wino3', 'in', 'v2', _k3(2, 4, 4, 128, 128), '33G', **LIFT),                     # the inside partner of the terms below
    _case('wino3', 'h_odd', 'v2', _k3(2, 5, 4, 128, 128), 'GGG', **LIFT),                  # even H
    _case('wino3', 'w_odd', 'v2', _k3(2, 4, 5, 128, 128), 'GGG', **LIFT),                  # even W
    _case('wino3', 'c160', 'v2', _k3(2, 4, 4, 160, 160), '33G', **LIFT),                   # C % 32 == 0 ...
    _case('wino3', 'cin144', 'v1', _k3(2, 4, 4, 144, 160), 'GGG', **LIFT),                 # ... Cin % 32 == 16
    _case('wino3', 'cout144', 'v1', _k3(2, 4, 4, 160, 144), 'GGG', **LIFT),                # ... Cout % 32 == 16
    _case('wino3', 'minc96', 'v2', _k3(2, 4, 4, 96, 128), 'GGG', **LIFT),                  # winograd_minc = 128: min(Cin, Cout) = 96
    _case('wino3', 'maxhw_in', 'v2', _k3(1, 8, 8, 128, 128), '33G', winograd_maxhw=64, **LIFT),      # H W = 64 <= winograd_maxhw (set to 64)
    _case('wino3', 'maxhw_out', 'v2', _k3(1, 8, 10, 128, 128), 'GGG', winograd_maxhw=64, **LIFT),    # H W = 80
    _case('wino3', 'f65536', 'v2', _k3(2, 4, 4, 128, 512), '333', **LIFT),                 # Cin Cout = 65536: the filter gradient too
    _case('wino3', 'f61440', 'v2', _k3(2, 4, 4, 128, 480), '33G', **LIFT),                 # Cin Cout = 61440
    _case('wino3', 'hw2', 'v2', _k3(3, 2, 2, 128, 128), '33G', **LIFT),                    # every tile is all border
    _case('wino3', 'hw2_filter', 'v2', _k3(3, 2, 2, 256, 256), '333', **LIFT),
    _case('wino3', 'map2x16', 'v2', _k3(1, 2, 16, 128, 128), '33G', **LIFT),               # non-square
    _case('wino3', 'c160x224', 'v2', _k3(2, 4, 4, 160, 224), '33G', **LIFT),               # Cin != Cout, neither a multiple of 64
    _case('wino3', 'c224x160', 'v2', _k3(2, 4, 4, 224, 160), '33G', **LIFT),
    _case('wino3', 'c288x256', 'v2', _k3(1, 4, 6, 288, 256), '333', **LIFT),               # ... with the Winograd filter gradient, K and N ragged in 64
    _case('wino3', 't75', 'v2', _k3(3, 10, 10, 128, 128), '33G', **LIFT),                  # T = 75: one full GEMM tile and a ragged one
    _case('wino3', 'k1152', 'v2', _k3(1, 4, 4, 1152, 128), '333', **LIFT),                 # K = 1152 (features ++ text channels), T = 4
    _case('wino3', 'default_off', 'v2', _k3(2, 4, 4, 128, 128), 'GGG'),                    # the work threshold at its default: the direct GEMM
]

# ---- Winograd F(2x2,2x2), the k4 s2 SAME form: the terms of winograd_k4s2_eligible ---------------------------------------------------
WINO2 = [
    _case('wino2', 'in', 'v2', _k4s2(2, 8, 8, 128, 128), '222', **LIFT),
    _case('wino2', 'smallest', 'v2', _k4s2(1, 4, 4, 128, 128), '222', **LIFT),             # the smallest map it accepts: one tile
    _case('wino2', 'w6', 'v2', _k4s2(2, 8, 6, 128, 128), 'GGG', **LIFT),                   # W % 4 != 0
    _case('wino2', 'h6', 'v2', _k4s2(2, 6, 8, 128, 128), 'GGG', **LIFT),                   # H % 4 != 0
    _case('wino2', 'cin136', 'v1', _k4s2(2, 8, 8, 136, 128), '2G2', **LIFT),               # fwd: Cin % 8 == 0; bwd_data: Cin % 32 != 0, outside
    _case('wino2', 'cin132', 'v1', _k4s2(2, 8, 8, 132, 128), 'GGG', **LIFT),               # Cin % 8 != 0
    _case('wino2', 'cout160', 'v2', _k4s2(2, 8, 8, 128, 160), '222', **LIFT),              # Cout % 32 == 0 ...
    _case('wino2', 'cout144', 'v1', _k4s2(2, 8, 8, 128, 144), 'GGG', **LIFT),              # ... Cout % 32 == 16
    _case('wino2', 'cin96', 'v2', _k4s2(2, 8, 8, 96, 128), 'GGG', **LIFT),                 # winograd_k4s2_minc = 128
    _case('wino2', 'cout96', 'v2', _k4s2(2, 8, 8, 128, 96), 'GGG', **LIFT),
    _case('wino2', 'map4x12', 'v2', _k4s2(3, 4, 12, 160, 128), '222', **LIFT),             # non-square, T = 9
    _case('wino2', 'default_off', 'v2', _k4s2(2, 8, 8, 128, 128), 'GGG'),                  # the work thresholds at their defaults
]

WINO_PAIRS = [   # (family, just-eligible tag, just-ineligible tag): the fast path and its fallback at the same kernel geometry
    ('wino3', 'in', 'h_odd'), ('wino3', 'in', 'w_odd'), ('wino3', 'c160', 'cin144'), ('wino3', 'c160', 'cout144'), ('wino3', 'in', 'minc96'),
    ('wino3', 'maxhw_in', 'maxhw_out'), ('wino3', 'f65536', 'f61440'), ('wino3', 'in', 'default_off'),
    ('wino2', 'in', 'w6'), ('wino2', 'in', 'h6'), ('wino2', 'cin136', 'cin132'), ('wino2', 'cout160', 'cout144'), ('wino2', 'in', 'cin96'),
    ('wino2', 'in', 'cout96'), ('wino2', 'in', 'default_off'),
    ('k15', 'k1x15', 'k1x16'), ('k15', 'k15x1', 'k16x1'), ('hf', 'cout72', 'cout68'), ('hf', 'wo8', 'wo6'),
]

# ---- census rows: the geometry keys of the models' own layers that no row above has (tests/test_conv_geom_host.py forms the keys) -----
CENSUS = [
    # InceptionV3 (models/inception/model.py) at 299 x 299: the stem
    _case('census', 'stem_1a', 'v0', (1, 9, 9, 3, 32, 3, 3, 2, 2, 'VALID')),               # Conv2d_1a_3x3, 3 -> 32 on 299 x 299
    _case('census', 'stem_2a', 'v2', (1, 7, 7, 32, 32, 3, 3, 1, 1, 'VALID')),              # Conv2d_2a_3x3 on 149 x 149
    _case('census', 'stem_2b', 'v2', (1, 7, 7, 32, 64, 3, 3, 1, 1, 'SAME')),               # Conv2d_2b_3x3 on 147 x 147
    _case('census', 'stem_3b', 'v2', (1, 5, 5, 64, 80, 1, 1, 1, 1, 'VALID')),              # Conv2d_3b_1x1 on 73 x 73, Cout = 80
    _case('census', 'stem_4a', 'v1', (1, 7, 7, 80, 192, 3, 3, 1, 1, 'VALID')),             # Conv2d_4a_3x3, Cin = 80
    # 35 x 35 and 17 x 17 (odd maps): 1 x 1, 5 x 5, 3 x 3, 1 x 7, 7 x 1, and the stride-2 VALID reductions
    _case('census', 'k1_odd', 'v2', (2, 5, 5, 192, 64, 1, 1, 1, 1, 'SAME')),
    _case('census', 'k1_odd_c48', 'v2', (2, 5, 5, 192, 48, 1, 1, 1, 1, 'SAME')),           # Cout = 48
    _case('census', 'k5_c48', 'v1', (2, 7, 7, 48, 64, 5, 5, 1, 1, 'SAME')),                # Cin = 48
    _case('census', 'k3_odd', 'v2', (2, 5, 5, 64, 96, 3, 3, 1, 1, 'SAME')),
    _case('census', 'k3s2v_odd', 'v2', (2, 7, 7, 96, 96, 3, 3, 2, 2, 'VALID')),
    _case('census', 'k1x7_odd', 'v2', (1, 7, 9, 128, 128, 1, 7, 1, 1, 'SAME')),
    _case('census', 'k7x1_odd', 'v2', (1, 9, 7, 160, 192, 7, 1, 1, 1, 'SAME')),
    # 8 x 8 (even map): 1 x 1, 1 x 3, 3 x 1, 3 x 3; the logits
    _case('census', 'k1_even', 'v2', (1, 8, 8, 320, 192, 1, 1, 1, 1, 'SAME')),
    _case('census', 'k1x3_even', 'v2', (1, 8, 8, 384, 384, 1, 3, 1, 1, 'SAME')),
    _case('census', 'k3x1_even', 'v2', (1, 8, 8, 384, 384, 3, 1, 1, 1, 'SAME')),
    _case('census', 'k3_even', 'v2', (1, 8, 8, 448, 384, 3, 3, 1, 1, 'SAME')),             # (default thresholds: the direct GEMM at B = 1)
    _case('census', 'logits', 'v2', (3, 1, 1, 256, 20, 1, 1, 1, 1, 'VALID')),              # Logits/Conv2d_1c_1x1: Cout = 20
    # the GAN layers tests/test_host.py and FULL of tests/test_kernels_gpu.py list, whose keys the rows above do not have
    _case('census', 'gan_1x1', 'v2', (2, 4, 4, 256, 64, 1, 1, 1, 1, 'SAME')),              # 4 x 4 x 1024 -> 256, k1
    _case('census', 'gan_stem', 'v0', (2, 8, 8, 3, 160, 4, 4, 2, 2, 'SAME')),              # 3 -> 128 k4 s2 (Cout = 160: not the stem kernel's own 64 / 128)
    _case('census', 'gan_out', 'v0', (2, 8, 8, 3, 5, 3, 3, 1, 1, 'SAME')),                 # 3 -> 3 k3 (Cout = 5: the GEMM, not the tiny kernels)
    _case('census', 'gan_head', 'v2', (3, 4, 4, 64, 5, 4, 4, 4, 4, 'VALID')),              # the logit head's geometry with Cout = 5: the GEMM
]

ALL = GEOMETRY + H_FILTER + WALK + K15 + WINO3 + WINO2 + CENSUS
TABLES = collections.OrderedDict([('GEOMETRY', GEOMETRY), ('H_FILTER', H_FILTER), ('WALK', WALK), ('K15', K15), ('WINO3', WINO3),
                                  ('WINO2', WINO2), ('CENSUS', CENSUS)])
TABLE_LENGTHS = {'GEOMETRY': 92, 'H_FILTER': 4, 'WALK': 6, 'K15': 4, 'WINO3': 20, 'WINO2': 12, 'CENSUS': 21}

# the GAN layers as tests/test_host.py (test_conv_algorithm_choice_on_the_benchmark_layers) and FULL (tests/test_kernels_gpu.py) list
# them: (H, W, Cin, Cout, k, stride, padding)
GAN_LAYERS = [
    (64, 64, 3, 128, 4, 2, 'SAME'), (32, 32, 128, 256, 4, 2, 'SAME'), (16, 16, 256, 512, 4, 2, 'SAME'), (8, 8, 512, 1024, 4, 2, 'SAME'),
    (4, 4, 512, 1024, 3, 1, 'SAME'), (4, 4, 1152, 1024, 3, 1, 'SAME'), (8, 8, 512, 512, 3, 1, 'SAME'), (16, 16, 256, 256, 3, 1, 'SAME'),
    (32, 32, 128, 128, 3, 1, 'SAME'), (8, 8, 128, 512, 3, 1, 'SAME'), (8, 8, 128, 128, 3, 1, 'SAME'), (4, 4, 1024, 256, 1, 1, 'SAME'),
    (64, 64, 3, 3, 3, 1, 'SAME'), (4, 4, 1024, 1, 4, 4, 'VALID'),
]


def ids(cases):
    return dict(ids=[c.id for c in cases])


def by_tag(family, tag):
    hit = [c for c in ALL if c.family == family and c.tag == tag]
    assert len(hit) == 1, (family, tag, len(hit))
    return hit[0]


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def geometry(case):
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    return O.out_geometry(H, W, KH, KW, SH, SW, pad)          # Ho, Wo, pad_top, pad_left


def phase_table(case):
    """fill_phases (csrc/t2i_capi.hip) restated: per stride phase (ph, pw) of the input gradient its first taps (kh0, kw0), tap counts
    (nth, ntw) and output offsets (oh_off, ow_off)"""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    _, _, pt, pl = geometry(case)
    out = []
    for ph in range(SH):
        for pw in range(SW):
            kh0, kw0 = (ph + pt) % SH, (pw + pl) % SW
            nth = -(-(KH - kh0) // SH) if kh0 < KH else 0
            ntw = -(-(KW - kw0) // SW) if kw0 < KW else 0
            out.append((ph, pw, kh0, kw0, nth, ntw, (ph + pt - kh0) // SH, (pw + pl - kw0) // SW))
    return out


def reductions(case):
    """K_red per entry point: the most products any output element sums"""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    Ho, Wo, _, _ = geometry(case)
    return {'fwd': KH * KW * Ci, 'bwd_data': KH * KW * Co, 'bwd_filter': B * Ho * Wo}


def direct_bound(case, entry, amax=2):
    """largest magnitude of any partial sum of the direct GEMM, bias or accumulate base included, in units of 1"""
    return reductions(case)[entry] * amax * amax + amax


def winograd_bound(case, entry, amax=2):
    """largest magnitude of any intermediate of a Winograd form, in units of 1/4 (the module docstring derives it): K_red is the
    reduction of one batched GEMM: the channels (4 x the channels for the space-to-depth form) or the tiles T"""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    s2d = 4 if KH == 4 else 1
    T = B * (-(-H // (2 * SH))) * (-(-W // (2 * SW)))
    k_red = {'fwd': s2d * Ci, 'bwd_data': s2d * Co, 'bwd_filter': T}[entry]
    gain = 4                                                 # one 2-D transform: absolute row sums <= 2, twice
    return 4 * (gain * amax) * (gain * amax) * k_red * gain + 4 * amax


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(case, integer=False):
    """float32 {x, w, b (bias over Cout), bi (bias over Cin: the input gradient's, the transposed-conv form), dy, base (a filter-shaped
    accumulator)}, seeded from the case id.  integer: everything is drawn from {-2..2}; otherwise as test_conv_medium_vs_oracle draws
    (standard normal x, dy and bias, w / sqrt(KH KW Cin))."""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    Ho, Wo, _, _ = geometry(case)
    rng = np.random.default_rng(zlib.crc32(repr((case.id, integer)).encode()))
    if integer:
        draw = lambda shape: rng.integers(-2, 3, shape).astype(np.float32)      # noqa: E731
        out = dict(x=draw((B, H, W, Ci)), w=draw((KH, KW, Ci, Co)), dy=draw((B, Ho, Wo, Co)), b=draw(Co), bi=draw(Ci), base=draw((KH, KW, Ci, Co)))
    else:
        normal = lambda shape: rng.standard_normal(shape).astype(np.float32)    # noqa: E731
        out = dict(x=normal((B, H, W, Ci)), w=(rng.standard_normal((KH, KW, Ci, Co)) / np.sqrt(KH * KW * Ci)).astype(np.float32),
                   dy=normal((B, Ho, Wo, Co)), b=normal(Co), bi=normal(Ci), base=normal((KH, KW, Ci, Co)))
    for a in out.values():
        a.setflags(write=False)
    return out


def rne_bf16(a):
    """float32 -> nearest-even bf16 -> float32, in integer arithmetic on the bits"""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


# ---- references -----------------------------------------------------------------------------------------------------------------------
def _three(x, w, dy, xs, stride, pad, entries):
    out = {}
    if 'fwd' in entries:
        out['fwd'] = O.conv2d(x, w, None, stride, pad)
    if 'bwd_data' in entries:
        out['bwd_data'] = O.conv2d_bwd_data(dy, w, xs, stride, pad)
    if 'bwd_filter' in entries:
        out['bwd_filter'] = O.conv2d_bwd_filter(x, dy, w.shape, stride, pad)
    return out


@functools.lru_cache(maxsize=None)
def refs(case, integer=False, bf16=False):
    """float64 {entry: reference} without bias or activation; computed once, read-only.  fwd = conv(x, w), bwd_data = conv^T(dy, w),
    bwd_filter = x (*) dy.  bf16: on the RNE-rounded operands (what the bf16 math mode multiplies)."""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    I = inputs(case, integer)
    rnd = rne_bf16 if bf16 else (lambda a: a)
    x, w, dy = (rnd(I[k]).astype(np.float64) for k in ('x', 'w', 'dy'))
    out = _three(x, w, dy, (B, H, W, Ci), (SH, SW), pad, case.entries)
    for a in out.values():
        a.setflags(write=False)
    return out


def act(a, name):
    return {'none': lambda v: v, 'relu': O.relu, 'lrelu': lambda v: O.lrelu(v, LRELU_ALPHA)}[name](a)


def transpose_ref(case, integer=False):
    """conv2d_transpose of the `deconv` rows through the oracle's own entry (O.conv2d_transpose: VALID output (H - 1) s + k), with the
    bias over the image-side channels: what K.deconv_desc + conv_bwd_data compute"""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    I = inputs(case, integer)
    y = O.conv2d_transpose(I['dy'].astype(np.float64), I['w'].astype(np.float64), I['bi'].astype(np.float64), (SH, SW), pad)
    assert y.shape == (B, H, W, Ci), (y.shape, case.shape)
    return y


def torch_refs(case, integer=False, dtype='float64'):
    """The same three quantities from torch on the CPU: conv2d on the explicitly padded input, and autograd of it."""
    import torch
    import torch.nn.functional as F
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    I = inputs(case, integer)
    if pad == 'SAME':
        (_, pt, pb), (_, pl, pr) = O.same_pad(H, KH, SH), O.same_pad(W, KW, SW)
    else:
        pt = pb = pl = pr = 0
    dt = getattr(torch, dtype)
    xt = torch.from_numpy(I['x'].copy()).to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.from_numpy(I['w'].copy()).to(dt).permute(3, 2, 0, 1).contiguous().requires_grad_(True)      # HWIO -> OIHW
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, stride=(SH, SW))
    gt = torch.from_numpy(I['dy'].copy()).to(dt).permute(0, 3, 1, 2)
    dx, dw = torch.autograd.grad(y, [xt, wt], gt)
    return {'fwd': y.detach().permute(0, 2, 3, 1).numpy(), 'bwd_data': dx.permute(0, 2, 3, 1).numpy(),
            'bwd_filter': dw.permute(2, 3, 1, 0).numpy()}


def f32_yardstick(case, entry):
    """The error of the same operation evaluated in float32 by torch on the CPU against the float64 reference: it rounds the way a
    kernel must.  A case that states a bound of its own may state at most min(1e-4, 4 x this)."""
    return relerr(torch_refs(case, False, 'float32')[entry].astype(np.float64), refs(case)[entry])


# per-check bounds a case states for itself, with the measured value and the float32 yardstick beside it: {case id: {check: bound}}
STATED = {}


# ---- corruptions ----------------------------------------------------------------------------------------------------------------------
CORRUPTIONS = ('tap', 'khkw', 'io', 'hw', 'shsw', 'phase')


def exchange_io(w):
    """the filter read as [KH, KW, Cout, Cin] on the same memory (tests/thin_cases.py)"""
    KH, KW, Ci, Co = w.shape
    return np.ascontiguousarray(w.reshape(KH, KW, Co, Ci).transpose(0, 1, 3, 2))


def border_tap(case):
    """(kh, kw) of the first tap that meets the image at all"""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    Ho, Wo, pt, pl = geometry(case)
    return next(iter(O._taps(H, W, KH, KW, SH, SW, Ho, Wo, pt, pl)))[:2]


def _exchanged(case, corrupt):
    """the geometry an indexing that exchanges H / W (Ho / Wo), KH / KW or SH / SW computes with, on the same memory:
    (H, W, KH, KW, SH, SW, Ho, Wo), or None where that geometry's tensors do not have the sizes of the case's (the exchange then changes
    a tensor's size, or has no output: it is no quiet error)"""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    Ho, Wo, _, _ = geometry(case)
    if corrupt == 'hw':
        g = (W, H, KH, KW, SH, SW)
    elif corrupt == 'khkw':
        g = (H, W, KW, KH, SH, SW)
    else:
        g = (H, W, KH, KW, SW, SH)
    if pad == 'VALID' and (g[0] < g[2] or g[1] < g[3]):
        return None
    Ho2, Wo2, _, _ = O.out_geometry(*g, pad)
    if Ho2 <= 0 or Wo2 <= 0 or Ho2 * Wo2 != Ho * Wo:
        return None
    return g + (Ho2, Wo2)


def identity(case, corrupt):
    """True where the corruption is provably the identity on this case (the host test asserts that instead):
    tap: never; khkw: a square kernel whose taps that meet the image all lie on its diagonal; io: Cin or Cout is 1; hw: H == W and Ho == Wo with equal kernel extents and strides; shsw: SH == SW;
    phase: every stride phase has the same tap count (nothing beyond a phase's own K exists)."""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    if corrupt == 'khkw':                                   # (k3 on a 1 x 1 map: only the centre tap meets the image)
        Ho, Wo, pt, pl = geometry(case)
        return KH == KW and all(t[0] == t[1] for t in O._taps(H, W, KH, KW, SH, SW, Ho, Wo, pt, pl))
    if corrupt == 'io':
        return Ci == 1 or Co == 1
    if corrupt == 'hw':
        return H == W
    if corrupt == 'shsw':
        return SH == SW
    if corrupt == 'phase':
        return len(set(p[4] * p[5] for p in phase_table(case))) == 1
    return False


def applies(case, corrupt):
    """the corruption is a quiet error on this case: not the identity, and every tensor keeps its size"""
    if identity(case, corrupt):
        return False
    if corrupt in ('hw', 'khkw', 'shsw'):
        B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
        if corrupt == 'khkw' and KH == KW:
            return True
        return _exchanged(case, corrupt) is not None
    return True


def _unmasked_phases(case, dy, w):
    """The input gradient of a kernel that runs every stride phase to the longest phase's tap count and does not mask: tap index t
    beyond a phase's own nth * ntw is decoded like the others (jh, jw = divmod(t, ntw)), the filter tap read from the same memory
    (index wrapped into the filter) and the dy pixel it points at added where it exists."""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    Ho, Wo, _, _ = geometry(case)
    dx = O.conv2d_bwd_data(dy, w, (B, H, W, Ci), (SH, SW), pad)
    wf = w.reshape(KH * KW, Ci, Co)
    table = phase_table(case)
    tmax = max(p[4] * p[5] for p in table)
    for ph, pw, kh0, kw0, nth, ntw, oh_off, ow_off in table:
        for t in range(nth * ntw, tmax):
            jh, jw = divmod(t, max(ntw, 1))
            tap = wf[((kh0 + SH * jh) * KW + (kw0 + SW * jw)) % (KH * KW)]
            for ih in range(ph, H, SH):
                oh = (ih - ph) // SH + oh_off - jh
                if not 0 <= oh < Ho:
                    continue
                for iw in range(pw, W, SW):
                    ow = (iw - pw) // SW + ow_off - jw
                    if 0 <= ow < Wo:
                        dx[:, ih, iw, :] += dy[:, oh, ow, :] @ tap.T
    return dx


def corrupted(case, corrupt, integer=False):
    """float64 {entry: what the erroneous indexing computes}, in the shapes of the true references"""
    B, H, W, Ci, Co, KH, KW, SH, SW, pad = case.shape
    Ho, Wo, _, _ = geometry(case)
    I = inputs(case, integer)
    x, w, dy = (I[k].astype(np.float64) for k in ('x', 'w', 'dy'))
    shapes = {'fwd': (B, Ho, Wo, Co), 'bwd_data': (B, H, W, Ci), 'bwd_filter': (KH, KW, Ci, Co)}
    if corrupt == 'phase':                                  # the stride phases exist in the input gradient only
        out = dict(refs(case, integer))
        if 'bwd_data' in out:
            out['bwd_data'] = _unmasked_phases(case, dy, w)
        return out
    if corrupt == 'tap':
        tap = border_tap(case)
        w = w.copy()
        w[tap] = 0.0                                        # a border tap of the filter is never applied
        out = _three(x, w, dy, (B, H, W, Ci), (SH, SW), pad, case.entries)
        if 'bwd_filter' in out:
            out['bwd_filter'][tap] = 0.0                    # ... or never written
    elif corrupt == 'io':
        out = _three(x, exchange_io(w), dy, (B, H, W, Ci), (SH, SW), pad, case.entries)
        if 'bwd_filter' in out:
            out['bwd_filter'] = exchange_io(out['bwd_filter'])
    elif corrupt == 'khkw' and KH == KW:                    # the tap index decoded as (kw, kh)
        out = _three(x, np.ascontiguousarray(w.transpose(1, 0, 2, 3)), dy, (B, H, W, Ci), (SH, SW), pad, case.entries)
        if 'bwd_filter' in out:
            out['bwd_filter'] = np.ascontiguousarray(out['bwd_filter'].transpose(1, 0, 2, 3))
    else:                                                   # every index computed in the exchanged geometry, on the same memory
        H2, W2, KH2, KW2, SH2, SW2, Ho2, Wo2 = _exchanged(case, corrupt)
        out = _three(x.reshape(B, H2, W2, Ci), w.reshape(KH2, KW2, Ci, Co), dy.reshape(B, Ho2, Wo2, Co), (B, H2, W2, Ci), (SH2, SW2), pad,
                     case.entries)
    return {e: a.reshape(shapes[e]) for e, a in out.items()}


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

    def exact(self, name, got, ref, dtype=np.float32):
        """bit equality with a float64 reference that `dtype` holds exactly (float32), or with its RNE bf16 rounding (dtype 'bf16')"""
        got, ref = f64(got), np.asarray(ref, np.float64)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), 'the reference is not representable in float32'
        if dtype == 'bf16':
            ref = rne_bf16(ref.astype(np.float32)).astype(np.float64)
        ok = got.shape == ref.shape and np.array_equal(got, ref)
        self.seen.append((name + ' exact', 0.0 if ok else (float(np.abs(got - ref).max()) if got.shape == ref.shape else float('inf')), 0.0))
        if not ok:
            self.bad.append((name + ' exact', int((got != ref).sum()) if got.shape == ref.shape else got.shape, 'wrong elements'))

    def done(self):
        print('  case %s: %s' % (self.case, ', '.join('%s %.2e/%.0e' % t for t in self.seen)))
        unused = set(self.stated) - set(n for n, _, _ in self.seen)
        assert not unused, ('stated bounds for checks that do not exist', unused)
        assert not self.bad, (self.case, self.bad)
