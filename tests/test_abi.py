"""The Python binding is READ from include/t2i_hip.h (text-to-image_amd/_lib.py); these host tests hold the reader to the header.

Parser cases: literal snippets, one per mapping rule, with the ctypes they must give.  Mutation cases: the real header with one
parameter narrowed, one dropped, one widened and two struct fields swapped — the derived entry must follow each time.  Symbols: every
derived name is exported by the built library.  Layout: tests/workers/abi_layout.c, compiled by the host clang, prints sizeof and
offsetof of the three structs, and the ctypes classes must agree.

That each mutation case can fail was checked once by running it against a reader made blind to that mutation (patched in a
throw-away script, not kept): `int64_t` mapped to c_int32 fails the narrowing case, `double` mapped to c_float fails the widening case,
a reader that deletes `float scale,` from the text before parsing fails the dropped-parameter case, and a header_structs that sorts
the fields by name fails the reordering case; all four pass against the real reader."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLANG = '/opt/rocm/lib/llvm/bin/clang'          # the host compiler of tools/sanitize_host.sh
C = ctypes


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(os.path.join(ROOT, 'text-to-image_amd', 'lib', 'libt2i_hip.so')):
        import __graft_entry__ as ge
        ge.build()
    import t2i_amd  # noqa: F401
    from t2i_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def header():
    with open(os.path.join(ROOT, 'include', 't2i_hip.h')) as f:
        return f.read()


# ---- parser cases: one per mapping rule ------------------------------------------------------------------------------------------
class Desc(ctypes.Structure):
    _fields_ = [('x', ctypes.c_int32)]


class Opts(ctypes.Structure):
    _fields_ = [('x', ctypes.c_int32)]


POINTERS = {'t2i_conv_desc': C.POINTER(Desc), 't2i_conv_opts': C.POINTER(Opts)}
CASES = [
    ('int f(int a, int32_t b);', (C.c_int, [C.c_int, C.c_int32])),
    ('int64_t f(int64_t a, uint64_t b);', (C.c_int64, [C.c_int64, C.c_uint64])),
    ('float f(float a, double b);', (C.c_float, [C.c_float, C.c_double])),
    ('size_t f(size_t n);', (C.c_size_t, [C.c_size_t])),
    ('long long f(long long a, const long long b);', (C.c_longlong, [C.c_longlong, C.c_longlong])),
    ('int f(int, float, long long);', (C.c_int, [C.c_int, C.c_float, C.c_longlong])),                       # unnamed parameters
    ('int f(t2i_stream_t stream);', (C.c_int, [C.c_void_p])),
    ('const char* f(const char* key, char* out);', (C.c_char_p, [C.c_char_p, C.c_char_p])),
    ('int f(const t2i_conv_desc* d, t2i_conv_opts* o, const t2i_conv_opts *p);', (C.c_int, [C.POINTER(Desc), C.POINTER(Opts), C.POINTER(Opts)])),
    ('int f(void* a, const void* b, float* c, const float* d);', (C.c_int, [C.c_void_p] * 4)),
    ('int f(void** a, int32_t* b, const t2i_image_desc* c, float* const* d, const uint8_t* e, char** f, t2i_conv_desc** g);',
     (C.c_int, [C.c_void_p] * 7)),
    ('void* f(int a);', (C.c_void_p, [C.c_int])),
    ('void f(const void* p, size_t n);', (None, [C.c_void_p, C.c_size_t])),
    ('int f(void);', (C.c_int, [])),
    ('size_t f();', (C.c_size_t, [])),
    ('int f(const float* x,\n      int64_t rows,   int32_t C,\n      t2i_stream_t stream);', (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p])),
    ('int f(const void* a /* of (rows, C); that is, a[r*C + c] */, int32_t dtype /* of a */, // trailing (x, y);\n t2i_stream_t stream);',
     (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p])),
]


@pytest.mark.parametrize('text,want', CASES, ids=[c[0][:40].replace('\n', ' ') for c in CASES])
def test_a_declaration_maps_by_the_rules(lib, text, want):
    assert lib.header_signatures(text, POINTERS) == {'f': want}


def test_declarations_keep_their_order_and_the_rest_of_a_header_is_not_a_function(lib):
    text = ('#ifndef H\n#define H\n#ifdef __cplusplus\nextern "C" {\n#endif\n#define T2I_N (1 << 4) /* f(x); */\ntypedef void* t2i_stream_t; /* s */\n'
            'enum { T2I_A = 0, T2I_B = 1 };\nenum {\n  T2I_C = 3, /* , */\n  T2I_D\n};\n'
            'typedef struct t2i_s {\n  int32_t a, b; /* ; */\n  const void* p;\n  size_t n;\n  int64_t o;\n} t2i_s;\n'
            'int zz(void);\nint aa(t2i_stream_t s);\n#ifdef __cplusplus\n}\n#endif\n#endif\n')
    assert list(lib.header_signatures(text)) == ['zz', 'aa']
    assert lib.header_constants(text) == {'T2I_N': 16, 'T2I_A': 0, 'T2I_B': 1, 'T2I_C': 3, 'T2I_D': 4}
    assert lib.header_structs(text) == {'t2i_s': [('a', C.c_int32), ('b', C.c_int32), ('p', C.c_void_p), ('n', C.c_size_t), ('o', C.c_int64)]}


@pytest.mark.parametrize('text', ['int ok(int a);\nint t2i_odd(int a, half b);', 'int ok(int a);\nhalf t2i_odd(int a);',
                                  'int t2i_odd(int a, unsigned b);', 'int t2i_odd(int (*cb)(int), int b);', 'int t2i_odd(int a[4]);',
                                  'int t2i_odd(int a)\nint next(void);', 'struct t2i_odd { int a; };', 'int t2i_odd;'])
def test_what_the_rules_do_not_cover_raises_and_names_it(lib, text):
    with pytest.raises(ValueError, match='t2i_odd'):
        lib.header_signatures(text, POINTERS)


def test_a_struct_field_or_enum_value_outside_the_rules_raises(lib):
    with pytest.raises(ValueError, match='t2i_odd'):
        lib.header_structs('typedef struct t2i_odd { int32_t a; half b; } t2i_odd;')
    with pytest.raises(ValueError, match='t2i_odd'):
        lib.header_structs('typedef struct t2i_odd { int32_t *a, b; } t2i_odd;')
    with pytest.raises(ValueError, match='T2I_ODD'):
        lib.header_constants('enum { T2I_ODD = sizeof(int) };')
    assert lib.header_constants('#define T2I_NAME "text"\n#define T2I_F 1.5f\n#define T2I_GUARD\n#define T2I_X 0x10\n') == {'T2I_X': 16}


# ---- mutation cases: the real header, changed; the derived entry follows -------------------------------------------------------------
def mutate(header, old, new):
    assert header.count(old) == 1, old
    return header.replace(old, new)


def test_narrowing_one_parameter_changes_the_entry(lib, header):
    old = 'size_t t2i_col_reduce_workspace_bytes(int64_t rows, int32_t C);'
    got = lib.header_signatures(mutate(header, old, old.replace('int64_t', 'int32_t')))
    assert lib.header_signatures(header)['t2i_col_reduce_workspace_bytes'] == (C.c_size_t, [C.c_int64, C.c_int32])
    assert got['t2i_col_reduce_workspace_bytes'] == (C.c_size_t, [C.c_int32, C.c_int32])


KT_SGD = 'int t2i_kt_sgd(float* kt, const float* wdist_sums, float scale, float lr, t2i_stream_t stream);'


def test_dropping_one_parameter_changes_the_entry(lib, header):
    got = lib.header_signatures(mutate(header, KT_SGD, KT_SGD.replace('float scale, ', '')))
    assert lib.header_signatures(header)['t2i_kt_sgd'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p])
    assert got['t2i_kt_sgd'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p])


def test_widening_one_float_changes_the_entry(lib, header):
    got = lib.header_signatures(mutate(header, KT_SGD, KT_SGD.replace('float lr', 'double lr')))
    assert got['t2i_kt_sgd'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_double, C.c_void_p])
    was = lib.header_signatures(header)
    assert was.pop('t2i_kt_sgd') == lib.SIGNATURES['t2i_kt_sgd'] != got.pop('t2i_kt_sgd') and got == was       # nothing else moved


def test_reordering_two_struct_fields_changes_the_fields(lib, header):
    a, b = '  size_t xform_bytes;\n', '  int32_t xform_mode;\n'
    got = lib.header_structs(mutate(header, a + b, b + a))
    want = list(lib.ConvOpts._fields_)
    i = [n for n, _ in want].index('xform_bytes')
    assert want[i:i + 2] == [('xform_bytes', C.c_size_t), ('xform_mode', C.c_int32)]
    want[i], want[i + 1] = want[i + 1], want[i]
    assert got['t2i_conv_opts'] == want != list(lib.ConvOpts._fields_)
    assert got['t2i_conv_desc'] == list(lib.ConvDesc._fields_) and got['t2i_image_desc'] == list(lib.ImageDesc._fields_)


# ---- the real header against the module, the library and the C compiler -------------------------------------------------------------
def test_the_module_holds_what_the_header_declares(lib, header):
    pointers = {'t2i_conv_desc': C.POINTER(lib.ConvDesc), 't2i_conv_opts': C.POINTER(lib.ConvOpts)}
    assert lib.SIGNATURES == lib.header_signatures(header, pointers) and len(lib.SIGNATURES) >= 140
    assert list(lib.SIGNATURES)[:3] == ['t2i_version', 't2i_last_error', 't2i_stat']                        # header order
    assert lib.SIGNATURES['t2i_conv2d_algo'] == (C.c_int, [C.POINTER(lib.ConvDesc), C.c_int32])
    assert lib.SIGNATURES['t2i_conv2d_bwd_filter'][1][5] is C.POINTER(lib.ConvOpts)
    assert lib.SIGNATURES['t2i_filter_cache_invalidate'] == (None, [C.c_void_p, C.c_size_t])
    assert lib.CONSTANTS == lib.header_constants(header)
    assert lib.ABI_VERSION == lib.CONSTANTS['T2I_ABI_VERSION'] == lib.lib.t2i_version()
    assert '#define T2I_ABI_VERSION %d' % lib.ABI_VERSION in header and 'currently %d' % lib.ABI_VERSION in header
    from t2i_amd import kernels as K
    assert K.ALGO_NAMES == ('implicit_gemm', 'winograd_f2x2_3x3', 'winograd_f2x2_2x2', 'direct_small', 'implicit_gemm_bf16_operands')
    assert (K.ACT_LRELU, K.KNN_MAX_K, K.SPECTRAL_MAX_ITEMS, lib.DT_BF16, lib.XFORM_KEEP) == (1, 8, 1 << 22, 1, 1)


def test_every_derived_name_is_a_symbol_with_its_types_set(lib):
    for name, (res, args) in lib.SIGNATURES.items():
        fn = getattr(lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_struct_layouts_match_the_c_compiler(lib, tmp_path):
    exe = str(tmp_path / 'abi_layout')
    subprocess.run([CLANG, '-O0', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'workers', 'abi_layout.c'),
                    '-o', exe], check=True)
    lines = subprocess.run([exe], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout.split('\n')
    got = [(s, f, int(v)) for s, f, v in (ln.split() for ln in lines if ln)]
    want = []
    for cname, cls in (('t2i_conv_desc', lib.ConvDesc), ('t2i_conv_opts', lib.ConvOpts), ('t2i_image_desc', lib.ImageDesc)):
        want.append((cname, 'sizeof', C.sizeof(cls)))
        want += [(cname, f, getattr(cls, f).offset) for f, _ in cls._fields_]
    assert got == want
    assert (C.sizeof(lib.ConvDesc), C.sizeof(lib.ConvOpts), C.sizeof(lib.ImageDesc)) == (56, 72, 40)
