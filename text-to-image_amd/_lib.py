"""ctypes binding of libt2i_hip.so, READ from the one declaration of its C ABI: include/t2i_hip.h.  At import this module parses
the header's function prototypes, struct bodies, `#define`s and enums into SIGNATURES, the three Structure classes and CONSTANTS
(tests/test_abi.py holds the reader to the header), so an entry point or a constant is written once, in C.  There is NO fallback:
if the shared library is missing, a symbol is absent or a declaration cannot be read, importing this module raises — the product
path never silently computes elsewhere."""
import ctypes
import os
import re

# The HIP runtime must come into the process through PyTorch first: libt2i_hip.so links against libamdhip64.so.7 by SONAME, and
# PyTorch ships its own copy.  Loaded in the other order (`from t2i_amd import _lib` before anything imported torch) the loader binds
# torch to /opt/rocm's runtime as well, and torch's device enumeration and this library's launches then disagree about the device
# ("no ROCm-capable device is detected" at the first launch: __graft_entry__.py run as a script did exactly that).
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('T2I_HIP_LIB', os.path.join(_HERE, 'lib', 'libt2i_hip.so'))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 't2i_hip.h')

# ---- reading the header: the ONE rule set that turns a C type of include/t2i_hip.h into a ctypes type -----------------------------
_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float,
            'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'long long': ctypes.c_longlong, 't2i_stream_t': ctypes.c_void_p}


def _code(text):
    """The header without comments and with runs of white space folded: declarations may span lines."""
    return re.sub(r'[ \t]+', ' ', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S))


def _ctype(decl, where, pointers=(), named=True):
    """ctypes type of one parameter, struct field (`named`: the last word is its name) or return type, written as in C."""
    words = [w for w in decl.replace('*', ' * ').split() if w != 'const']
    if not words or words[0] == '*' or re.search(r'[^\w\s*]', decl):
        raise ValueError('%s: cannot read `%s`' % (where, decl.strip()))
    if '*' in words:
        base = ' '.join(words[:words.index('*')])
        if words.count('*') > 1:
            return ctypes.c_void_p
        return ctypes.c_char_p if base == 'char' else dict(pointers).get(base, ctypes.c_void_p)
    for base in (' '.join(words), ' '.join(words[:-1])) if named else (' '.join(words),):
        if base in _SCALARS:
            return _SCALARS[base]
    raise ValueError('%s: no ctypes mapping for `%s`' % (where, decl.strip()))


_INT_EXPR = r'(?=.*\d)(?:0[xX][0-9a-fA-F]+|\d+|<<|>>|[\s()+\-*|&~])+'     # integer literals, parentheses and integer operators: safe to eval
_ENUM = r'\benum\b[^{;]*\{([^}]*)\}'
_STRUCT = r'\btypedef struct \w*\s*\{([^}]*)\}\s*(\w+)\s*;'


def header_constants(text):
    """name -> int for every `#define T2I_* <integer expression>` and every enum member, in header order."""
    found = []
    for define, expr, members in re.findall(r'^ ?# ?define (T2I_\w+) ([^\n]+)$|' + _ENUM, _code(text), re.M):
        if define and re.fullmatch(_INT_EXPR, expr):
            found.append((define, int(eval(expr))))
        nxt = 0
        for item in filter(None, (i.strip() for i in members.split(','))):
            name, eq, expr = (p.strip() for p in item.partition('='))
            if eq and not re.fullmatch(_INT_EXPR, expr):
                raise ValueError('include/t2i_hip.h: enum member %s = `%s` is not an integer expression' % (name, expr))
            nxt = int(eval(expr)) if eq else nxt
            found.append((name, nxt))
            nxt += 1
    return dict(found)


def header_structs(text):
    """typedef name -> ctypes `_fields_` list, from the header's `typedef struct { ... } name;` bodies, fields in declared order."""
    out = {}
    for body, name in re.findall(_STRUCT, _code(text)):
        out[name] = fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            first, *more = decl.split(',')         # `int32_t B, H, W, Cin`: the type is written with the first name
            if more and '*' in decl:
                raise ValueError('%s: one pointer field per declaration, not `%s`' % (name, decl))
            kind = _ctype(first, name)
            fields += [(n.strip(), kind) for n in [first.replace('*', ' ').split()[-1]] + more]
    return out


def header_signatures(text, pointers=()):
    """name -> (restype, [argtypes]) for every function the header declares, in header order.  `pointers`: struct typedef name ->
    what a single pointer to it maps to.  Whatever is left of the header besides the preprocessor lines, the `extern "C"` braces,
    the typedefs and the enums must be a function declaration this module can read: anything else raises, naming it."""
    code = re.sub(_STRUCT + '|' + _ENUM + r'\s*;|\btypedef void ?\* ?t2i_stream_t\s*;|extern "C" \{|^ ?#[^\n]*$|^ ?\}\s*$', ' ',
                  _code(text), flags=re.M)
    out = {}
    for stmt in filter(None, (' '.join(s.split()) for s in code.split(';'))):
        m = re.fullmatch(r'(.+?)\b(\w+) ?\(([^()]*)\)', stmt)
        if not m:
            raise ValueError('include/t2i_hip.h: cannot read the declaration `%s`' % stmt)
        ret, name, args = m.groups()
        out[name] = (None if ret.strip() == 'void' else _ctype(ret, name, pointers, named=False),
                     [] if args.strip() in ('void', '') else [_ctype(a, '%s, argument %d' % (name, i + 1), pointers) for i, a in enumerate(args.split(','))])
    return out


with open(HEADER_PATH) as _f:
    _HEADER = _f.read()
CONSTANTS = header_constants(_HEADER)            # every T2I_* value of the header; kernels.py names its own from here too
_FIELDS = header_structs(_HEADER)


class ConvDesc(ctypes.Structure):
    """t2i_conv_desc"""
    _fields_ = _FIELDS['t2i_conv_desc']


class ConvOpts(ctypes.Structure):
    """t2i_conv_opts: optional side inputs / outputs of one conv call"""
    _fields_ = _FIELDS['t2i_conv_opts']


class ImageDesc(ctypes.Structure):
    """t2i_image_desc: one image of t2i_preprocess_images' ragged batch"""
    _fields_ = _FIELDS['t2i_image_desc']


def header_values(*names):
    """(T2I_<name>, ...) as the header defines them: how this module and kernels.py give their public constants their values."""
    return tuple(CONSTANTS['T2I_' + n] for n in names)


XFORM_NONE, XFORM_KEEP, XFORM_HAVE = header_values('XFORM_NONE', 'XFORM_KEEP', 'XFORM_HAVE')
DT_F32, DT_BF16 = header_values('DT_F32', 'DT_BF16')      # t2i_dtype: element type of the activation tensors of a call
SIGNATURES = header_signatures(_HEADER, {'t2i_conv_desc': ctypes.POINTER(ConvDesc), 't2i_conv_opts': ctypes.POINTER(ConvOpts)})

if not os.path.exists(LIB_PATH):
    raise ImportError('libt2i_hip.so not found at %s — build it with text-to-image_amd/csrc/build.sh '
                      '(or `python -c "import __graft_entry__ as g; g.build()"`); there is no CPU fallback' % LIB_PATH)

ABI_VERSION = CONSTANTS['T2I_ABI_VERSION']       # argument lists changed in v5, v6 and v7 — symbols alone do not tell

lib = ctypes.CDLL(LIB_PATH)
try:
    lib.t2i_version.restype = ctypes.c_int
    _got = lib.t2i_version()
except AttributeError:
    _got = None
if _got != ABI_VERSION:
    raise ImportError('%s reports ABI version %r, this package binds version %d: a stale build would be called with shifted '
                      'arguments — rebuild with text-to-image_amd/csrc/build.sh' % (LIB_PATH, _got, ABI_VERSION))
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)          # AttributeError here == ABI mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


class T2IError(RuntimeError):
    pass


def check(rc, what=''):
    if rc != 0:
        raise T2IError('%s failed (%d): %s' % (what, rc, lib.t2i_last_error().decode('utf-8', 'replace')))
