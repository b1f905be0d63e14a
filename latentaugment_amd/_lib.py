"""ctypes binding of liblatentaug_hip.so.  The C ABI is written down once, in include/latentaug_hip.h: the library is compiled
against that header and this module reads its prototypes and structs from it (`parse_header`), so there is no second table here.

The library is the product: there is no CPU or PyTorch fallback.  If it is missing, or a call fails, this module
raises (`LatentAugHipError`) -- it never silently computes elsewhere.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'liblatentaug_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'latentaug_hip.h')


class LatentAugHipError(RuntimeError):
    pass


_I = C.c_int
_SCALARS = {'void': None, 'int': _I, 'long': C.c_long, 'float': C.c_float, 'double': C.c_double, 'size_t': C.c_size_t,
            'unsigned': C.c_uint, 'unsigned long long': C.c_ulonglong, 'la_stream_t': C.c_void_p}
_TYPE_WORDS = {w for k in _SCALARS for w in k.split()} | {'char', 'short', 'signed'}


def _ctype(decl, named=True):
    """ctypes type of one C declarator: a named parameter or struct field ('const float* x', 'unsigned long long seed'), or with
    named=False a return type.  Every pointer is c_void_p (a `const char*` return: c_char_p); a scalar must be in _SCALARS."""
    if '*' in decl:
        return C.c_char_p if not named and decl.replace(' ', '') == 'constchar*' else C.c_void_p
    words = [w for w in decl.split() if w != 'const']
    if named:
        if len(words) < 2 or words[-1] in _TYPE_WORDS:
            raise LatentAugHipError(f'C header: parameter or field without a name: {decl!r}')
        words.pop()
    if ' '.join(words) not in _SCALARS or (named and words == ['void']):
        raise LatentAugHipError(f'C header: unknown type {" ".join(words)!r} in {decl!r}')
    return _SCALARS[' '.join(words)]


def parse_header(text):
    """The C ABI as ctypes: ({entry: (restype, argtypes)}, {struct: ctypes.Structure subclass}) from the text of the public header.
    Its style is regular -- /* */ comments, one `ret la_name(type name, ...);` per entry, `typedef struct tag { fields } name;` -- and
    whatever is left over after those (and the opaque-handle typedefs) is an error, never skipped or guessed at."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    structs, sigs = {}, {}

    def take_struct(m):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(';'))):
            if '*' in decl:
                raise LatentAugHipError(f'C header: pointer field in struct {m.group(2)}: {decl!r}')
            first, *more = [s.strip() for s in decl.split(',')]
            fields += [(n, _ctype(first)) for n in [first.split()[-1]] + more]
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {'_fields_': fields})
        return ''
    text = re.sub(r'typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;', take_struct, text, flags=re.S)
    text = re.sub(r'typedef\s+struct\s+\w+\s*\*?\s*\w+\s*;', '', text)      # opaque handles, la_stream_t
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r'\1', text, flags=re.S)
    for stmt in filter(None, (' '.join(s.split()) for s in text.split(';'))):
        m = re.fullmatch(r'(.+?)\s*\b(la_\w+)\s*\(([^()]*)\)', stmt)
        if not m or m.group(2) in sigs:
            raise LatentAugHipError(f'C header: not a prototype, or declared twice: {stmt!r}')
        ret, name, args = m.groups()
        sigs[name] = (_ctype(ret, named=False), [] if args.strip() == 'void' else [_ctype(a) for a in args.split(',')])
    return sigs, structs


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise LatentAugHipError(f'{HEADER_PATH}: the public header is the source of this binding and could not be read ({e})')


# name -> (restype, argtypes) of every entry of the header; la_feat_op / la_opt_config as ctypes structures
SIGNATURES, _structs = _read_header()
FeatOp, OptConfig = _structs['la_feat_op'], _structs['la_opt_config']

_lib = None
LOADED_PATH = None
DEV_LIB_PATH = os.path.join(_HERE, 'liblatentaug_hip_dev.so')      # `make -C latentaugment_amd/csrc dev`: measurement tools only
_use_dev = False


def select_dev_build():
    """Measurement tools (scripts/) and the one test that compares two internal code paths call this BEFORE the first load():
    the process then runs on the development build (kernel-variant knobs + LA_* environment switches).  The package never does."""
    global _use_dev
    if _lib is not None and not _use_dev:
        raise LatentAugHipError('select_dev_build() must come before the library is first used')
    _use_dev = True


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own HIP runtime: import it FIRST so that liblatentaug_hip.so binds to the runtime that owns torch's
    # streams and allocations (loading ours first leaves two runtimes in the process and HIP calls fail with
    # "no ROCm-capable device is detected")
    import torch  # noqa: F401
    path = DEV_LIB_PATH if _use_dev else LIB_PATH
    if not os.path.isfile(path):
        raise LatentAugHipError(
            f'{path} not found: build it with `make -C latentaugment_amd/csrc{" dev" if _use_dev else ""}` (or __graft_entry__.build()). '
            'There is no CPU fallback for the latent-augmentation hot path.')
    lib = C.CDLL(path)
    global LOADED_PATH
    LOADED_PATH = os.path.realpath(path)      # what was actually dlopen'ed (tests check it is the in-tree product build)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if _use_dev:
        lib.la_dev_knob_set.restype = _I
        lib.la_dev_knob_set.argtypes = [_I, _I]
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().la_last_error()
        raise LatentAugHipError(f'{what} failed (code {rc}): {msg.decode() if msg else "?"}')


def require_gpu(t):
    """Product tensors must live on the GPU: this path has no host implementation."""
    if not t.is_cuda:
        raise LatentAugHipError('latentaugment_amd needs a ROCm device tensor (no CPU fallback); got ' + str(t.device))


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def workspace(nbytes, device, dtype=None):
    """The one place where the package allocates a workspace or scratch buffer that it hands to the library: `nbytes` bytes, seen as
    `dtype` (uint8 unless given).  Uninitialised on purpose -- the library's contract (include/latentaug_hip.h) is that a workspace may
    hold any bytes when it is handed over and that nothing outside it is written.  Callers use the module attribute
    (`_lib.workspace(...)`), so that a test can put a guarded, pre-filled allocator in its place."""
    import torch
    dtype = torch.uint8 if dtype is None else dtype
    return torch.empty([int(nbytes) // torch.empty([], dtype=dtype).element_size()], dtype=dtype, device=device)


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
