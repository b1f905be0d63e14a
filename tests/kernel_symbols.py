"""The gfx950 code objects embedded in the product library, and the kernels they hold.

`code_objects(lib_path, out_dir)` unbundles every `__CLANG_OFFLOAD_BUNDLE__` section of the .so into one ELF file per code object;
`kernel_symbols(lib_path)` is the sorted set of mangled kernel names: every symbol X for which a code object carries the kernel
descriptor X.kd as an object symbol.  One kernel template instantiation is one name, so this is the list of kernel forms the library
ships.  `demangle(names)` gives the readable spelling of each."""
import os
import re
import subprocess
import tempfile

LLVM_BIN = '/opt/rocm/lib/llvm/bin'
BUNDLER = os.path.join(LLVM_BIN, 'clang-offload-bundler')
READELF = os.path.join(LLVM_BIN, 'llvm-readelf')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def tools_present():
    return os.path.isfile(BUNDLER) and os.path.isfile(READELF)


def code_objects(lib_path, out_dir):
    """Unbundle every gfx950 code object of `lib_path` into `out_dir`; returns their paths in file order."""
    blob = open(lib_path, 'rb').read()
    starts = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', blob)]
    objs = []
    for i, p in enumerate(starts):
        src, obj = os.path.join(str(out_dir), f'b{i}.bin'), os.path.join(str(out_dir), f'c{i}.o')
        with open(src, 'wb') as f:
            f.write(blob[p:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        r = subprocess.run([BUNDLER, '--type=o', f'--targets={TARGET}', f'--input={src}', f'--output={obj}', '--unbundle'], capture_output=True)
        assert r.returncode == 0 and os.path.getsize(obj) > 0, r.stderr.decode()[-500:]
        objs.append(obj)
    return objs


_SYM_ROW = re.compile(r'^\s*\d+:\s+[0-9a-fA-F]+\s+\d+\s+(\w+)\s+\w+\s+\w+\s+\S+\s+(\S+)\s*$')


def kernel_symbols(lib_path, out_dir=None):
    """Sorted mangled names of every kernel in the gfx950 code objects of `lib_path`."""
    if out_dir is None:
        with tempfile.TemporaryDirectory() as d:
            return kernel_symbols(lib_path, d)
    names = set()
    for obj in code_objects(lib_path, out_dir):
        r = subprocess.run([READELF, '--symbols', '-W', obj], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-500:]
        rows = [m.groups() for m in map(_SYM_ROW.match, r.stdout.decode(errors='replace').splitlines()) if m]
        syms = {name for _, name in rows}
        for kind, name in rows:
            if kind == 'OBJECT' and name.endswith('.kd'):
                assert name[:-3] in syms, f'{name} has no kernel symbol beside it'
                names.add(name[:-3])
    return sorted(names)


def demangle(names):
    """{mangled: demangled} by c++filt; a name it does not know stays as it is."""
    names = list(names)
    if not names:
        return {}
    r = subprocess.run(['c++filt'], input='\n'.join(names) + '\n', capture_output=True, text=True)
    out = r.stdout.splitlines() if r.returncode == 0 else names
    assert len(out) == len(names)
    return dict(zip(names, out))
