"""Dev tool: one sha256 per translation unit of the gfx950 code object inside its object file.
    python scripts/device_code_hashes.py DIR
For every csrc/*.o under DIR (DIR itself, DIR/csrc or DIR/latentaugment_amd/csrc): the .hip_fatbin section dumped with llvm-objcopy, the
hipv4-amdgcn-amd-amdhsa--gfx950 entry unbundled with clang-offload-bundler, hashed.  Two trees whose lists are equal run the same
device code (a unit without kernels has no such section and prints dashes): a host-only change (an engine's launch set-up, a header's host helpers) leaves every line as it was.  Compare with diff."""
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def main():
    root = sys.argv[1]
    objs = []
    for sub in ('', 'csrc', os.path.join('latentaugment_amd', 'csrc')):
        objs = sorted(glob.glob(os.path.join(root, sub, '*.o')))
        if objs:
            break
    if not objs:
        sys.exit(f'no csrc/*.o under {root}: build the library first')
    with tempfile.TemporaryDirectory() as tmp:
        fatbin, code = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'code')
        for obj in objs:
            if subprocess.run([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', f'.hip_fatbin={fatbin}', obj],
                              stderr=subprocess.DEVNULL).returncode:
                print('-' * 64, os.path.basename(obj), '(host code only)')
                continue
            subprocess.run([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', f'--targets={TARGET}',
                            f'--input={fatbin}', f'--output={code}'], check=True)
            with open(code, 'rb') as f:
                print(hashlib.sha256(f.read()).hexdigest(), os.path.basename(obj))


if __name__ == '__main__':
    main()
