"""Dev tool: bench.py on ANOTHER build of the library (same-box A/B of two .so files in one gpurun call):
    python scripts/bench_with_lib.py tmp_libs/base/liblatentaug_hip.so --steps 20 --warmup 5 --no-cpu-baseline
    python scripts/bench_with_lib.py tmp_libs/base/liblatentaug_hip.so --script bench_kid.py [that script's args]
The library path replaces latentaugment_amd._lib.LIB_PATH before anything loads it; symbols the other build lacks are dropped from the
binding table (an older build has no la_noise_normal_f32: the bench workload does not call it).  `--script NAME` as the first argument
after the library runs scripts/NAME (a benchmark of the product library) in place of bench.py."""
import ctypes
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lib_path = os.path.abspath(sys.argv[1])
script = os.path.join(ROOT, 'bench.py')
args = sys.argv[2:]
if args[:1] == ['--script']:
    script, args = os.path.join(ROOT, 'scripts', os.path.basename(args[1])), args[2:]
sys.argv = [script] + args
import torch  # noqa: E402,F401  (its HIP runtime first, as _lib.load() does)
from latentaugment_amd import _lib  # noqa: E402
_lib.LIB_PATH = lib_path
probe = ctypes.CDLL(lib_path)
for k in list(_lib.SIGNATURES):
    if not hasattr(probe, k):
        del _lib.SIGNATURES[k]
runpy.run_path(script, run_name='__main__')
