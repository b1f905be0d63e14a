#!/usr/bin/env python3
"""Which GPU test file launches which kernel form: writes tests/golden/kernel_reach.json from kernel traces.

One trace per GPU test file, each from a fresh process, with mangled names (-M):

    rocprofv3 --kernel-trace -M -f csv -d DIR -o test_hip_x -- python -m pytest -m gpu -x -q tests/test_hip_x.py

The trace's file name names the test file: `test_hip_x_kernel_trace.csv` (what rocprofv3 writes) or `test_hip_x.csv` stands for
tests/test_hip_x.py.  A raw trace has one row per dispatch; `--reduce RAW... -o OUT.csv` folds it into one row per kernel name with
a `Count` column, which this tool reads just as well (a traced file of the suite dispatches some 10^5 kernels).

    python scripts/kernel_reach.py traces/*.csv            # the whole record, from traces of every GPU test file
    python scripts/kernel_reach.py --merge traces/test_hip_pair_metrics.csv     # replace the entries of that file only

The record is {mangled: {"name": demangled, "files": {"tests/test_hip_x.py": dispatch count}}} over the kernel symbols of the
product library (tests/kernel_symbols.py); names of torch, rocBLAS or the development build are dropped.  With
`--by-reading tests/test_hip_x.py:MANGLED ...` a form that the named file launches by the host dispatch code, but whose file could not
be traced, is entered as {"count": 0, "by_reading": true}.  Printed at the end: the forms no file reaches, and the forms reached by
non-judging files only.  tests/test_kernel_reach_cpu.py holds the built library against the record."""
import argparse
import collections
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'kernel_reach.json')

# GPU test files whose assertions do not hold a kernel's values against a float64 restatement or a reference golden: a form reached
# only from these has no judge.
NON_JUDGING = {
    'tests/test_hip_history.py': 'compares a used handle with a fresh one, HIP against HIP',
    'tests/test_hip_workspace_guard.py': 'checks the guard bands round each workspace, not the values written inside',
    'tests/test_hip_bwd_cone.py': 'windowed backward against the whole-frame backward of the same build',
    'tests/test_hip_col_window_up.py': 'column-window launches against the whole-frame pass of the same build',
    'tests/test_hip_image_chain.py': 'deferred ToRGB schedule against the per-block schedule of the same handle, bit for bit',
    'tests/test_hip_loop_handle.py': 'a second LatentAug and the stream lanes against the first run, bit for bit',
}


def test_file_of(trace_path):
    stem = os.path.basename(trace_path)
    for tail in ('_kernel_trace.csv', '.csv'):
        if stem.endswith(tail):
            stem = stem[:-len(tail)]
            break
    return f'tests/{stem}.py'


def read_counts(paths):
    """{kernel name: dispatches} summed over raw (one row per dispatch) or reduced (Count column) traces."""
    counts = collections.Counter()
    for p in paths:
        with open(p, newline='') as f:
            for row in csv.DictReader(f):
                name = row['Kernel_Name']
                counts[name[:-3] if name.endswith('.kd') else name] += int(row.get('Count') or 1)     # (the descriptor's name)
    return counts


def reduce_traces(paths, out):
    counts = read_counts(paths)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['Kernel_Name', 'Count'])
        for name in sorted(counts):
            w.writerow([name, counts[name]])
    print(f'{out}: {len(counts)} kernel names, {sum(counts.values())} dispatches')


def report(record, out=None):
    out = out or sys.stdout
    unreached = [m for m, e in record.items() if not e['files']]
    unjudged = [m for m, e in record.items() if e['files'] and all(f in NON_JUDGING for f in e['files'])]
    by_reading = [m for m, e in record.items() if any(isinstance(v, dict) and v.get('by_reading') for v in e['files'].values())]
    print(f'{len(record)} kernel forms; {len(unreached)} unreached; {len(unjudged)} reached by non-judging files only; '
          f'{len(by_reading)} with a file entered by reading', file=out)
    for title, ms in (('unreached', unreached), ('non-judging only', unjudged), ('by reading', by_reading)):
        for m in ms:
            print(f'  {title}: {record[m]["name"]}   [{m}]   {" ".join(sorted(record[m]["files"]))}', file=out)
    return unreached, unjudged


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('traces', nargs='*', help='kernel-trace CSVs, raw or reduced, named after their test file')
    ap.add_argument('--reduce', action='store_true', help='fold the given raw traces into one reduced CSV (-o) and stop')
    ap.add_argument('-o', '--out', default=None, help='output of --reduce, or the record to write (default tests/golden/kernel_reach.json)')
    ap.add_argument('--merge', action='store_true', help='keep the record; replace only the entries of the test files given')
    ap.add_argument('--lib', default=None, help='product library (default: the one the package loads)')
    ap.add_argument('--by-reading', nargs='*', default=[], metavar='FILE:MANGLED', help='forms an untraced file launches, by the dispatch code')
    a = ap.parse_args(argv)
    if a.reduce:
        if not (a.out and a.traces):
            ap.error('--reduce needs raw traces and -o OUT.csv')
        return reduce_traces(a.traces, a.out)

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import kernel_symbols
    from latentaugment_amd import _lib
    symbols = kernel_symbols.kernel_symbols(a.lib or _lib.LIB_PATH)
    names = kernel_symbols.demangle(symbols)
    out = a.out or RECORD
    old = json.load(open(out)) if a.merge and os.path.isfile(out) else {}

    per_file = collections.defaultdict(list)
    for p in a.traces:
        per_file[test_file_of(p)].append(p)
    read = collections.defaultdict(list)
    for item in a.by_reading:
        f, m = item.split(':', 1)
        assert m in names, f'{m} is no kernel of the library'
        read[f].append(m)
    for f in list(per_file) + list(read):
        assert os.path.isfile(os.path.join(ROOT, f)), f'{f}: no such test file'
    assert not set(per_file) & set(read), 'a file is either traced or entered by reading'
    replaced = set(per_file) | set(read)

    record = {}
    for m in symbols:
        files = {f: v for f, v in old.get(m, {}).get('files', {}).items() if f not in replaced}
        record[m] = {'name': names[m], 'files': files}
    dropped = collections.Counter()
    for f, paths in per_file.items():
        for m, n in read_counts(paths).items():
            if m in record:
                record[m]['files'][f] = n
            else:
                dropped[f] += 1
    for f, ms in read.items():
        for m in ms:
            record[m]['files'][f] = {'count': 0, 'by_reading': True}
    for e in record.values():
        e['files'] = dict(sorted(e['files'].items()))
    with open(out, 'w') as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(f'{out}: entries of {len(replaced)} test files {"merged" if a.merge else "written"}; '
          f'{sum(dropped.values())} kernel names outside the library dropped')
    unreached, unjudged = report(record)
    return 1 if unreached or unjudged else 0


if __name__ == '__main__':
    sys.exit(main())
