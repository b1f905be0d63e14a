"""Every kernel form the library ships has a GPU test file that launches it and judges its values.

tests/golden/kernel_reach.json records, per mangled kernel symbol of the product library, which GPU test files dispatched it in a
kernel trace of that file (scripts/kernel_reach.py writes it; DESIGN.md 'Kernel reach' says how to refresh it).  Here, without a GPU:
the kernel symbols of the built library (tests/kernel_symbols.py) must be exactly the record's keys, and every key needs one
reaching file that exists, is a GPU test file, and judges values -- not one of scripts.kernel_reach.NON_JUDGING, which compare HIP
with HIP or check bands.  A new template instantiation therefore fails here until a float64 case launches it and the record says so."""
import json
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_symbols  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'kernel_reach.json')

# GPU test files that could not be traced when the record was made: only their forms may stand in the record by reading of the
# dispatch code ("by_reading": true) instead of by a traced dispatch count.  Every file was traced.
UNTRACED_FILES = ()


@pytest.fixture(scope='module')
def symbols(tmp_path_factory):
    from latentaugment_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    if not kernel_symbols.tools_present():
        pytest.skip('LLVM tools of the ROCm image not found')
    return kernel_symbols.kernel_symbols(_lib.LIB_PATH, tmp_path_factory.mktemp('code_objects'))


@pytest.fixture(scope='module')
def record():
    return json.load(open(RECORD))


def test_symbol_helper_finds_the_kernels(symbols):
    names = kernel_symbols.demangle(symbols)
    assert len(symbols) == len(set(symbols)) > 100 and symbols == sorted(symbols)
    assert all(s.startswith('_Z') or re.fullmatch(r'\w+', s) for s in symbols)
    text = '\n'.join(names.values())
    for kernel in ('la_pm_level_kernel<9, true>', 'la_pm_level_kernel<9, false>', 'la_pm_finish_kernel', 'la_joint_hist_kernel'):
        assert kernel in text, kernel
    assert not any(s.endswith('.kd') for s in symbols)


def test_record_lists_exactly_the_built_kernel_forms(symbols, record):
    names = kernel_symbols.demangle(symbols)
    new = [m for m in symbols if m not in record]
    stale = [m for m in record if m not in set(symbols)]
    msg = [f'new kernel form `{names[m]}`: add a float64 case and re-record (scripts/kernel_reach.py --merge)' for m in new]
    msg += [f'stale record key `{record[m]["name"]}` [{m}]: the library no longer has this kernel form; re-record '
            f'(scripts/kernel_reach.py --merge)' for m in stale]
    assert not msg, '\n'.join(msg)
    for m in symbols:
        assert record[m]['name'] == names[m], m


def _is_gpu_test_file(rel):
    path = os.path.join(ROOT, rel)
    return bool(re.fullmatch(r'tests/test_\w+\.py', rel)) and os.path.isfile(path) and 'pytest.mark.gpu' in open(path).read()


def test_every_form_is_reached_by_a_judging_gpu_test_file(record):
    from scripts import kernel_reach
    for f in kernel_reach.NON_JUDGING:
        assert _is_gpu_test_file(f), f'{f}: listed as non-judging but no GPU test file'
    bad = []
    for m, e in sorted(record.items()):
        files = e['files']
        for f, v in files.items():
            n = v['count'] if isinstance(v, dict) else v
            by_reading = isinstance(v, dict) and v.get('by_reading') is True
            if not (isinstance(n, int) and (n > 0 or (by_reading and n == 0))):
                bad.append(f'{e["name"]}: dispatch count {v!r} of {f}')
        judges = [f for f in files if _is_gpu_test_file(f) and f not in kernel_reach.NON_JUDGING]
        if not judges:
            bad.append(f'{e["name"]} [{m}]: no judging GPU test file reaches it (files: {sorted(files) or "none"})')
    assert not bad, '\n'.join(bad)


def test_forms_entered_by_reading_belong_to_the_untraced_files(record):
    read = [(e['name'], f) for m, e in sorted(record.items()) for f, v in e['files'].items() if isinstance(v, dict) and v.get('by_reading')]
    for name, f in read:
        print(f'by reading: {name} <- {f}')
    outside = [(name, f) for name, f in read if f not in UNTRACED_FILES]
    assert not outside, f'entered by reading although their file is not among the untraced ones {UNTRACED_FILES}: {outside}'


def test_reach_tool_maps_traces_and_reports(tmp_path, symbols, monkeypatch, capsys):
    """scripts/kernel_reach.py on two made-up traces: raw rows and reduced rows count alike, names outside the library are dropped, --merge
    replaces the entries of the given file only, and the report names the unreached and the non-judging-only forms."""
    from latentaugment_amd import _lib
    from scripts import kernel_reach
    a, b, c = symbols[0], symbols[1], symbols[2]
    raw = tmp_path / 'test_hip_pair_metrics_kernel_trace.csv'
    raw.write_text('"Kind","Kernel_Name"\n' + f'"KERNEL_DISPATCH","{a}.kd"\n' * 3 + f'"KERNEL_DISPATCH","{b}"\n' + '"KERNEL_DISPATCH","rocblas_thing"\n')
    red = tmp_path / 'test_hip_history.csv'
    kernel_reach.main(['--reduce', str(raw), '-o', str(red)])
    assert red.read_text().splitlines() == ['Kernel_Name,Count', f'{a},3', f'{b},1', 'rocblas_thing,1']
    red.write_text(f'Kernel_Name,Count\n{b},5\n{c},2\n')
    out = tmp_path / 'record.json'
    rc = kernel_reach.main(['--lib', _lib.LIB_PATH, '-o', str(out), str(raw), str(red)])
    rec = json.load(open(out))
    assert rc == 1 and sorted(rec) == symbols
    assert rec[a]['files'] == {'tests/test_hip_pair_metrics.py': 3}
    assert rec[b]['files'] == {'tests/test_hip_history.py': 5, 'tests/test_hip_pair_metrics.py': 1}
    assert rec[c]['files'] == {'tests/test_hip_history.py': 2} and 'rocblas_thing' not in rec
    text = capsys.readouterr().out
    assert f'{len(symbols)} kernel forms; {len(symbols) - 3} unreached; 1 reached by non-judging files only' in text
    assert f'non-judging only: {rec[c]["name"]}' in text
    raw.write_text(f'Kernel_Name,Count\n{c},7\n')
    kernel_reach.main(['--lib', _lib.LIB_PATH, '-o', str(out), '--merge', str(raw)])
    rec = json.load(open(out))
    assert rec[a]['files'] == {} and rec[b]['files'] == {'tests/test_hip_history.py': 5}
    assert rec[c]['files'] == {'tests/test_hip_history.py': 2, 'tests/test_hip_pair_metrics.py': 7}
