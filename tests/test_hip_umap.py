"""The UMAP embedding on the GPU: the la_umap_* entries at the C ABI and embedding.LatentUMAP / embed_aug_runs, against the float64
restatements of tests/umap_cases.py.

POINTWISE (budgets derived in umap_cases.py, never measured): smooth-kNN (rho bit for bit, sigma and w within their budgets), the
union graph (row_ptr and col exactly, val within its budget, wmax the exact maximum of the device's val), one epoch from given
positions and a given CSR (idle rows bit for bit), the negative rows decoded from moves and equal to the Philox restatement as
integers, three chained epochs, la_umap_layout_f64 = its epochs one by one (eager and in a captured graph).  Every bounded case
prints its measured fraction of the budget.
WHOLE RUNS through LatentUMAP on properties: a force layout is chaotic (a 2^-50 perturbation is O(10) after 50 epochs), so runs are
not compared point by point.  The thresholds are the restatement's records (umap_cases.py, re-computed by test_umap_cases_cpu.py)
minus 0.01, never a figure the device gave.

Largest measured on an MI355X, as fractions of the budgets: sigma 0.058 (the hand-made rows), w 0.19 (n 257, k 14), val 0.36 (the
chain smooth-kNN -> graph on the device; 0 where the weights are given), one epoch 0.029 (c2, the last epoch), the weighted mean of
the transform 0.046; three chained epochs at most 2.4e-3 of the chained bound; 1728 negative draws decoded, all equal.  Whole runs:
sheet 0.9972 / 0.9959 / 0.9944 (floor 0.9830, PCA at most 0.9192), blobs 0.9338 and 0.9320 (floors 0.9199 and 0.9225) with label
purity 1.0 of the fitted and of the transformed rows.  Wall time of the file: 3 s for 58 tests.
"""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import umap_cases as uc  # noqa: E402
import helpers_formats as hf  # noqa: E402
from guarded_alloc import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
LA_ERR_ARG, LA_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from latentaugment_amd import _lib
    return _lib.load()


def _p(t):
    from latentaugment_amd import _lib
    return _lib.ptr(t)


def _s():
    from latentaugment_amd import _lib
    return _lib.stream_ptr()


def _to(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(np.array(a, dtype))).to(dev)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _smooth(lib, dev, dist2, idx, n_neighbors):
    """la_umap_smooth_knn_f64 on numpy or device inputs -> (rho, sigma, w) numpy; outputs between guard bands"""
    d2 = dist2 if torch.is_tensor(dist2) else _to(dist2, np.float64, dev)
    ix = idx if torch.is_tensor(idx) else _to(idx, np.int32, dev)
    n, k = d2.shape
    g = Guarded('ones')
    rho, sigma, w = (g.tensor(s, torch.float64, dev, -7.0) for s in ([n], [n], [n, k]))
    with torch.cuda.device(dev):
        rc = lib.la_umap_smooth_knn_f64(_p(d2), _p(ix), n, k, float(np.log2(n_neighbors)), _p(rho), _p(sigma), _p(w), _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    g.check()
    return rho.cpu().numpy(), sigma.cpu().numpy(), w.cpu().numpy()


def _graph(lib, dev, idx, w, pattern='ones'):
    """la_umap_graph_f64 -> (row_ptr, col[:nnz], val[:nnz], wmax); outputs and scratch between guard bands"""
    ix, wd = _to(idx, np.int32, dev), _to(w, np.float64, dev)
    n, k = ix.shape
    nbytes = lib.la_umap_scratch_bytes(n, k)
    assert nbytes > 0
    g = Guarded(pattern)
    ws = g.alloc(nbytes, dev, torch.float64)
    cap = 2 * n * k
    row_ptr = g.tensor([n + 1], torch.int32, dev, -7)
    col = g.tensor([cap], torch.int32, dev, -7)
    val = g.tensor([cap], torch.float64, dev, -7.0)
    wmax = g.tensor([1], torch.float64, dev, -7.0)
    with torch.cuda.device(dev):
        rc = lib.la_umap_graph_f64(_p(ix), _p(wd), n, k, _p(row_ptr), _p(col), _p(val), cap, _p(wmax), _p(ws), nbytes, _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    g.check()
    row_ptr = row_ptr.cpu().numpy()
    nnz = int(row_ptr[-1])
    assert 0 <= nnz <= cap and (col[nnz:] == -7).all() and (val[nnz:] == -7.0).all()          # nothing past the end is written
    return row_ptr, col.cpu().numpy()[:nnz], val.cpu().numpy()[:nnz], float(wmax.cpu()[0])


class _Epochs:
    """a case's CSR and tails on the device, once; run(y, e) -> y' through la_umap_epoch_f64 with y' between guard bands"""

    def __init__(self, lib, dev, case):
        self.lib, self.dev, self.case = lib, dev, case
        self.row_ptr, self.col = _to(case['row_ptr'], np.int32, dev), _to(case['col'], np.int32, dev)
        self.val, self.wmax = _to(case['val'], np.float64, dev), _to([case['wmax']], np.float64, dev)
        self.yt = None if case['yt'] is None else _to(case['yt'], np.float64, dev)

    def args(self, n, n_tail, Cc):
        c = self.case
        return (n, n_tail, Cc), (_p(self.row_ptr), _p(self.col), _p(self.val), self.col.numel(), _p(self.wmax)), \
            (c['a'], c['b'], c.get('rate_now', c['rate']), c['lr'], c['seed'], c['row0'], int(c['skip_self']))

    def run(self, y, e, E=uc.EPOCH_E):
        yin = _to(y, np.float64, self.dev)
        n, Cc = yin.shape
        tail = yin if self.yt is None else self.yt
        g = Guarded('ones')
        out = g.tensor([n, Cc], torch.float64, self.dev, -7.0)
        (n_, nt, Cc_), csr, rest = self.args(n, tail.shape[0], Cc)
        with torch.cuda.device(self.dev):
            rc = self.lib.la_umap_epoch_f64(_p(yin), _p(out), n, _p(tail), nt, Cc, *csr, e, E, *rest, _s())
        torch.cuda.synchronize()
        assert rc == 0, self.lib.la_last_error()
        g.check()
        return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# smooth-kNN

def _compare_smooth(tag, got, sk):
    rho, sigma, w = got
    assert _same_bits(rho, sk['rho'])
    ex = sk['exact']
    assert _same_bits(sigma[ex], sk['sigma'][ex])
    es, ew = np.abs(sigma - sk['sigma']), np.abs(w - sk['w'])
    ne = ~ex
    fs = float((es[ne] / sk['B_sigma'][ne]).max()) if ne.any() else 0.0
    fw = float((ew / np.where(sk['B_w'] > 0, sk['B_w'], 1.0)).max())
    print(f'smooth-kNN {tag}: worst |sigma - ref| {es.max():.2e} = {fs:.4f} of its budget; worst |w - ref| {ew.max():.2e} = {fw:.4f} of its budget')
    assert (es[ne] <= sk['B_sigma'][ne]).all() and (ew <= sk['B_w']).all()


@pytest.mark.parametrize('n', uc.SMOOTH_N)
@pytest.mark.parametrize('k', uc.SMOOTH_K)
def test_smooth_knn_cases(lib, dev, n, k):
    d2, idx = uc.smooth_case(n, k)
    _compare_smooth(f'n {n} k {k}', _smooth(lib, dev, d2, idx, k + 1), uc.smooth_knn(d2, idx, k + 1))


def test_smooth_knn_special_rows(lib, dev):
    d2, idx = uc.smooth_special()
    got = _smooth(lib, dev, d2, idx, 7)
    _compare_smooth('special rows', got, uc.smooth_knn(d2, idx, 7))
    assert (got[2][0] == 1).all() and (got[2][1] == 1).all() and (got[2][3] == 0).all()


def test_smooth_knn_straight_from_la_knn(lib, dev):
    from latentaugment_amd import metrics
    x = torch.from_numpy(np.array(uc.smooth_points(257))).to(dev)
    for k in (14, 32):
        dist2, idx = metrics._knn_device(x, x, k, True)
        got = _smooth(lib, dev, dist2, idx, k + 1)
        _compare_smooth(f'la_knn_f32 output, k {k}', got, uc.smooth_knn(dist2.cpu().numpy(), idx.cpu().numpy(), k + 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# the union graph

@pytest.mark.parametrize('name', sorted(uc.graph_cases()))
def test_graph_cases(lib, dev, name):
    idx, w = uc.graph_cases()[name]
    row_ptr, col, val, wmax = _graph(lib, dev, idx, w)
    want_rp, want_col, want_val, bud = uc.graph(idx, w, np.zeros_like(w))
    assert _same_bits(row_ptr, want_rp) and _same_bits(col, want_col)
    err = np.abs(val - want_val)
    print(f'graph {name}: {len(col)} entries, longest row {int(np.diff(row_ptr).max())}, worst |val - ref| {err.max():.2e} = '
          f'{float((err / bud).max()):.4f} of its budget')
    assert (err <= bud).all() and wmax == val.max()
    n = len(idx)          # symmetric to the bit
    D = np.zeros([n, n])
    D[np.repeat(np.arange(n), np.diff(row_ptr)), col] = val
    assert (D == D.T).all()
    again = _graph(lib, dev, idx, w, pattern='bytes')          # two runs, other scratch contents: the same bits
    assert all(_same_bits(a, b) for a, b in zip((row_ptr, col, val), again[:3])) and again[3] == wmax


def test_graph_from_device_weights(lib, dev):
    """the chain smooth-kNN -> graph on the device against the restatement's chain: val within the w budgets through a + b - a b"""
    X = uc.smooth_points(257)
    d2, idx = uc.knn_exact(X, X, 14, exclude_self=True)
    sk = uc.smooth_knn(d2, idx, 15)
    _, _, w = _smooth(lib, dev, d2, idx, 15)
    row_ptr, col, val, wmax = _graph(lib, dev, idx, w)
    want_rp, want_col, want_val, bud = uc.graph(idx, sk['w'], sk['B_w'])
    err = np.abs(val - want_val)
    print(f'graph from device weights: worst |val - ref| {err.max():.2e} = {float((err / bud).max()):.4f} of its budget')
    assert _same_bits(row_ptr, want_rp) and _same_bits(col, want_col) and (err <= bud).all() and wmax == val.max()


# ---------------------------------------------------------------------------------------------------------------------------------
# initial layouts

def test_initial_layout_is_the_restatement_and_a_function_of_the_global_row(lib, dev):
    for n, Cc, row0 in ((257, 2, 0), (5, 8, 1000), (1, 1, 7), (66, 5, 3)):
        g = Guarded('ones')
        y = g.tensor([n, Cc], torch.float64, dev, -7.0)
        rc = lib.la_umap_init_f64(_p(y), n, Cc, 42, row0, _s())
        torch.cuda.synchronize()
        assert rc == 0, lib.la_last_error()
        g.check()
        assert _same_bits(y.cpu().numpy(), uc.init_layout(n, Cc, 42, row0))


def test_transform_init_weighted_mean(lib, dev):
    case = uc.epoch_case('transform')
    n, k = len(case['yh']), 4
    idx, w = case['col'].reshape(n, k), case['val'].reshape(n, k)
    Cc = case['yt'].shape[1]
    g = Guarded('ones')
    y = g.tensor([n, Cc], torch.float64, dev, -7.0)
    row_ptr = g.tensor([n + 1], torch.int32, dev, -7)
    wmax = g.tensor([1], torch.float64, dev, -7.0)
    ix, wd, bank = _to(idx, np.int32, dev), _to(w, np.float64, dev), _to(case['yt'], np.float64, dev)          # (named: they live until the sync)
    rc = lib.la_umap_transform_init_f64(_p(ix), _p(wd), n, k, _p(bank), len(case['yt']), Cc, _p(y), _p(row_ptr), _p(wmax), _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    g.check()
    ok = idx >= 0
    ww = np.where(ok, w, 0.0)
    want = (ww[:, :, None] * case['yt'][np.where(ok, idx, 0)]).sum(1) / ww.sum(1)[:, None]
    bound = (3 * k + 2) * uc.U * np.abs(case['yt']).max()          # k products and sums a side, the denominator's sums, one division
    err = np.abs(y.cpu().numpy() - want)
    print(f'transform init: worst |y - ref| {err.max():.2e} = {err.max() / bound:.4f} of its bound')
    assert (err <= bound).all() and (row_ptr.cpu().numpy() == np.arange(n + 1) * k).all() and float(wmax.cpu()[0]) == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# one epoch

@pytest.mark.parametrize('name', sorted(uc.EPOCH_CASES))
def test_one_epoch_within_its_budget(lib, dev, name):
    case = uc.epoch_case(name)
    ep = _Epochs(lib, dev, case)
    yt = case['yh'] if case['yt'] is None else case['yt']
    for e in uc.EPOCH_EPOCHS:
        got = ep.run(case['yh'], e)
        want, T, _, clipped = uc.epoch(case['yh'], yt, *uc.epoch_args(case, e), detail=True)
        bud = uc.epoch_budget(want, T, e, uc.EPOCH_E, case['lr'])
        err = np.abs(got - want)
        idle = T == 0
        print(f'epoch {name} e {e}: {int((~idle).sum())} rows moved, {clipped} components at the clip, most terms in a row {int(T.max())}, worst '
              f'|y - ref| {err.max():.2e} = {float((err / bud).max()):.4f} of its budget')
        assert np.isfinite(got).all() and (err <= bud).all()
        assert _same_bits(got[idle], case['yh'][idle])          # a row without an active entry comes back bit for bit
        assert _same_bits(got, ep.run(case['yh'], e))          # two runs


def test_negative_rows_are_the_philox_restatement(lib, dev):
    """draw m of every head row, decoded from the difference of the moves under rates m + 1 and m (umap_cases.decode_case)"""
    case = dict(uc.decode_case())
    table = uc.decode_table(case)
    n, nt = len(case['yh']), len(case['yt'])
    heads, pos = np.arange(n) + case['row0'], np.zeros([n], np.int64)
    checked = 0
    for e in (0, 7, uc.EPOCH_E - 1):
        alpha = case['lr'] * (1.0 - e / uc.EPOCH_E)
        prev = np.zeros([n])
        for m in range(12):          # groups 0, 1, 2: every word of a group
            case['rate'] = m + 1
            move = (_Epochs(lib, dev, case).run(case['yh'], e)[:, 0] - case['yh'][:, 0]) / alpha
            term = move - prev
            near = np.abs(term[:, None] - table[None, :])
            got = near.argmin(axis=1)
            assert (near.min(axis=1) < 1e-9).all()          # (the table's entries are more than 1e-4 apart)
            want = uc.negative_rows(pos, heads, e, m, nt, case['seed'])
            assert (got == want).all(), (e, m)
            prev = move
            checked += n
    print(f'negative rows: {checked} draws decoded, all equal to the restatement')


@pytest.mark.parametrize('name', ['c2', 'c8', 'star', 'transform'])
def test_three_chained_epochs(lib, dev, name):
    case = uc.epoch_case(name)
    ep = _Epochs(lib, dev, case)
    y_dev = y_ref = case['yh']
    B = 0.0
    for e in (10, 11, 12):
        y_dev = ep.run(y_dev, e)
        y_ref, T, _, _ = uc.epoch(y_ref, y_ref if case['yt'] is None else case['yt'], *uc.epoch_args(case, e), detail=True)
        B = float(uc.epoch_budget(y_ref, T, e, uc.EPOCH_E, case['lr']).max()) + 16.0 * uc.AMPLIFICATION[name] * B
        err = float(np.abs(y_dev - y_ref).max())
        print(f'chained {name} after epoch {e}: worst |y - ref| {err:.2e} = {err / B:.2e} of the chained bound {B:.2e}')
        assert err <= B


def _layout_buffers(dev, case):
    ya = _to(case['yh'], np.float64, dev)
    return ya, torch.full_like(ya, -7.0)


@pytest.mark.parametrize('name', ['c2', 'transform'])
def test_layout_gives_the_bits_of_its_epochs_eager_and_captured(lib, dev, name):
    case = uc.epoch_case(name)
    ep = _Epochs(lib, dev, case)
    e0, e1 = 5, 10
    y = case['yh']
    for e in range(e0, e1):
        y = ep.run(y, e)
    n, Cc = case['yh'].shape
    nt = n if ep.yt is None else ep.yt.shape[0]
    _, csr, rest = ep.args(n, nt, Cc)

    def call(ya, yb, which):
        return lib.la_umap_layout_f64(_p(ya), _p(yb), n, _p(ep.yt), nt, Cc, *csr, e0, e1, uc.EPOCH_E, *rest, C.byref(which), _s())
    ya, yb = _layout_buffers(dev, case)
    which = C.c_int(-1)
    with torch.cuda.device(dev):
        rc = call(ya, yb, which)
    torch.cuda.synchronize()
    assert rc == 0, lib.la_last_error()
    assert which.value == (e1 - e0) % 2 and _same_bits((ya, yb)[which.value].cpu().numpy(), y)
    ya, yb = _layout_buffers(dev, case)
    which = C.c_int(-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = call(ya, yb, which)
    assert rc == 0, lib.la_last_error()
    graph.replay()
    torch.cuda.synchronize()
    assert which.value == (e1 - e0) % 2 and _same_bits((ya, yb)[which.value].cpu().numpy(), y)


def test_refused_calls_launch_nothing(lib, dev):
    idx, w = uc.graph_cases()['knn65']
    n, k = idx.shape
    ix, wd = _to(idx, np.int32, dev), _to(w, np.float64, dev)
    need = lib.la_umap_scratch_bytes(n, k)
    g = Guarded('zeros')
    ws = torch.full([need // 8], -7.0, dtype=torch.float64, device=dev)
    row_ptr = g.tensor([n + 1], torch.int32, dev, -7)
    col = g.tensor([2 * n * k], torch.int32, dev, -7)
    val = g.tensor([2 * n * k], torch.float64, dev, -7.0)
    wmax = g.tensor([1], torch.float64, dev, -7.0)
    rc = lib.la_umap_graph_f64(_p(ix), _p(wd), n, k, _p(row_ptr), _p(col), _p(val), 2 * n * k, _p(wmax), _p(ws), need - 8, _s())
    rc2 = lib.la_umap_graph_f64(_p(ix), _p(wd), n, k, _p(row_ptr), _p(col), _p(val), 2 * n * k - 1, _p(wmax), _p(ws), need, _s())
    rc3 = lib.la_umap_graph_f64(_p(ix), _p(wd), n, 33, _p(row_ptr), _p(col), _p(val), 2 * n * k, _p(wmax), _p(ws), need, _s())
    torch.cuda.synchronize()
    g.check()
    assert (rc, rc2, rc3) == (LA_ERR_WORKSPACE, LA_ERR_ARG, LA_ERR_ARG)
    assert (ws == -7.0).all() and (row_ptr == -7).all() and (col == -7).all() and (val == -7.0).all() and (wmax == -7.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# whole runs through LatentUMAP

def test_two_fits_give_the_same_bits_and_a_batch_equals_its_rows(dev):
    from latentaugment_amd.embedding import LatentUMAP
    X, labels, Xq, lq = uc.blobs(0)
    a, b = LatentUMAP(device=dev).fit(X), LatentUMAP(device=dev).fit(X)
    assert _same_bits(a.embedding_, b.embedding_) and all(_same_bits(p, q) for p, q in zip(a.graph_, b.graph_))
    assert a.embedding_.shape == (300, 2) and a.embedding_.dtype == np.float64 and np.isfinite(a.embedding_).all()
    assert (a.a, a.b) == (uc.A_DEFAULT, uc.B_DEFAULT)
    rp, col, val = a.graph_
    want = uc.graph(*(lambda d2, idx: (idx, uc.smooth_knn(d2, idx, 15)['w']))(*uc.knn_exact(X, X, 14, exclude_self=True)))
    assert _same_bits(rp, want[0]) and _same_bits(col, want[1]) and val.shape == want[2].shape and ((val > 0) & (val < 1 + 4 * uc.U)).all()
    batch = a.transform(Xq[:9], row0=100)
    assert batch.shape == (9, 2) and np.isfinite(batch).all() and _same_bits(batch, a.transform(Xq[:9], row0=100))
    for i in range(9):
        assert _same_bits(a.transform(Xq[i:i + 1], row0=100 + i), batch[i:i + 1]), i
    assert not _same_bits(a.transform(Xq[:9], row0=0), batch)          # the draws are keyed by the global row
    # a caller's initial layout, other components
    y0 = uc.init_layout(300, 3, 5)
    c = LatentUMAP(n_components=3, n_epochs=20, init=y0, device=dev).fit_transform(X)
    assert c.shape == (300, 3) and np.isfinite(c).all() and not _same_bits(c, y0)


@pytest.mark.parametrize('seed', uc.SHEET_SEEDS)
def test_sheet_is_unrolled_as_well_as_the_restatement_does(dev, seed):
    from latentaugment_amd.embedding import LatentUMAP
    X = uc.sheet(seed)
    y = LatentUMAP(device=dev).fit_transform(X)
    t = uc.trustworthiness(X, y, 15)
    floor = min(uc.SHEET_TRUST.values()) - 0.01
    print(f'sheet {seed}: trustworthiness {t:.4f} (restatement {uc.SHEET_TRUST[seed]}, floor {floor:.4f}, PCA {uc.SHEET_TRUST_PCA[seed]})')
    assert np.isfinite(y).all() and t >= floor and t > uc.SHEET_TRUST_PCA[seed] + 0.0005


@pytest.mark.parametrize('i', range(len(uc.BLOBS)))
def test_blobs_stay_apart_and_transformed_rows_join_their_own(dev, i):
    from latentaugment_amd.embedding import LatentUMAP
    X, labels, Xq, lq = uc.blobs(i)
    um = LatentUMAP(device=dev).fit(X)
    yq = um.transform(Xq)
    t = uc.trustworthiness(X, um.embedding_, 15)
    pur, purq = uc.label_purity(um.embedding_, labels), uc.label_purity(um.embedding_, labels, 10, yq, lq)
    print(f'blobs {i}: trustworthiness {t:.4f} (restatement {uc.BLOBS_TRUST[i]}), purity {pur}, of the transformed rows {purq}')
    assert np.isfinite(um.embedding_).all() and np.isfinite(yq).all()
    assert pur == 1.0 and purq == 1.0 and t >= uc.BLOBS_TRUST[i] - 0.01


def test_package_scratch_is_guarded_and_its_contents_are_not_read(dev, monkeypatch):
    from latentaugment_amd import _lib
    from latentaugment_amd.embedding import LatentUMAP
    X, _, Xq, _ = uc.blobs(0)
    res = {}
    for pattern in ('zeros', 'ones', 'bytes'):
        g = Guarded(pattern)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'workspace', g.alloc)
            um = LatentUMAP(n_epochs=30, device=dev).fit(X)
            yq = um.transform(Xq[:5])
            torch.cuda.synchronize()
        g.check()
        assert len(g.records) == 2 + 1          # the neighbour search and the graph of the fit, the neighbour search of the transform
        res[pattern] = (um.embedding_, um.graph_[2], yq)
    for pattern in ('ones', 'bytes'):
        assert all(_same_bits(a, b) for a, b in zip(res['zeros'], res[pattern])), pattern


def test_embed_aug_runs_on_a_synthetic_zip_and_two_run_directories(dev, tmp_path):
    from latentaugment_amd.embedding import LatentUMAP, embed_aug_runs
    X, labels, _, _ = uc.blobs(0)
    X = np.array(X[:150])
    rng = np.random.default_rng(5)
    members = {f'train/p{i // 50:03d}/s_{i % 50:05d}.pickle': np.stack([rng.standard_normal(16).astype(np.float32), X[i]]) for i in range(150)}
    members['val/p900/s_00000.pickle'] = np.zeros([2, 16], np.float32)
    hf.write_zip(str(tmp_path / 'w.zip'), members)
    names = sorted(n for n in members if 'train' in n)
    W = np.stack([members[n][1] for n in names])          # the order the dataset reads them in
    runs = []
    for r in range(2):
        d = tmp_path / f'run{r}'
        (d / 'latent').mkdir(parents=True)
        (d / 'latent_aug').mkdir()
        for f in range(3):          # batches of 5: [5, 16], the dict the reference's script reads, and [5, 2, 16]
            real = W[10 * f:10 * f + 5]
            aug = (real + 0.05 * (r + 1) * rng.standard_normal(real.shape)).astype(np.float32)
            both = [np.stack([np.zeros_like(v), v], axis=1) for v in (real, aug)]
            dump = [(real, aug), ({'w': real}, {'w': aug}), both][f]
            for sub, stem, obj in (('latent', 'w', dump[0]), ('latent_aug', 'w_aug', dump[1])):
                with open(d / sub / f'{stem}_{f}', 'wb') as fh:
                    pickle.dump(obj, fh)
        runs.append(str(d))
    kw = dict(n_neighbors=10, n_epochs=200, device=dev)
    emb, lab = embed_aug_runs(str(tmp_path / 'w.zip'), 'train', runs, n_per_group=12, w_row=1, **kw)
    assert emb.shape == (36, 2) and emb.dtype == np.float64 and np.isfinite(emb).all()
    assert lab.tolist() == [0] * 12 + [1] * 12 + [2] * 12
    fitted = LatentUMAP(**kw).fit(W).embedding_
    src = np.array([0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 20, 21])          # the zip rows the 12 real codes are copies of
    # a real row lands in the neighbourhood of its own fitted position: every fitted point at least as near to it as that position
    # carries its cluster's label, and so do the 10 nearest.  (The restatement puts the own position at rank 0 .. 23 of the cluster's
    # 50: the transformed row moves for 66 epochs among its cluster, so "among the 10 nearest" is not what the method gives.)
    lab150 = labels[:150]
    d2 = ((emb[:12, None, :] - fitted[None, :, :]) ** 2).sum(-1)
    nearest = np.argsort(d2, axis=1, kind='stable')[:, :10]
    for i in range(12):
        assert (lab150[d2[i] <= d2[i, src[i]]] == lab150[src[i]]).all(), i
    assert (lab150[nearest] == lab150[src][:, None]).all()
    # and the augmented codes of both runs stay with their sources' clusters
    for grp in (1, 2):
        d2 = ((emb[12 * grp:12 * grp + 12, None, :] - fitted[None, :, :]) ** 2).sum(-1)
        assert (lab150[np.argsort(d2, axis=1, kind='stable')[:, :10]] == lab150[src][:, None]).all()
