"""GPU tests for the split-row ALS route (csrc/als_heavy.hip): rows of
degree > PIO_ALS_HEAVY_MIN are cut into chunks of PIO_ALS_HEAVY_CHUNK
entries, one workgroup forms each chunk's partial normal equations on fp32
MFMA, and one workgroup per row adds them in chunk order and solves.

Every case solves with als_ops.als_solve on the GPU into a NaN-prefilled
buffer with guard rows and compares with als_solve_ref in float64 on the
CPU (tests/_als_solve_oracle.py). The knobs are read on every call, so the
routes run side by side in one process.
"""

import functools

import pytest
import torch

from _als_solve_oracle import ALPHA, LAM, TOL, _csr, _factors, _ref64

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

HMIN, CHUNK = 64, 64
# one entry into the second chunk, a half tile, the chunk seam on both
# sides, a 16-chunk reduce
HEAVY = [65, 96, 127, 128, 129, 1000]
# empty, Woodbury, Woodbury, dense (the last degree that is not heavy) and
# one more heavy row: 129 | 100 | 1000 are three heavy rows in a row
LIGHT = [0, 20, 40, 64, 100]
GUARD = 64


def _sizes(seed):
    asc = [n for pair in zip(HEAVY, LIGHT) for n in pair] + HEAVY[-1:]
    perm = torch.randperm(
        len(asc), generator=torch.Generator().manual_seed(seed)).tolist()
    return asc + [asc[i] for i in perm]


def _expected_counts(sizes, hmin, chunk):
    heavy = [n for n in sizes if n > hmin]
    return len(heavy), sum((n + chunk - 1) // chunk for n in heavy)


@functools.lru_cache(maxsize=None)
def heavy_problem(f, implicit):
    g = torch.Generator().manual_seed(7100 + f)
    sizes = _sizes(7100 + f)
    indptr, cols, vals = _csr(sizes, g)
    Y = _factors(f, g)
    return sizes, indptr, cols, vals, Y, _ref64(indptr, cols, vals, Y, LAM,
                                                implicit)


def _solve_guarded(indptr, cols, vals, Y, implicit, pieces=None):
    """Solve into the middle of a NaN buffer, whole or in row_range
    pieces; returns (X, guards_untouched, growth of heavy_stats)."""
    from predictionio_amd.ops import als as als_ops
    n_rows, f = indptr.shape[0] - 1, Y.shape[1]
    buf = torch.full((n_rows + 2 * GUARD, f), float("nan"), device="cuda")
    out = buf[GUARD:GUARD + n_rows]
    dev = (indptr.cuda(), cols.cuda(), vals.cuda(), Y.cuda())
    before = als_ops.heavy_stats()
    for lo, hi in (pieces or [(0, n_rows)]):
        als_ops.als_solve(*dev, lam=LAM, alpha=ALPHA, implicit=implicit,
                          row_range=(lo, hi), out=out[lo:hi])
    after = als_ops.heavy_stats()
    buf = buf.cpu()
    guards = torch.cat([buf[:GUARD], buf[GUARD + n_rows:]])
    return (buf[GUARD:GUARD + n_rows].clone(),
            bool(torch.isnan(guards).all()),
            {k: after[k] - before[k] for k in after})


def _check(X, X64, what):
    diff = (X.double() - X64).abs().max().item()
    print(f"{what}: max abs diff {diff:.3e}")
    assert torch.isfinite(X).all(), f"{what}: rows left NaN"
    assert torch.allclose(X.double(), X64, atol=TOL, rtol=TOL), \
        f"{what}: max abs diff {diff}"


@pytest.fixture
def small_knobs(monkeypatch):
    monkeypatch.setenv("PIO_ALS_HEAVY_MIN", str(HMIN))
    monkeypatch.setenv("PIO_ALS_HEAVY_CHUNK", str(CHUNK))


@requires_gpu
@pytest.mark.parametrize("f", [10, 32, 64, 128])
@pytest.mark.parametrize("implicit", [False, True])
def test_seams(f, implicit, small_knobs):
    sizes, indptr, cols, vals, Y, X64 = heavy_problem(f, implicit)
    X, guards, grew = _solve_guarded(indptr, cols, vals, Y, implicit)
    n_heavy, n_chunks = _expected_counts(sizes, HMIN, CHUNK)
    assert (grew["calls"], grew["rows"], grew["chunks"]) == \
        (1, n_heavy, n_chunks)
    _check(X, X64, f"f={f} implicit={implicit}")
    assert guards


@requires_gpu
@pytest.mark.parametrize("implicit", [False, True])
def test_independent_of_call_shape(implicit, small_knobs):
    """Whole, whole again, and in row_range pieces cut on both sides of
    the middle one of three adjacent heavy rows: the same bits."""
    sizes, indptr, cols, vals, Y, X64 = heavy_problem(64, implicit)
    k = len(HEAVY) + len(LIGHT) - 2
    assert sizes[k - 1:k + 2] == [129, 100, 1000]
    whole, guards, _ = _solve_guarded(indptr, cols, vals, Y, implicit)
    assert guards
    again, _, _ = _solve_guarded(indptr, cols, vals, Y, implicit)
    parts, guards, grew = _solve_guarded(
        indptr, cols, vals, Y, implicit,
        pieces=[(0, k), (k, k + 1), (k + 1, len(sizes))])
    assert guards
    assert grew["rows"] == _expected_counts(sizes, HMIN, CHUNK)[0]
    _check(whole, X64, f"implicit={implicit} whole")
    assert torch.equal(whole.view(torch.int32), again.view(torch.int32))
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))


@requires_gpu
@pytest.mark.parametrize("implicit", [False, True])
def test_workspace_batches(implicit, small_knobs, monkeypatch):
    """A workspace of three slots: rows are cut by batch boundaries and
    carry their running sums across; the same bits as in one batch."""
    sizes, indptr, cols, vals, Y, X64 = heavy_problem(64, implicit)
    whole, _, _ = _solve_guarded(indptr, cols, vals, Y, implicit)
    monkeypatch.setenv("PIO_ALS_HEAVY_WS_MB", "0.05")   # 3 slots at f = 64
    small, guards, _ = _solve_guarded(indptr, cols, vals, Y, implicit)
    assert guards
    _check(small, X64, f"implicit={implicit} three slots")
    assert torch.equal(whole.view(torch.int32), small.view(torch.int32))


@requires_gpu
@pytest.mark.parametrize("f", [64, 128])
@pytest.mark.parametrize("implicit", [False, True])
def test_no_less_accurate_than_one_unit_per_row(f, implicit, small_knobs,
                                                monkeypatch):
    """Heavy rows: the relative Frobenius error against float64 is at most
    4x that of the one-unit-per-row kernels (PIO_ALS_HEAVY_MIN=0), the
    margin test_als_wide_woodbury_gpu.py uses between kernels."""
    sizes, indptr, cols, vals, Y, X64 = heavy_problem(f, implicit)
    rows = torch.tensor([r for r, n in enumerate(sizes) if n > HMIN])

    def err(X):
        assert torch.isfinite(X[rows]).all()
        return ((X[rows].double() - X64[rows]).norm()
                / X64[rows].norm()).item()

    on = err(_solve_guarded(indptr, cols, vals, Y, implicit)[0])
    monkeypatch.setenv("PIO_ALS_HEAVY_MIN", "0")
    X, _, grew = _solve_guarded(indptr, cols, vals, Y, implicit)
    off = err(X)
    assert grew["rows"] == 0
    print(f"f={f} implicit={implicit} heavy rows rel fro: on {on:.4e} "
          f"off {off:.4e} ratio {on / off:.2f}")
    assert on <= 4.0 * off


@requires_gpu
@pytest.mark.parametrize("implicit", [False, True])
def test_defaults(implicit, monkeypatch):
    from predictionio_amd.ops import als as als_ops
    monkeypatch.delenv("PIO_ALS_HEAVY_MIN", raising=False)
    monkeypatch.delenv("PIO_ALS_HEAVY_CHUNK", raising=False)
    assert als_ops.heavy_min() >= 256 and als_ops.heavy_chunk() % 32 == 0
    g = torch.Generator().manual_seed(7200)
    sizes = [20] * 100 + [4 * als_ops.heavy_min()] + [20] * 100
    indptr, cols, vals = _csr(sizes, g)
    Y = _factors(64, g)
    X64 = _ref64(indptr, cols, vals, Y, LAM, implicit)
    X, guards, grew = _solve_guarded(indptr, cols, vals, Y, implicit)
    assert grew["rows"] == 1
    _check(X, X64, f"defaults implicit={implicit}")
    assert guards


@requires_gpu
@pytest.mark.parametrize("implicit", [False, True])
def test_edge_values(implicit, small_knobs):
    """A heavy row whose values are all 0 (implicit mode: w_a = 0, the
    normal matrix is YtY + lam I alone) and one that repeats one column."""
    g = torch.Generator().manual_seed(7300)
    sizes = [200, 20, 200, 0]
    indptr, cols, vals = _csr(
        sizes, g, cols_of={2: torch.full((200,), 11)},
        vals_of={0: torch.zeros(200)} if implicit else None)
    Y = _factors(64, g)
    X64 = _ref64(indptr, cols, vals, Y, LAM, implicit)
    X, guards, grew = _solve_guarded(indptr, cols, vals, Y, implicit)
    assert grew["rows"] == 2
    _check(X, X64, f"edge values implicit={implicit}")
    assert guards
