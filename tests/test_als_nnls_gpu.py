"""GPU tests of the nonnegative ALS half-step (csrc/als_nnls.hip): per row
the minimiser of 1/2 x'Ax - b'x over x >= 0 by block principal pivoting,
one wave per row (f <= 64), one workgroup per row (f = 128), and behind the
split-row Gramians for heavy rows.

Every case solves with als_solve(nonnegative=True) into a NaN-prefilled
buffer with guard rows and compares with als_solve_nnls_ref in float64 on
the CPU, and checks the KKT conditions of the returned X in float64."""

import functools

import pytest
import torch

from _als_solve_oracle import ALPHA, LAM, TOL, _csr, _factors

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEGREES = [0, 1, 5, 20, 31, 32, 33, 48, 49, 63, 64, 65, 100, 300]
GUARD = 64
# KKT residual bound, relative to |b|_inf. The unconstrained als_solve
# leaves max |A x - b| / |b|_inf = KKT_MEASURED against its own float64
# system on the problems of test_every_shape (all 16 cases, rows of every
# degree; scripts/als_nnls_probe.py residual prints it); the bound is 4x
# that, the margin test_als_wide_woodbury_gpu.py uses between kernels.
KKT_MEASURED = 3.41e-6
KKT_TOL = 4 * KKT_MEASURED


def _ref64(indptr, cols, vals, Y, implicit):
    from predictionio_amd.ops import als as als_ops
    Yd = Y.double()
    return als_ops.als_solve_nnls_ref(indptr, cols, vals.double(), Yd,
                                      als_ops.gramian(Yd), LAM, ALPHA,
                                      implicit)


@functools.lru_cache(maxsize=None)
def shape_problem(f, implicit, abs_y):
    g = torch.Generator().manual_seed(8100 + f)
    perm = torch.randperm(len(DEGREES), generator=g).tolist()
    sizes = DEGREES + [DEGREES[i] for i in perm]
    indptr, cols, vals = _csr(sizes, g)
    Y = _factors(f, g)
    Y = Y.abs() if abs_y else Y
    return sizes, indptr, cols, vals, Y, _ref64(indptr, cols, vals, Y,
                                                implicit)


def _solve_guarded(indptr, cols, vals, Y, implicit, pieces=None, **kw):
    """Solve into the middle of a NaN buffer, whole or in row_range
    pieces; returns (X, guards_untouched)."""
    from predictionio_amd.ops import als as als_ops
    n_rows, f = indptr.shape[0] - 1, Y.shape[1]
    buf = torch.full((n_rows + 2 * GUARD, f), float("nan"), device="cuda")
    out = buf[GUARD:GUARD + n_rows]
    dev = (indptr.cuda(), cols.cuda(), vals.cuda(), Y.cuda())
    for lo, hi in (pieces or [(0, n_rows)]):
        als_ops.als_solve(*dev, lam=LAM, alpha=ALPHA, implicit=implicit,
                          row_range=(lo, hi), out=out[lo:hi], **kw)
    buf = buf.cpu()
    guards = torch.cat([buf[:GUARD], buf[GUARD + n_rows:]])
    return buf[GUARD:GUARD + n_rows].clone(), bool(torch.isnan(guards).all())


def _check(X, guards, indptr, cols, vals, Y, implicit, X64, what):
    from predictionio_amd.ops import als as als_ops
    assert guards, f"{what}: guard rows written"
    assert not torch.isnan(X).any(), f"{what}: rows left NaN"
    assert (X >= 0).all() and not torch.signbit(X).any(), f"{what}: sign"
    Yd = Y.double()
    YtY = als_ops.gramian(Yd)
    worst_on = worst_off = 0.0
    for r in range(X.shape[0]):
        A, b = als_ops.normal_equations(indptr, cols, vals, Yd, YtY, LAM,
                                        ALPHA, implicit, not implicit, r)
        s = b.abs().max().item()
        if s == 0:
            assert not X[r].any()
            continue
        g = (A @ X[r].double() - b) / s
        on = X[r] > 0
        worst_on = max(worst_on, g[on].abs().max().item() if on.any() else 0)
        worst_off = max(worst_off,
                        -g[~on].min().item() if (~on).any() else 0)
    diff = (X.double() - X64).abs().max().item()
    print(f"{what}: max abs diff {diff:.3e}, KKT |g| on support "
          f"{worst_on:.3e}, -min g off it {worst_off:.3e} (of |b|_inf)")
    assert worst_on <= KKT_TOL and worst_off <= KKT_TOL, what
    assert torch.allclose(X.double(), X64, atol=TOL, rtol=TOL), what


@requires_gpu
@pytest.mark.parametrize("abs_y", [False, True])
@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("f", [10, 32, 64, 128])
def test_every_shape(f, implicit, abs_y):
    sizes, indptr, cols, vals, Y, X64 = shape_problem(f, implicit, abs_y)
    iters = torch.full((len(sizes),), -1, dtype=torch.int32, device="cuda")
    X, guards = _solve_guarded(indptr, cols, vals, Y, implicit,
                               nonnegative=True, nnls_iters=iters)
    print(f"trips per row: max {int(iters.max())} of {sizes}")
    _check(X, guards, indptr, cols, vals, Y, implicit, X64,
           f"f={f} implicit={implicit} abs_y={abs_y}")


@requires_gpu
@pytest.mark.parametrize("implicit", [False, True])
def test_heavy_rows_and_call_shape(implicit, monkeypatch):
    from predictionio_amd.ops import als as als_ops
    monkeypatch.setenv("PIO_ALS_HEAVY_MIN", "64")
    monkeypatch.setenv("PIO_ALS_HEAVY_CHUNK", "64")
    sizes = [65, 20, 129, 100, 1000, 0]
    g = torch.Generator().manual_seed(8200)
    indptr, cols, vals = _csr(sizes, g)
    Y = _factors(64, g)
    X64 = _ref64(indptr, cols, vals, Y, implicit)
    args = (indptr, cols, vals, Y, implicit)
    before = als_ops.heavy_stats()
    whole, guards = _solve_guarded(*args, nonnegative=True)
    after = als_ops.heavy_stats()
    assert [after[k] - before[k] for k in ("calls", "rows", "chunks")] == \
        [1, 4, 2 + 3 + 2 + 16]
    _check(whole, guards, *args, X64, f"heavy implicit={implicit}")
    again, _ = _solve_guarded(*args, nonnegative=True)
    parts, guards = _solve_guarded(*args, pieces=[(0, 3), (3, 4), (4, 6)],
                                   nonnegative=True)
    assert guards
    monkeypatch.setenv("PIO_ALS_HEAVY_WS_MB", "0.05")   # three slots
    small, guards = _solve_guarded(*args, nonnegative=True)
    assert guards
    for other in (again, parts, small):
        assert torch.equal(whole.view(torch.int32), other.view(torch.int32))


@requires_gpu
@pytest.mark.parametrize("f", [64, 128])
def test_bound_is_a_bound(f):
    """Explicit mode, |Y|. Row 0 has one positive rating: its unconstrained
    solution is positive, so every coordinate is passive. Row 64 has only
    negative ratings: b <= 0 and x = 0 with no solve. Rows 64 apart belong
    to different waves; the 100-entry rows around them keep both busy."""
    from predictionio_amd.ops import als as als_ops
    sizes = [1] + [100] * 63 + [5] + [100] * 3
    g = torch.Generator().manual_seed(8300 + f)
    indptr, cols, vals = _csr(sizes, g, vals_of={64: -torch.ones(5)})
    Y = _factors(f, g).abs()
    X64 = _ref64(indptr, cols, vals, Y, False)
    iters = torch.full((len(sizes),), -1, dtype=torch.int32, device="cuda")
    X, guards = _solve_guarded(indptr, cols, vals, Y, False,
                               nonnegative=True, nnls_iters=iters)
    _check(X, guards, indptr, cols, vals, Y, False, X64, f"bound f={f}")
    free, _ = _solve_guarded(indptr, cols, vals, Y, False)
    assert (X[0] > 0).all()
    assert torch.allclose(X[0], free[0], atol=TOL, rtol=TOL)
    iters = iters.cpu()
    print(f"f={f} trips: max {int(iters.max())} mean "
          f"{iters.float().mean():.2f}")
    assert not X[64].any() and iters[64] == 0 and iters[0] == 1
    assert iters.min() >= 0 and iters.max() < als_ops.NNLS_REF_MAX_IT


@requires_gpu
@pytest.mark.parametrize("implicit", [False, True])
def test_off_means_off(implicit):
    from predictionio_amd.models.als import ALSParams, train_als
    from predictionio_amd.ops import als as als_ops
    sizes, indptr, cols, vals, Y, _ = shape_problem(64, implicit, False)
    default, _ = _solve_guarded(indptr, cols, vals, Y, implicit)
    off, _ = _solve_guarded(indptr, cols, vals, Y, implicit,
                            nonnegative=False)
    assert torch.equal(default.view(torch.int32), off.view(torch.int32))
    before = als_ops.nnls_stats()
    g = torch.Generator().manual_seed(5)
    key = torch.randperm(60 * 40, generator=g)[:600]
    params = ALSParams(rank=8, iterations=2, implicit=implicit, seed=1)
    train_als(key // 40, key % 40, torch.rand(600, generator=g) + 0.5, 60,
              40, params, torch.device("cuda"))
    assert als_ops.nnls_stats() == before
    params.nonnegative = True
    X, Y2 = train_als(key // 40, key % 40, torch.rand(600, generator=g) + 0.5,
                      60, 40, params, torch.device("cuda"))
    assert als_ops.nnls_stats()["calls"] == before["calls"] + 4
    assert (X >= 0).all() and (Y2 >= 0).all()
