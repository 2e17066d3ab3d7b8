"""GPU tests for the wide Woodbury variants (als_woodbury_kernel<F, 40, 32>
and <F, 48, 40>, F in {64, 128}) and for the 64-row block scan by which
the one-wave-per-row solvers find their rows.

Every case solves on the GPU with als_ops.als_solve into a buffer
prefilled with NaN and compares with als_ops.als_solve_ref in float64 on
the CPU (tests/_als_solve_oracle.py: Y = randn / sqrt(f), values in
[0.5, 3.5), lam = 0.05, alpha = 2.0, 400 columns).

PIO_ALS_WOODBURY_MAX=32 keeps rows of degree 33..48 on the dense kernels;
the launcher reads it on every call, so both routes run in one process.
"""

import functools

import pytest
import torch

from _als_solve_oracle import (
    ALPHA, LAM, N_COLS, TOL, _csr, _factors, _ref64,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

# every degree across the seams at 32 | 33, 40 | 41 and 48 | 49, plus the
# dense kernel around its 64-lane width and one long row
DEGREES = list(range(51)) + [63, 64, 65, 100]
GUARD = 64   # NaN rows kept before and after every output buffer


def _solve_guarded(indptr, cols, vals, Y, implicit, chunks=None):
    """Solve into the middle of a NaN buffer with GUARD rows on either
    side, whole or in row_range chunks; returns (X, guards_untouched)."""
    from predictionio_amd.ops import als as als_ops
    n_rows, f = indptr.shape[0] - 1, Y.shape[1]
    buf = torch.full((n_rows + 2 * GUARD, f), float("nan"), device="cuda")
    out = buf[GUARD:GUARD + n_rows]
    dev = (indptr.cuda(), cols.cuda(), vals.cuda(), Y.cuda())
    for lo, hi in (chunks or [(0, n_rows)]):
        als_ops.als_solve(*dev, lam=LAM, alpha=ALPHA, implicit=implicit,
                          row_range=(lo, hi), out=out[lo:hi])
    buf = buf.cpu()
    guards = torch.cat([buf[:GUARD], buf[GUARD + n_rows:]])
    return buf[GUARD:GUARD + n_rows].clone(), bool(torch.isnan(guards).all())


def _check(X, X64, sizes, what):
    bad = sorted({sizes[r] for r in range(len(sizes))
                  if not torch.isfinite(X[r]).all()})
    diff = (X.double() - X64).abs().max().item() if not bad else float("nan")
    print(f"{what}: max abs diff {diff:.3e}")
    assert not bad, f"{what}: rows left NaN or non-finite, degrees {bad}"
    assert torch.allclose(X.double(), X64, atol=TOL, rtol=TOL), \
        f"{what}: max abs diff {diff}"


@functools.lru_cache(maxsize=None)
def seam_problem(f, implicit):
    """DEGREES ascending, then in a seeded shuffle (as every_degree_problem
    does), with the float64 reference; computed once and shared."""
    g = torch.Generator().manual_seed(4242 + f)
    perm = torch.randperm(len(DEGREES), generator=g).tolist()
    sizes = DEGREES + [DEGREES[i] for i in perm]
    indptr, cols, vals = _csr(sizes, g)
    Y = _factors(f, g)
    return sizes, indptr, cols, vals, Y, _ref64(indptr, cols, vals, Y, LAM,
                                                implicit)


@requires_gpu
@pytest.mark.parametrize("f", [64, 128])
@pytest.mark.parametrize("implicit", [False, True])
def test_every_degree_across_wide_seams(f, implicit):
    sizes, indptr, cols, vals, Y, X64 = seam_problem(f, implicit)
    X, guards = _solve_guarded(indptr, cols, vals, Y, implicit)
    _check(X, X64, sizes, f"f={f} implicit={implicit}")
    assert guards


@requires_gpu
@pytest.mark.parametrize("implicit", [False, True])
def test_knob_keeps_dense_route(implicit, monkeypatch):
    """PIO_ALS_WOODBURY_MAX=32: rows 33..48 go back to the dense kernel
    and every row is still right."""
    monkeypatch.setenv("PIO_ALS_WOODBURY_MAX", "32")
    sizes, indptr, cols, vals, Y, X64 = seam_problem(64, implicit)
    X, guards = _solve_guarded(indptr, cols, vals, Y, implicit)
    _check(X, X64, sizes, f"knob=32 implicit={implicit}")
    assert guards


@requires_gpu
@pytest.mark.parametrize("f", [64, 128])
@pytest.mark.parametrize("implicit", [False, True])
def test_wide_route_no_less_accurate(f, implicit, monkeypatch):
    """Rows of degree 33..48: the wide route's relative Frobenius error
    against float64 is at most 4x the dense route's (the margin
    test_als_optin_gpu.py uses between kernels). Both are about 3e-7 in an
    fp32 emulation; a wrong lane or a stale row costs orders of magnitude.
    """
    sizes, indptr, cols, vals, Y, X64 = seam_problem(f, implicit)
    rows = torch.tensor([r for r, n in enumerate(sizes) if 33 <= n <= 48])
    assert len(rows) == 32

    def err(X):
        assert torch.isfinite(X[rows]).all()
        return ((X[rows].double() - X64[rows]).norm()
                / X64[rows].norm()).item()

    wide = err(_solve_guarded(indptr, cols, vals, Y, implicit)[0])
    monkeypatch.setenv("PIO_ALS_WOODBURY_MAX", "32")
    dense = err(_solve_guarded(indptr, cols, vals, Y, implicit)[0])
    print(f"f={f} implicit={implicit} rows 33..48 rel fro: wide "
          f"{wide:.4e} dense {dense:.4e} ratio {wide / dense:.2f}")
    assert wide <= 4.0 * dense


@requires_gpu
@pytest.mark.parametrize("f", [64, 128])
@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("long_n,short_n", [(48, 33), (40, 33), (48, 41)])
def test_stale_lds_rows(long_n, short_n, f, implicit):
    """256 rows alternating a long and a short degree. The long rows draw
    their columns from factor rows that no short row uses and that are
    scaled by 64, so staged rows left over from a long row would swamp a
    short row that read them. (40, 33) and (48, 41) share one
    instantiation, so a wave solves a long and a short row back to back;
    (48, 33) splits the block between the two wide instantiations."""
    g = torch.Generator().manual_seed(99 + long_n + short_n)
    sizes = [long_n, short_n] * 128
    half = N_COLS // 2
    cols_of = {
        r: (torch.randint(half, N_COLS, (n,), generator=g) if n == long_n
            else torch.randint(0, half, (n,), generator=g))
        for r, n in enumerate(sizes)}
    indptr, cols, vals = _csr(sizes, g, cols_of=cols_of)
    Y = _factors(f, g)
    Y[half:] *= 64.0
    X64 = _ref64(indptr, cols, vals, Y, LAM, implicit)
    X, guards = _solve_guarded(indptr, cols, vals, Y, implicit)
    _check(X, X64, sizes, f"{long_n}/{short_n} f={f} implicit={implicit}")
    assert guards


POOL = [0, 19, 20, 21, 24, 25, 32, 33, 40, 41, 48, 49, 70]


@functools.lru_cache(maxsize=None)
def scan_problem(n_rows, sparse, implicit):
    """Degrees drawn from POOL; `sparse`: about one row in 200 has degree
    > 32, so most 64-row blocks are empty for most kernels."""
    g = torch.Generator().manual_seed(31 * n_rows + sparse)
    pool = torch.tensor(POOL)
    if sparse:
        low = pool[pool <= 32]
        high = pool[pool > 32]
        sizes = low[torch.randint(0, len(low), (n_rows,), generator=g)]
        pick = torch.rand(n_rows, generator=g) < 1.0 / 200
        sizes[pick] = high[torch.randint(0, len(high), (int(pick.sum()),),
                                         generator=g)]
        assert 5 <= int(pick.sum()) <= n_rows // 50
    else:
        sizes = pool[torch.randint(0, len(pool), (n_rows,), generator=g)]
    sizes = sizes.tolist()
    indptr, cols, vals = _csr(sizes, g)
    Y = _factors(64, g)
    return sizes, indptr, cols, vals, Y, _ref64(indptr, cols, vals, Y, LAM,
                                                implicit)


@requires_gpu
@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("n_rows,sparse", [
    (1, False), (63, False), (64, False), (65, False), (129, False),
    (5000, False), (4000, True)])
def test_block_scan_edges(n_rows, sparse, implicit):
    """Row counts around the 64-row block, whole and in three row_range
    chunks whose bounds are no multiples of 64: every row right, nothing
    written outside the rows asked for, the same bits either way."""
    sizes, indptr, cols, vals, Y, X64 = scan_problem(n_rows, sparse,
                                                     implicit)
    whole, guards = _solve_guarded(indptr, cols, vals, Y, implicit)
    _check(whole, X64, sizes, f"n_rows={n_rows} sparse={sparse} whole")
    assert guards, "guard rows overwritten (whole)"
    cuts = sorted({0, n_rows // 3, 2 * n_rows // 3, n_rows})
    assert all(c % 64 for c in cuts[1:-1])
    chunks = list(zip(cuts[:-1], cuts[1:]))
    parts, guards = _solve_guarded(indptr, cols, vals, Y, implicit,
                                   chunks=chunks)
    assert guards, "guard rows overwritten (chunked)"
    assert torch.isfinite(parts).all()
    ndiff = (whole.view(torch.int32) != parts.view(torch.int32)).sum().item()
    print(f"chunks {chunks}: {ndiff} differing words")
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))
