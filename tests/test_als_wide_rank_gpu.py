"""ALS at factor ranks 129..256 (csrc/als_wide.hip): the packed-triangle
MFMA solver against float64, its placement invariance, and the trainer.

One CSR holds one row of every degree in DEGREES: both sides of the
16-wide Cholesky panel, of the 32-entry staging tile and of F itself, an
empty row and a long one. The CPU tests at the end need no GPU.
"""

import functools

import pytest
import torch

from _als_solve_oracle import (ALPHA, LAM, TOL, _csr, _factors, _ref64,
                               _rel_fro)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DEGREES = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191,
           192, 193, 255, 256, 257, 300, 700]


@functools.lru_cache(maxsize=None)
def wide_problem(f, implicit):
    g = torch.Generator().manual_seed(9200 + f)
    indptr, cols, vals = _csr(DEGREES, g)
    Y = _factors(f, g)
    return indptr, cols, vals, Y, _ref64(indptr, cols, vals, Y, LAM, implicit)


def _solve(indptr, cols, vals, Y, implicit, pieces=None):
    from predictionio_amd.ops import als as als_ops
    n_rows = indptr.shape[0] - 1
    out = torch.full((n_rows, Y.shape[1]), float("nan"), device="cuda")
    dev = (indptr.cuda(), cols.cuda(), vals.cuda(), Y.cuda())
    for lo, hi in (pieces or [(0, n_rows)]):
        als_ops.als_solve(*dev, lam=LAM, alpha=ALPHA, implicit=implicit,
                          row_range=(lo, hi), out=out[lo:hi])
    return out.cpu()


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("implicit", [False, True],
                         ids=["explicit", "implicit"])
@pytest.mark.parametrize("f", [129, 192, 193, 256])
def test_wide_solve_matches_float64(f, implicit):
    indptr, cols, vals, Y, X64 = wide_problem(f, implicit)
    X = _solve(indptr, cols, vals, Y, implicit)
    print(f"f={f} implicit={implicit}: rel fro {_rel_fro(X, X64):.3e}, "
          f"max abs {(X.double() - X64).abs().max().item():.3e}")
    assert torch.isfinite(X).all()
    assert torch.allclose(X.double(), X64, atol=TOL, rtol=TOL)


@pytest.mark.gpu
@requires_gpu
def test_wide_rows_do_not_depend_on_placement(monkeypatch):
    """Whole, in two row_range pieces into one buffer, and on a grid of 3
    workgroups: the same bits."""
    indptr, cols, vals, Y, _ = wide_problem(193, True)
    n_rows = indptr.shape[0] - 1
    whole = _solve(indptr, cols, vals, Y, True)
    pieces = _solve(indptr, cols, vals, Y, True,
                    [(0, 10), (10, n_rows)])
    monkeypatch.setenv("PIO_ALS_WIDE_GRID", "3")
    small = _solve(indptr, cols, vals, Y, True)
    assert torch.isfinite(whole).all()
    assert torch.equal(whole, pieces)
    assert torch.equal(whole, small)


@pytest.mark.gpu
@requires_gpu
def test_trainer_rank_200():
    from predictionio_amd.models.als import ALSParams, ALSTrainer
    from predictionio_amd.ops import als as als_ops
    n_users, n_items, nnz = 300, 200, 6000
    g = torch.Generator().manual_seed(77)
    key = torch.randperm(n_users * n_items, generator=g)[:nnz]
    users, items = key // n_items, key % n_items
    vals = torch.rand(nnz, generator=g) * 3 + 0.5

    def trainer(**kw):
        p = ALSParams(rank=200, iterations=1, lambda_=LAM, alpha=ALPHA,
                      implicit=True, seed=5, **kw)
        tr = ALSTrainer(p, n_users, n_items, torch.device("cuda", 0))
        tr.set_ratings(users, items, vals)
        tr.init_factors()
        return tr

    tr = trainer()
    Y0 = tr.Y.cpu().double()
    ip, ix, vv = (t.cpu() for t in tr.user_csr)
    tr.step()
    X64 = als_ops.als_solve_ref(ip, ix, vv.double(), Y0,
                                YtY=als_ops.gramian(Y0), lam=LAM,
                                alpha=ALPHA, implicit=True)
    X = tr.X.cpu()
    print(f"trainer rank 200: rel fro {_rel_fro(X, X64):.3e}")
    assert X.shape == (n_users, 200) and tr.Y.shape == (n_items, 200)
    assert torch.allclose(X.double(), X64, atol=TOL, rtol=TOL)
    assert torch.isfinite(tr.Y).all()

    with pytest.raises(ValueError):
        trainer(nonnegative=True).step()
    indptr, cols, vals_, _, _ = wide_problem(256, False)
    Y257 = torch.zeros((400, 257), device="cuda")
    with pytest.raises(ValueError, match="256"):
        als_ops.als_solve(indptr.cuda(), cols.cuda(), vals_.cuda(), Y257)


def test_als_rank_mapping():
    from predictionio_amd.ops.als import (SUPPORTED_RANKS, als_pad_rank,
                                          pad_rank)
    assert SUPPORTED_RANKS == (16, 32, 64, 128)
    with pytest.raises(ValueError):
        pad_rank(129)
    assert [als_pad_rank(f) for f in (10, 128, 129, 192, 193, 256)] == \
        [16, 128, 192, 192, 256, 256]
    with pytest.raises(ValueError, match="256"):
        als_pad_rank(257)
