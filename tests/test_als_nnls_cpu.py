"""CPU tests of the nonnegative ALS half-step: the torch reference
(als_solve_nnls_ref, block principal pivoting) against scipy's Lawson-Hanson
NNLS in float64, and the trainer with ALSParams.nonnegative."""

import numpy as np
import pytest
import torch
from scipy.optimize import nnls

from _als_solve_oracle import ALPHA, LAM, _csr, _factors

DEGREES = [0, 1, 5, 20, 48, 49, 64, 65, 100, 300]


@pytest.mark.parametrize("abs_y", [False, True])
@pytest.mark.parametrize("f", [10, 64])
@pytest.mark.parametrize("implicit", [False, True])
def test_reference_against_scipy(implicit, f, abs_y):
    """min 1/2 x'Ax - b'x over x >= 0 is min |L'x - L^-1 b| with A = LL'.
    With Y as generated about half the coordinates end at 0; with |Y| few
    do in explicit mode and most in implicit mode."""
    from predictionio_amd.ops import als as als_ops
    g = torch.Generator().manual_seed(9000 + f)
    indptr, cols, vals = _csr(DEGREES, g)
    Y = _factors(f, g).double()
    Y = Y.abs() if abs_y else Y
    YtY = als_ops.gramian(Y)
    X = als_ops.als_solve(indptr, cols, vals.double(), Y, YtY, LAM, ALPHA,
                          implicit, nonnegative=True)
    assert X.dtype == torch.float64 and (X >= 0).all()
    zeros = []
    for r, n in enumerate(DEGREES):
        if n == 0 and not implicit:
            assert not X[r].any()
            continue
        A, b = als_ops.normal_equations(indptr, cols, vals, Y, YtY, LAM,
                                        ALPHA, implicit, not implicit, r)
        L = np.linalg.cholesky(A.numpy())
        x, _ = nnls(L.T, np.linalg.solve(L, b.numpy()), maxiter=10000)
        x = torch.from_numpy(x)
        diff = (X[r] - x).abs().max().item()
        assert diff <= 1e-10, f"row {r} (degree {n}): {diff}"
        assert torch.equal(X[r] == 0, x == 0), f"row {r}: zero pattern"
        if n:
            zeros.append(int((x == 0).sum()))
    print(f"implicit={implicit} f={f} abs_y={abs_y} zeros per row {zeros}")
    # explicit mode with |Y| binds few coordinates or none
    assert (abs_y and not implicit) or sum(zeros) > 0
    assert sum(zeros) < f * len(zeros)


@pytest.mark.parametrize("implicit", [False, True])
def test_trainer_nonnegative(implicit):
    """Every half-step minimises the objective exactly over a feasible set
    that holds the previous point: the loss never goes up."""
    from predictionio_amd.models.als import ALSParams, ALSTrainer
    g = torch.Generator().manual_seed(77)
    n_u, n_i, nnz = 60, 40, 600
    key = torch.randperm(n_u * n_i, generator=g)[:nnz]
    t = ALSTrainer(ALSParams(rank=8, iterations=6, lambda_=LAM, alpha=ALPHA,
                             implicit=implicit, seed=3, nonnegative=True,
                             loss_every=1), n_u, n_i, torch.device("cpu"))
    t.set_ratings(key // n_i, key % n_i,
                  torch.rand(nnz, generator=g) * 3 + 0.5)
    X, Y = t.fit()
    assert (X >= 0).all() and (Y >= 0).all() and X.any() and Y.any()
    losses = [h["loss"] for h in t.loss_history]
    print(f"implicit={implicit} losses {losses}")
    assert len(losses) == 6
    assert all(b <= a for a, b in zip(losses, losses[1:]))
