"""als_loss.hip on the GPU: exact lane layout on integer data, several
grid-stride passes, random data against fp64 within a computed bound,
determinism, validation, and the trainer's loss() end to end.
"""

import functools

import pytest
import torch

from _als_loss_oracle import (
    ALPHA, LAM, N_ITEMS, N_USERS, dense_objective, problem,
)
from predictionio_amd.models.als import ALSParams, ALSTrainer
from predictionio_amd.ops import als as als_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -23


def csr_of(degrees, n_cols, seed):
    """A CSR with the given row degrees, random column ids, r in 1..5."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.as_tensor(degrees, dtype=torch.int64)
    indptr = torch.zeros(deg.numel() + 1, dtype=torch.int64)
    indptr[1:] = deg.cumsum(0)
    nnz = int(indptr[-1])
    indices = torch.randint(0, n_cols, (nnz,), generator=g, dtype=torch.int32)
    values = torch.randint(1, 6, (nnz,), generator=g).float()
    return indptr.to(DEV), indices.to(DEV), values.to(DEV)


def int_factors(n, f, seed, misalign=False):
    g = torch.Generator().manual_seed(seed)
    F = torch.randint(-4, 5, (n, f), generator=g).float().to(DEV)
    if misalign:
        # the same values, starting one float into a fresh buffer
        buf = torch.empty(n * f + 1, device=DEV)
        view = buf[1:].view(n, f)
        view.copy_(F)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    return F


def row_ids(indptr):
    n = indptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=indptr.device),
                                   indptr[1:] - indptr[:-1])


def check_exact(indptr, indices, values, X, Y):
    """A, B and pred against int64 arithmetic, both modes."""
    rows = row_ids(indptr)
    s = (X[rows].long() * Y[indices.long()].long()).sum(1)
    r = values.long()
    want = {False: ((r - s) ** 2).sum(),
            True: ((1 + int(ALPHA) * r) * (1 - s) ** 2).sum()}
    for implicit in (False, True):
        pred = torch.full((indices.numel(),), float("nan"), device=DEV)
        got = als_ops.als_residual_sums(indptr, indices, values, X, Y,
                                        alpha=ALPHA, implicit=implicit,
                                        pred=pred)
        assert got.dtype == torch.float64 and got.shape == (2,)
        assert got[0].item() == float(want[implicit].item())
        assert got[1].item() == float((s * s).sum().item())
        assert torch.equal(pred, s.float())


MIXED = [0, 1, 3, 4, 5, 8, 9, 64, 5000]


@pytest.mark.parametrize("f", [1, 10, 12, 16, 64, 128])
def test_exact_layout_mixed_degrees(f):
    n_cols = 301
    csr = csr_of(MIXED, n_cols, seed=f)
    check_exact(*csr, int_factors(len(MIXED), f, 1), int_factors(n_cols, f, 2))


def test_exact_layout_misaligned_y_takes_scalar_path():
    n_cols = 301
    csr = csr_of(MIXED, n_cols, seed=7)
    check_exact(*csr, int_factors(len(MIXED), 64, 1),
                int_factors(n_cols, 64, 2, misalign=True))


@pytest.mark.parametrize("n_rows", [1, 4, 5])
@pytest.mark.parametrize("f", [10, 64])
def test_exact_layout_few_rows(n_rows, f):
    csr = csr_of([5, 0, 9, 3, 12][:n_rows], 50, seed=n_rows)
    check_exact(*csr, int_factors(n_rows, f, 3), int_factors(50, f, 4))


@pytest.mark.parametrize("f", [10, 16])
def test_exact_many_passes_with_empty_tail(f):
    """70 000 rows of degree 0..7: several passes of the persistent grid,
    the last block's rows all empty."""
    deg = torch.arange(70_000) % 8
    deg[-8:] = 0
    n_cols = 1000
    csr = csr_of(deg, n_cols, seed=11)
    check_exact(*csr, int_factors(70_000, f, 5), int_factors(n_cols, f, 6))


@pytest.mark.parametrize("f", [10, 64, 128])
def test_random_within_fma_chain_bound(f):
    """Against fp64. Per rating delta = f 2^-23 sum_k |x_k||y_k| bounds the
    fp32 fma-chain dot (as in test_als_mfma_gpu.py), so
    |A - A_ref| <= sum w (2 |t - s| delta + delta^2) and
    |B - B_ref| <= sum (2 |s| delta + delta^2)."""
    g = torch.Generator().manual_seed(100 + f)
    n_rows, n_cols = 2000, 3000
    deg = torch.randint(0, 41, (n_rows,), generator=g)
    indptr, indices, values = csr_of(deg, n_cols, seed=f)
    X = (torch.randn((n_rows, f), generator=g) / f ** 0.5).to(DEV)
    Y = (torch.randn((n_cols, f), generator=g) / f ** 0.5).to(DEV)
    rows, cols = row_ids(indptr), indices.long()
    Xd, Yd = X.double(), Y.double()
    s = (Xd[rows] * Yd[cols]).sum(1)
    delta = f * U * (Xd[rows].abs() * Yd[cols].abs()).sum(1)
    r = values.double()
    for implicit in (False, True):
        t = torch.ones_like(r) if implicit else r
        w = 1.0 + ALPHA * r if implicit else torch.ones_like(r)
        ref = als_ops.als_residual_sums_ref(indptr, indices, values, Xd, Yd,
                                            ALPHA, implicit)
        bound_a = (w * (2 * (t - s).abs() * delta + delta ** 2)).sum().item()
        bound_b = (2 * s.abs() * delta + delta ** 2).sum().item()
        pred = torch.empty(indices.numel(), device=DEV)
        got = als_ops.als_residual_sums(indptr, indices, values, X, Y,
                                        alpha=ALPHA, implicit=implicit,
                                        pred=pred)
        err_a = abs(got[0].item() - ref[0].item())
        err_b = abs(got[1].item() - ref[1].item())
        print(f"f={f} implicit={implicit}: |dA| / bound = "
              f"{err_a / bound_a:.4f}, |dB| / bound = {err_b / bound_b:.4f}")
        assert err_a <= bound_a and err_b <= bound_b
        assert ((pred.double() - s).abs() <= delta).all()


def test_two_calls_bit_identical():
    g = torch.Generator().manual_seed(9)
    deg = torch.randint(0, 30, (5000,), generator=g)
    csr = csr_of(deg, 800, seed=9)
    X = torch.randn((5000, 64), generator=g).to(DEV)
    Y = torch.randn((800, 64), generator=g).to(DEV)
    a = als_ops.als_residual_sums(*csr, X, Y, alpha=ALPHA, implicit=True)
    b = als_ops.als_residual_sums(*csr, X, Y, alpha=ALPHA, implicit=True)
    assert torch.equal(a, b)


def test_empty_inputs_return_zeros():
    Y = int_factors(7, 10, 1)
    zeros = torch.zeros(2, dtype=torch.float64, device=DEV)
    got = als_ops.als_residual_sums(*csr_of([0, 0, 0], 7, 1),
                                    int_factors(3, 10, 2), Y)
    assert got.dtype == torch.float64 and torch.equal(got, zeros)
    got = als_ops.als_residual_sums(*csr_of([], 7, 1),
                                    torch.empty((0, 10), device=DEV), Y)
    assert got.dtype == torch.float64 and torch.equal(got, zeros)


def test_rejects_bad_arguments():
    indptr, indices, values = csr_of([2, 3], 7, 1)
    X, Y = int_factors(2, 10, 2), int_factors(7, 10, 3)
    call = als_ops.als_residual_sums
    with pytest.raises(RuntimeError):   # dtype
        call(indptr, indices, values, X.half(), Y)
    with pytest.raises(RuntimeError):
        call(indptr, indices.long(), values, X, Y)
    with pytest.raises(RuntimeError):   # rank mismatch
        call(indptr, indices, values, X, int_factors(7, 12, 3))
    with pytest.raises(RuntimeError):   # X rows vs CSR rows
        call(indptr, indices, values, int_factors(3, 10, 2), Y)
    with pytest.raises(RuntimeError):   # f = 129
        call(indptr, indices, values, int_factors(2, 129, 2),
             int_factors(7, 129, 3))
    with pytest.raises(RuntimeError):   # pred length
        call(indptr, indices, values, X, Y,
             pred=torch.empty(4, device=DEV))
    with pytest.raises(RuntimeError):   # non-contiguous factors
        call(indptr, indices, values, int_factors(2, 20, 2)[:, :10], Y)
    bad = indices.clone()
    bad[3] = 7
    with pytest.raises(ValueError):     # out-of-range id: before any launch
        call(indptr, bad, values, X, Y)
    bad[3] = -1
    with pytest.raises(ValueError):
        call(indptr, bad, values, X, Y)


# ---------------------------------------------------------------- trainer

@functools.lru_cache(maxsize=None)
def fit_gpu(f, implicit):
    """12 iterations on the GPU with the history on; shared by the tests
    below and left unchanged by them."""
    users, items, ratings = problem()
    p = ALSParams(rank=f, iterations=12, lambda_=LAM, alpha=ALPHA,
                  implicit=implicit, seed=3, loss_every=1)
    t = ALSTrainer(p, N_USERS, N_ITEMS, torch.device(DEV))
    t.set_ratings(users, items, ratings)
    t.fit()
    return t


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("f", [10, 64])
def test_trainer_history_strictly_decreasing(f, implicit):
    t = fit_gpu(f, implicit)
    losses = [h["loss"] for h in t.loss_history]
    print(f"f={f} implicit={implicit}:", " ".join(f"{v:.9g}" for v in losses))
    assert len(losses) == 12
    assert all(b < a for a, b in zip(losses, losses[1:]))


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("f", [10, 64])
def test_trainer_loss_matches_dense_fp64(f, implicit):
    """loss() against the all-pairs fp64 objective of the same factors.
    Bound: the residual bound of test_random_within_fma_chain_bound, plus,
    in implicit mode, gamma_n = n 2^-23 (n = factor rows) on each of the
    two fp32 Gramians in <XtX, YtY>_F:
      |dG| <= gamma_n |F|^T |F|,
      |d<Gx, Gy>| <= sum (|dGx| |Gy| + |Gx| |dGy| + |dGx| |dGy|)."""
    t = fit_gpu(f, implicit)
    users, items, ratings = problem()
    got = t.loss()
    assert got == {k: v for k, v in t.loss_history[-1].items()
                   if k != "iteration"}
    X, Y = t.X.double().cpu(), t.Y.double().cpu()
    want, want_sq = dense_objective(users, items, ratings, X, Y, LAM, ALPHA,
                                    implicit)
    u, i, r = users.long(), items.long(), ratings.double()
    s = (X[u] * Y[i]).sum(1)
    delta = f * U * (X[u].abs() * Y[i].abs()).sum(1)
    if implicit:
        w, d = 1.0 + ALPHA * r, (1.0 - s).abs()
    else:
        w, d = torch.ones_like(r), (r - s).abs()
    bound = (w * (2 * d * delta + delta ** 2)).sum().item()
    if implicit:
        bound += (2 * s.abs() * delta + delta ** 2).sum().item()
        gx, gy = X.t() @ X, Y.t() @ Y
        dgx = N_USERS * U * (X.abs().t() @ X.abs())
        dgy = N_ITEMS * U * (Y.abs().t() @ Y.abs())
        bound += (dgx * gy.abs() + gx.abs() * dgy + dgx * dgy).sum().item()
    err = abs(got["loss"] - want)
    print(f"f={f} implicit={implicit}: loss {got['loss']:.12g} dense "
          f"{want:.12g} |err| / bound = {err / bound:.4f}")
    assert err <= bound
    if not implicit:
        assert abs(got["sq_err"] - want_sq) <= bound
        assert got["rmse"] == (got["sq_err"] / got["nnz"]) ** 0.5
