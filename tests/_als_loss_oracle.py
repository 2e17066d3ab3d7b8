"""Shared by the ALS-objective tests: the small training problem and the
objective evaluated from its definition over all user-item pairs in fp64.
"""

import torch

N_USERS, N_ITEMS, NNZ = 60, 40, 700
LAM, ALPHA = 0.05, 2.0


def problem():
    """(users, items, ratings): 700 distinct pairs of the 60 x 40 grid,
    r in {1..5}."""
    g = torch.Generator().manual_seed(20)
    cells = torch.randperm(N_USERS * N_ITEMS, generator=g)[:NNZ]
    users = (cells // N_ITEMS).to(torch.int32)
    items = (cells % N_ITEMS).to(torch.int32)
    ratings = torch.randint(1, 6, (NNZ,), generator=g).float()
    return users, items, ratings


def dense_objective(users, items, ratings, X, Y, lam, alpha, implicit):
    """(loss, sum_obs (r - s)^2) from the definition, all pairs, fp64."""
    X, Y = X.double().cpu(), Y.double().cpu()
    S = X @ Y.t()
    R = torch.zeros_like(S)
    M = torch.zeros_like(S)
    R[users.long(), items.long()] = ratings.double()
    M[users.long(), items.long()] = 1.0
    if implicit:
        # Hu-Koren: p = 1, c = 1 + alpha r on stored pairs; p = 0, c = 1
        # elsewhere
        C = 1.0 + alpha * R
        fit = (M * C * (1.0 - S) ** 2 + (1.0 - M) * S ** 2).sum()
        reg = lam * ((X ** 2).sum() + (Y ** 2).sum())
    else:
        fit = (M * (R - S) ** 2).sum()
        reg = lam * ((M.sum(1) * (X ** 2).sum(1)).sum()
                     + (M.sum(0) * (Y ** 2).sum(1)).sum())
    return float(fit + reg), float((M * (R - S) ** 2).sum())
