"""Held-out rank kernels (rank_count.hip) against CPU brute force: exact on
integer data, bit identity of target and streamed scores, fp64 bounds."""

import functools

import pytest
import torch

from predictionio_amd.ops import ranking

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

I64, I32 = torch.int64, torch.int32
TMAX = 4  # targets per slot, RK_TMAX of rank_count.hip
T_LENS = [TMAX + 1, 0, 1, TMAX, 2 * TMAX + 3]


def csr(lists, device="cuda"):
    ptr = [0]
    for lst in lists:
        ptr.append(ptr[-1] + len(lst))
    return (torch.tensor(ptr, dtype=I64, device=device),
            torch.tensor([j for lst in lists for j in lst], dtype=I32,
                         device=device))


def brute(S, tests, seens):
    """gt, eq of every pair from a CPU score matrix S [B, N]."""
    gt, eq = [], []
    for b, targets in enumerate(tests):
        cand = torch.ones(S.shape[1], dtype=torch.bool)
        cand[seens[b]] = False
        for t in targets:
            gt.append(int((S[b][cand] > S[b, t]).sum()))
            eq.append(int((S[b][cand] == S[b, t]).sum()) - 1)
    return gt, eq


# (f, N, B, n_slices): both sides of the 32-row tile and of the 64-item
# chunk, a tail, slices that cut the data (and, N = 200 in 3, an empty
# one); 1 / 33 / 100 users make 2, 45 and 140 slots (one wave, two waves,
# two workgroups). Seen lengths run through 0, 1, 40 and all-but-targets.
INT_CASES = [(16, 1, 1, 1), (16, 31, 33, 3), (32, 32, 100, 1),
             (32, 33, 1, 3), (64, 64, 33, 1), (64, 65, 100, 3),
             (128, 65, 33, 3), (128, 200, 100, 3), (64, 200, 100, 1),
             (16, 200, 33, 3)]


@functools.lru_cache(maxsize=None)
def int_problem(f, N, B):
    g = torch.Generator().manual_seed(f * 1000 + N + B)
    X = torch.randint(-4, 5, (B, f), generator=g)
    Y = torch.randint(-4, 5, (N, f), generator=g)
    tests, seens = [], []
    for b in range(B):
        perm = torch.randperm(N, generator=g).tolist()
        nt = min(T_LENS[b % 5], N)
        ns = min([0, 1, 40, N][(b // 5 + b) % 4], N - nt)
        tests.append(sorted(perm[:nt]))
        seens.append(sorted(perm[nt:nt + ns]))
    return X, Y, tests, seens, brute(X @ Y.t(), tests, seens)


@requires_gpu
@pytest.mark.parametrize("f,N,B,n_slices", INT_CASES)
def test_exact_on_integers(f, N, B, n_slices):
    X, Y, tests, seens, (bgt, beq) = int_problem(f, N, B)
    args = (X.float().cuda(), Y.float().cuda(), *csr(tests), *csr(seens))
    gt, eq, nc = ranking.heldout_ranks(*args, n_slices=n_slices)
    assert gt.dtype == I32 and eq.dtype == I32 and nc.dtype == I32
    assert gt.tolist() == bgt
    assert eq.tolist() == beq
    assert nc.tolist() == [N - len(s) for s in seens]
    again = ranking.heldout_ranks(*args, n_slices=n_slices)
    assert all(torch.equal(a, b) for a, b in zip((gt, eq, nc), again))
    gt0, eq0, _ = ranking.heldout_ranks(*args, n_slices=n_slices,
                                        count_ties=False)
    assert gt0.tolist() == bgt and not eq0.any()


@requires_gpu
def test_unpadded_rank_and_no_seen_list():
    X, Y, tests, _, _ = int_problem(32, 33, 1)
    X, Y = X[:, :21], Y[:, :21]
    bgt, beq = brute(X @ Y.t(), tests, [[]])
    gt, eq, nc = ranking.heldout_ranks(X.float().cuda(), Y.float().cuda(),
                                       *csr(tests))
    assert (gt.tolist(), eq.tolist(), nc.tolist()) == (bgt, beq, [33])


@functools.lru_cache(maxsize=None)
def float_problem():
    """f = 64, N = 300 in three slices of two 64-item chunks. User b holds
    out 10 + b, whose row is copied to 100 + b (another chunk), 200 + b
    (another slice, and seen) and 280 + b (the last slice); 20 + b, no
    copies; and 50 + b, made the user's best item by construction."""
    g = torch.Generator().manual_seed(77)
    f, N, B = 64, 300, 8
    X = torch.randn(B, f, generator=g)
    Y = torch.randn(N, f, generator=g)
    top = Y.norm(dim=1).max()
    tests, seens = [], []
    for b in range(B):
        for c in (100, 200, 280):
            Y[c + b] = Y[10 + b]
        Y[50 + b] = X[b] * (2 * top / X[b].norm())
        tests.append([10 + b, 20 + b, 50 + b])
        seens.append([5, 150, 200 + b])
    gt, eq, _ = ranking.heldout_ranks(X.cuda(), Y.cuda(), *csr(tests),
                                      *csr(seens), n_slices=3)
    return X, Y, tests, seens, gt.view(B, 3).tolist(), eq.view(B, 3).tolist()


@requires_gpu
def test_bit_identity_of_target_and_streamed_scores():
    *_, gt, eq = float_problem()
    assert [e[0] for e in eq] == [2] * 8   # the two unseen copies
    assert [e[1] for e in eq] == [0] * 8
    assert [e[2] for e in eq] == [0] * 8
    assert [g[2] for g in gt] == [0] * 8   # the arg-max item


@requires_gpu
def test_within_fp64_bounds():
    """lo <= gt <= hi with e_j = f 2^-23 |x_b| . |y_j|, the bound of
    test_row_transform_random, on both scores of a compare."""
    X, Y, tests, seens, gt, _ = float_problem()
    S = X.double() @ Y.double().t()
    E = 64 * 2.0 ** -23 * (X.double().abs() @ Y.double().abs().t())
    for b, targets in enumerate(tests):
        cand = torch.ones(Y.shape[0], dtype=torch.bool)
        cand[seens[b]] = False
        for m, t in enumerate(targets):
            d, e = S[b] - S[b, t], E[b] + E[b, t]
            lo = int((cand & (d > e)).sum())
            cand_t = cand.clone()
            cand_t[t] = False
            hi = int((cand_t & (d >= -e)).sum())
            assert lo <= gt[b][m] <= hi, (b, t, lo, gt[b][m], hi)


@requires_gpu
@pytest.mark.parametrize("what", ["order", "test id", "seen id", "ptr",
                                  "overlap", "finite", "none"])
def test_validation_on_device(what):
    X, Y = torch.ones(2, 4).cuda(), torch.ones(9, 4).cuda()
    tests, seens = [[1], [2, 3]], [[4], [5]]
    if what == "order":
        tests[1] = [3, 2]
    elif what == "test id":
        tests[1] = [2, 9]
    elif what == "seen id":
        seens[0] = [-1]
    elif what == "overlap":
        seens[1] = [2]
    elif what == "finite":
        Y[8, 3] = float("nan")
    (tp, ti), (sp, si) = csr(tests), csr(seens)
    if what == "ptr":
        sp[2] = 1
    if what == "none":
        assert ranking.heldout_ranks(X, Y, tp, ti, sp, si)[2].tolist() == [8, 8]
        return
    with pytest.raises(ValueError):
        ranking.heldout_ranks(X, Y, tp, ti, sp, si)


@requires_gpu
def test_trainer_heldout():
    from predictionio_amd.models.als import ALSParams, ALSTrainer
    g = torch.Generator().manual_seed(3)
    U, N = 40, 90
    u = torch.randint(0, U, (600,), generator=g)
    i = torch.randint(0, N, (600,), generator=g)
    tr = ALSTrainer(ALSParams(rank=16, iterations=2, implicit=True, seed=1),
                    U, N)
    tr.set_ratings(u, i, torch.ones(600))
    tr.fit()
    tr.X = (tr.X * 8).round()  # exact scores, plenty of ties
    tr.Y = (tr.Y * 8).round()
    seen = torch.zeros(U, N, dtype=torch.bool)
    seen[u, i] = True
    tu, ti = torch.nonzero(~seen)[::37].t()  # unseen pairs, user-sorted
    w = torch.rand(tu.numel(), generator=g)
    got = tr.heldout(tu, ti, test_values=w, ks=(5, 20))
    users = torch.unique(tu)
    t_ptr = torch.zeros(users.numel() + 1, dtype=I64)
    t_ptr[1:] = torch.cumsum(torch.bincount(tu)[users], 0)
    s_ptr, s_idx = csr([torch.nonzero(seen[b])[:, 0].tolist()
                        for b in users.tolist()], "cpu")
    ref = ranking.heldout_ranks_ref(tr.X[users].cpu(), tr.Y.cpu(), t_ptr,
                                    ti.to(I32), s_ptr, s_idx,
                                    dtype=torch.float64)
    want = ranking.ranking_metrics(*ref, t_ptr, ks=(5, 20), weights=w)
    assert got["n_pairs"] == tu.numel() and got.keys() == want.keys()
    for k in want:
        assert got[k] == pytest.approx(want[k], abs=1e-12), k
