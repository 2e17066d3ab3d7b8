"""Held-out ranks on the CPU: heldout_ranks_ref and ranking_metrics against
a brute-force loop and hand-computed metrics; every validation error."""

import math

import pytest
import torch

from predictionio_amd.ops import ranking

I64, I32 = torch.int64, torch.int32


def csr(lists):
    ptr = [0]
    for lst in lists:
        ptr.append(ptr[-1] + len(lst))
    return (torch.tensor(ptr, dtype=I64),
            torch.tensor([j for lst in lists for j in lst], dtype=I32))


def brute(X, Y, tests, seens):
    gt, eq = [], []
    for b, targets in enumerate(tests):
        s = [sum(int(X[b, k]) * int(Y[j, k]) for k in range(X.shape[1]))
             for j in range(Y.shape[0])]
        cand = [j for j in range(Y.shape[0]) if j not in seens[b]]
        for t in targets:
            gt.append(sum(s[j] > s[t] for j in cand))
            eq.append(sum(s[j] == s[t] for j in cand if j != t))
    return gt, eq


def test_ref_matches_brute_force():
    g = torch.Generator().manual_seed(5)
    N, B, f = 40, 6, 16
    X = torch.randint(-2, 3, (B, f), generator=g).float()
    Y = torch.randint(-2, 3, (N, f), generator=g).float()
    tests = [[3], [], [0, 7, 39], [5, 6, 8, 9, 11, 30], [1, 2], [38]]
    seens = [[], [4, 5], [1], list(range(12, 30)),
             [j for j in range(N) if j not in (1, 2)], [0, 39]]
    tp, ti = csr(tests)
    sp, si = csr(seens)
    bgt, beq = brute(X, Y, tests, seens)
    for dtype in (torch.float32, torch.float64):
        gt, eq, nc = ranking.heldout_ranks_ref(X, Y, tp, ti, sp, si,
                                               dtype=dtype, block_elems=2 * N)
        assert gt.tolist() == bgt and eq.tolist() == beq
        assert nc.tolist() == [N - len(s) for s in seens]
    assert max(beq) > 0  # the data has ties
    gt, eq, nc = ranking.heldout_ranks(X, Y, tp, ti, sp, si)  # CPU route
    assert gt.tolist() == bgt and eq.tolist() == beq
    gt, eq, nc = ranking.heldout_ranks(X, Y, tp, ti, count_ties=False)
    assert gt.tolist() == brute(X, Y, tests, [[]] * B)[0]
    assert eq.tolist() == [0] * len(bgt) and nc.tolist() == [N] * B


def test_metrics_by_hand():
    # user 0: p = 0 and 2.5 (a tie) of 11 candidates; user 1: none;
    # user 2: p = 4 of 5 candidates
    tp = torch.tensor([0, 2, 2, 3], dtype=I64)
    gt = torch.tensor([0, 2, 4], dtype=I32)
    eq = torch.tensor([0, 1, 0], dtype=I32)
    nc = torch.tensor([11, 7, 5], dtype=I32)
    m = ranking.ranking_metrics(gt, eq, nc, tp, ks=(3, 1))
    assert (m["n_users"], m["n_pairs"]) == (2, 3)
    mpr = (0 / 10 + 2.5 / 10 + 4 / 4) / 3
    assert m["mpr"] == pytest.approx(mpr, abs=1e-15)
    assert m["auc"] == pytest.approx(1 - mpr, abs=1e-15)
    assert m["recall@3"] == pytest.approx((2 / 2 + 0) / 2, abs=1e-15)
    assert m["recall@1"] == pytest.approx((1 / 2 + 0) / 2, abs=1e-15)
    assert m["mrr"] == pytest.approx((1 / 1 + 1 / 5) / 2, abs=1e-15)
    dcg0 = 1 / math.log2(2) + 1 / math.log2(4.5)
    idcg0 = 1 / math.log2(2) + 1 / math.log2(3)
    assert m["ndcg@3"] == pytest.approx((dcg0 / idcg0 + 0) / 2, abs=1e-15)
    assert m["ndcg@1"] == pytest.approx((1 / 1 + 0) / 2, abs=1e-15)
    w = torch.tensor([1.0, 3.0, 4.0])
    mw = ranking.ranking_metrics(gt, eq, nc, tp, weights=w)
    assert mw["mpr"] == pytest.approx((3 * 0.25 + 4 * 1.0) / 8, abs=1e-15)


BAD = {
    "test ptr start": dict(tp=[1, 2, 3]),
    "test ptr end": dict(tp=[0, 1, 2]),
    "test ptr decreases": dict(tp=[0, 3, 2], ti=[1, 2, 3]),
    "test not ascending": dict(tp=[0, 3, 3], ti=[1, 3, 2]),
    "test repeated": dict(tp=[0, 3, 3], ti=[1, 1, 2]),
    "test id high": dict(ti=[1, 2, 9]),
    "test id negative": dict(ti=[-1, 2, 3]),
    "seen not ascending": dict(sp=[0, 2, 2], si=[5, 4]),
    "seen id high": dict(si=[4, 9]),
    "seen ptr end": dict(sp=[0, 1, 1]),
    "target seen": dict(si=[4, 2]),
    "X not finite": dict(x=float("inf")),
    "Y not finite": dict(y=float("nan")),
    "seen half given": dict(si=None),
    "ptr dtype": dict(tp_dtype=torch.int32),
    "rank mismatch": dict(fx=5),
}


def bad_inputs(case, device="cpu"):
    """A sound call (2 users, 9 items, f = 4) with one thing broken."""
    c = BAD[case]
    X = torch.ones(2, c.get("fx", 4))
    Y = torch.ones(9, 4)
    if "x" in c:
        X[1, 2] = c["x"]
    if "y" in c:
        Y[8, 0] = c["y"]
    tp = torch.tensor(c.get("tp", [0, 1, 3]), dtype=c.get("tp_dtype", I64))
    ti = torch.tensor(c.get("ti", [1, 2, 3]), dtype=I32)
    sp = torch.tensor(c.get("sp", [0, 1, 2]), dtype=I64)
    si = c.get("si", [4, 5])
    si = None if si is None else torch.tensor(si, dtype=I32).to(device)
    return (X.to(device), Y.to(device), tp.to(device), ti.to(device),
            sp.to(device), si)


@pytest.mark.parametrize("case", list(BAD))
def test_validation(case):
    with pytest.raises(ValueError):
        ranking.heldout_ranks(*bad_inputs(case))
    with pytest.raises(ValueError):
        ranking.heldout_ranks_ref(*bad_inputs(case))


def test_item_count_limit():
    Y = torch.ones(1, 4).expand(2 ** 31, 4)  # no storage behind it
    with pytest.raises(ValueError, match="2\\^31"):
        ranking.heldout_ranks(torch.ones(1, 4), Y,
                              torch.tensor([0, 0]), torch.zeros(0, dtype=I32))
