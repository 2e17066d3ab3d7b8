"""Cross-occurrence and LLR on the CPU: the torch reference against a
brute force in plain Python (the GPU tests use it too), the cross plan."""

import math
from collections import defaultdict

import pytest
import torch

from _cooc_oracle import random_pairs, star
from predictionio_amd.ops import cooccurrence as co

# fp32 rounding is 2^-24 relative; the fp64 sum is off by at most about
# 16 * 2^-52 * U ln U < 1e-10 at these sizes: 1e-6 is tenfold the first
TOL = 1e-6


def xlx(x):
    return x * math.log(x) if x > 0 else 0.0


def brute(ua, ia, ub, ib, n_users, score, exclude_self):
    """row item -> {column item: score} over every candidate (k11 > 0)."""
    A, B = defaultdict(set), defaultdict(set)
    for u, i in zip(ua.tolist(), ia.tolist()):
        A[i].add(u)
    for u, j in zip(ub.tolist(), ib.tolist()):
        B[j].add(u)
    U, out = n_users, {}
    for i, us in A.items():
        for j, vs in B.items():
            k11, ai, bj = len(us & vs), len(us), len(vs)
            if k11 == 0 or (exclude_self and i == j):
                continue
            llr = max(0.0, 2 * (
                xlx(U) - xlx(ai) - xlx(U - ai) - xlx(bj) - xlx(U - bj)
                + xlx(k11) + xlx(ai - k11) + xlx(bj - k11)
                + xlx(U - ai - bj + k11)))
            out.setdefault(i, {})[j] = llr if score == "llr" else k11
    return out


def check_rows(got, ref, score):
    """(ids, val) against ref = brute(...): counts exactly; LLR within TOL,
    ordered by the returned values, nothing better left out; -1/0 padding."""
    ids, val = got
    n = ids.shape[1]
    assert ids.dtype == torch.int32
    assert val.dtype == (torch.float32 if score == "llr" else torch.int32)
    for i, (rid, rv) in enumerate(zip(ids.cpu().tolist(), val.cpu().tolist())):
        cand = ref.get(i, {})
        k = min(n, len(cand))
        assert rid[k:] == [-1] * (n - k) and rv[k:] == [0] * (n - k)
        row = list(zip(rid[:k], rv[:k]))
        if score == "count":
            assert row == sorted(cand.items(),
                                 key=lambda jc: (-jc[1], jc[0]))[:n]
            continue
        assert row == sorted(row, key=lambda js: (-js[1], js[0]))
        assert len(set(rid[:k])) == k and set(rid[:k]) <= set(cand)
        for j, s in row:
            assert abs(s - cand[j]) <= TOL * max(1.0, cand[j])
        for j, r in cand.items():
            assert j in rid[:k] or r <= rv[k - 1] + TOL * max(1.0, r)


def cross_case(na, nb):
    ua, ia = random_pairs(300, na, 600, seed=21)
    ub, ib = random_pairs(300, nb, 900, seed=22)
    return ua, ia, na, ub, ib, nb, 300


@pytest.mark.parametrize("score", ["count", "llr"])
@pytest.mark.parametrize("na,nb,exclude_self,n", [
    (40, 70, False, 10), (70, 40, False, 64), (60, 60, True, 10)])
def test_reference_against_brute_force(na, nb, exclude_self, n, score):
    ua, ia, na, ub, ib, nb, U = cross_case(na, nb)
    ref = brute(ua, ia, ub, ib, U, score, exclude_self)
    check_rows(co.cross_occurrence_topn(ua, ia, na, ub, ib, nb, U, n,
                                        score=score,
                                        exclude_self=exclude_self),
               ref, score)
    if exclude_self:   # the self entry is the same thing with A = B
        ref = brute(ua, ia, ua, ia, U, score, True)
        check_rows(co.cooccurrence_topn(ua, ia, U, na, n, score=score),
                   ref, score)


@pytest.mark.parametrize("exclude_self", [False, True])
def test_cross_plan_bound(exclude_self):
    ua, ia, na, ub, ib, nb, U = cross_case(60, 60)
    a, b = co.build_csrs(ua, ia, U, na), co.build_csrs(ub, ib, U, nb)
    distinct = {i: len(r) for i, r in
                brute(ua, ia, ub, ib, U, "count", exclude_self).items()}
    for c in sorted(set(distinct.values())):   # a row with ub <= c - 1
        t0 = co.cooccurrence_plan(b[0], a[2], a[3], nb, (c - 1, c - 1),
                                  exclude_self=exclude_self, cross=True)[0]
        assert all(distinct[i] < c for i in t0.tolist())   # ub >= distinct
    # tight on a star whose centre is not a column: ub = its neighbours
    u, i, U, N = star(5, 7, 3)
    a = co.build_csrs(u, i, U, N)
    b = co.build_csrs(u[i != 0], i[i != 0], U, N)
    for c, tier in ((38, 0), (37, 2)):
        tiers = co.cooccurrence_plan(b[0], a[2], a[3], N, (c, c),
                                     exclude_self=exclude_self, cross=True)
        assert 0 in tiers[tier].tolist()


def test_validation():
    ua, ia, na, ub, ib, nb, U = cross_case(40, 70)
    args, f = (ua, ia, na, ub, ib, nb, U), co.cross_occurrence_topn
    for call in (lambda: f(*args, 5, score="cosine"),
                 lambda: f(*args, 5, exclude_self=True),   # Na != Nb
                 lambda: f(*args, 0),
                 lambda: f(ua, ia, na, ub, ib + nb, nb, U, 5),
                 lambda: co.cooccurrence_topn(ua, ia, U, na, 5,
                                              score="jaccard")):
        with pytest.raises(ValueError):
            call()
