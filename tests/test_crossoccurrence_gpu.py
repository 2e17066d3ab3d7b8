"""The cross-occurrence / LLR variants of cooc_topn.hip, every tier forced
at tiny shapes, against the brute force of test_crossoccurrence_cpu.py."""

import functools

import pytest
import torch

from _cooc_oracle import rising
from predictionio_amd.ops import cooccurrence as co
from test_crossoccurrence_cpu import TOL, brute, check_rows, cross_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
TIERS = {
    "wave": {},
    "hash256": {"hash_caps": (0, co.HASH_CAPS[1])},
    "dense_lds": {"hash_caps": (0, 0), "dense_lds": True},
    # pool_slots=1: one counter row, reused by every row of the launch
    "dense_pool": {"hash_caps": (0, 0), "dense_lds": False, "pool_slots": 1},
}
tiers = pytest.mark.parametrize("tier", list(TIERS))


@functools.lru_cache(maxsize=None)
def case(na, nb, self_mode=False):
    ua, ia, na, ub, ib, nb, U = cross_case(na, nb)
    if self_mode:
        ub, ib = ua, ia
    csrs = (co.build_csrs(ua.to(DEV), ia.to(DEV), U, na),
            co.build_csrs(ub.to(DEV), ib.to(DEV), U, nb))
    ref = {s: brute(ua, ia, ub, ib, U, s, self_mode) for s in ("count", "llr")}
    return csrs, ref


@tiers
@pytest.mark.parametrize("score", ["count", "llr"])
@pytest.mark.parametrize("na,nb,self_mode,n", [
    (40, 70, False, 10), (70, 40, False, 64), (60, 60, True, 1),
    (60, 60, True, 10)])
def test_against_brute_force(tier, na, nb, self_mode, n, score):
    (a, b), ref = case(na, nb, self_mode)
    pool = (torch.zeros((3, nb), dtype=torch.int32, device=DEV)
            if tier == "dense_pool" else None)
    got = co.cross_occurrence_topn_csr(a, b, n, score=score, pool=pool,
                                       exclude_self=self_mode, **TIERS[tier])
    check_rows(got, ref[score], score)
    assert pool is None or not bool(pool.any())   # all zero again
    ids = got[0].cpu()
    if self_mode:   # the self entry runs the same kernel: bit for bit
        same = co.cooccurrence_topn_csr(*a, n, score=score, **TIERS[tier])
        assert torch.equal(same[0], got[0]) and torch.equal(same[1], got[1])
    elif nb > na:
        assert int(ids.max()) >= na             # column ids beyond the rows
        assert any(i in ids[i].tolist() for i in range(na))   # (i, i) kept
    else:
        assert bool((ids[nb:, 0] >= 0).any())   # row ids beyond the columns


@tiers
def test_ranking_is_by_llr(tier):
    """U = 100, the row item seen by users 0..9. Column 2 is seen by all
    users (k11 = 10, LLR 0), columns 5 and 7 by users 0..4 (k11 = 5)."""
    ua, ia = torch.arange(10), torch.full((10,), 3)
    ub = torch.cat([torch.arange(100), torch.arange(5), torch.arange(5)])
    ib = torch.cat([torch.full((100,), 2), torch.full((5,), 5),
                    torch.full((5,), 7)])
    a = co.build_csrs(ua.to(DEV), ia.to(DEV), 100, 4)
    b = co.build_csrs(ub.to(DEV), ib.to(DEV), 100, 9)
    run = functools.partial(co.cross_occurrence_topn_csr, a, b, **TIERS[tier])
    assert run(1)[0][3].item() == 5
    assert run(1, score="count")[0][3].item() == 2
    ids, val = run(3)   # the tie by id, the popular column last
    assert ids[3].tolist() == [5, 7, 2]
    assert val[3, 0].item() == val[3, 1].item() > 1.0   # a bitwise tie
    assert abs(val[3, 2].item()) <= TOL


@pytest.mark.parametrize("n", [1, 64])
@pytest.mark.parametrize("tier", ["hash256", "dense_lds", "dense_pool"])
def test_compaction_with_float_keys(tier, n):
    """Row 0 has 3 * SELECT_BUF + 17 columns; the winners come last."""
    u, i, n_users, n_items = rising(47, 81)
    U = n_users + 200                    # users who saw nothing: LLR > 0
    ua, ia = u[i == 0], i[i == 0]
    ub, ib = u[i != 0], i[i != 0]
    ref = brute(ua, ia, ub, ib, U, "llr", False)
    assert len(ref[0]) == 3 * co.SELECT_BUF + 17
    assert max(ref[0], key=ref[0].get) == n_items - 1
    got = co.cross_occurrence_topn_csr(
        co.build_csrs(ua.to(DEV), ia.to(DEV), U, n_items),
        co.build_csrs(ub.to(DEV), ib.to(DEV), U, n_items), n, **TIERS[tier])
    check_rows(got, ref, "llr")


def test_validation():
    ua, ia, na, ub, ib, nb, U = cross_case(40, 70)
    dev = [t.to(DEV) for t in (ua, ia, ub, ib)]
    (a, b), _ = case(40, 70)
    raw, csr = co.cross_occurrence_topn, co.cross_occurrence_topn_csr
    for call in (
            lambda: raw(dev[0], dev[1], na, dev[2], dev[3] + nb, nb, U, 10),
            lambda: raw(dev[0], dev[1] + na, na, dev[2], dev[3], nb, U, 10),
            lambda: raw(dev[0], dev[1], na, dev[2], dev[3], nb, U, 10,
                        exclude_self=True),
            lambda: csr(a, b, 10, score="cosine"),
            lambda: csr(a, b, 0), lambda: csr(a, b, 65),
            # the two user counts differ
            lambda: csr(a, co.build_csrs(dev[2], dev[3], U + 1, nb), 10)):
        with pytest.raises(ValueError):
            call()


def test_template_on_device():
    from predictionio_amd.controller import Params
    from predictionio_amd.data.bimap import BiMap
    from predictionio_amd.templates.similarproduct.engine import (
        CooccurrenceAlgorithm, Item, PreparedData, ViewEvent,
    )
    ev = [ViewEvent(f"u{u}", f"i{(u * u + 3 * j) % 25}", 0.0,
                    "buy" if j == 5 else "view")
          for u in range(40) for j in range(6)]
    items = {f"i{k}": Item(categories=["c"]) for k in range(27)}
    algo = CooccurrenceAlgorithm(Params({
        "n": 10, "scoring": "llr", "event": "view", "targetEvent": "buy"}))
    model = algo.train(PreparedData(users={}, items=items, view_events=ev))
    imap = BiMap.string_int([v.item for v in ev] + list(items))
    umap = BiMap.string_int(v.user for v in ev)
    side = {name: (torch.tensor([umap[v.user] for v in ev if v.name == name]),
                   torch.tensor([imap[v.item] for v in ev if v.name == name]))
            for name in ("view", "buy")}
    ref = brute(*side["view"], *side["buy"], len(umap), "llr", True)
    check_rows((torch.from_numpy(model.top_ids),
                torch.from_numpy(model.top_cnt)), ref, "llr")
    it = next(iter(model.top_n))
    assert algo.predict(model, {"items": [model.item_inv[it]],
                                "num": 3}).item_scores
