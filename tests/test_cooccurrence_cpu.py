"""Co-occurrence top-N without a GPU: the torch reference against a
brute-force pair counter, the tier routing at its caps, and the
similar-product template's train."""

import pytest
import torch

from _cooc_oracle import (
    SHAPES, arrays_to_dict, brute_force, random_pairs, star,
)
from predictionio_amd.ops import cooccurrence as co


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ref_equals_brute_force(shape):
    n_users, n_items, nnz, n = shape
    u, i = random_pairs(n_users, n_items, nnz, seed=n_items)
    # the data holds what the reference must cope with
    key = u * n_items + i
    assert key.unique().numel() < nnz                      # duplicate pairs
    assert n_items - 1 not in i.tolist()                   # unviewed item
    per_user = torch.bincount(key.unique() // n_items, minlength=n_users)
    assert bool((per_user == 1).any())                     # one-item user
    ids, cnt = co.cooccurrence_topn(u, i, n_users, n_items, n)
    assert ids.shape == (n_items, n) and cnt.shape == (n_items, n)
    want = brute_force(u, i, n)
    assert arrays_to_dict(ids, cnt) == want
    if n == 64:  # n above every row's neighbour count: padded rows
        assert max(len(v) for v in want.values()) < n
    # an item never lists itself
    own = torch.arange(n_items, dtype=torch.int32).unsqueeze(1)
    assert not bool((ids == own).any())


def test_ref_handles_empty_and_single():
    e = torch.zeros(0, dtype=torch.int64)
    ids, cnt = co.cooccurrence_topn_ref(e, e, 3, 4, 2)
    assert bool((ids == -1).all()) and bool((cnt == 0).all())
    # every user views one item: no pair at all
    u = torch.arange(5)
    ids, cnt = co.cooccurrence_topn_ref(u, u % 3, 5, 3, 2)
    assert bool((ids == -1).all()) and bool((cnt == 0).all())


def _plan(u, i, n_users, n_items, caps=co.HASH_CAPS):
    u_indptr, _, i_indptr, i_users = co.build_csrs(u, i, n_users, n_items)
    return co.cooccurrence_plan(u_indptr, i_indptr, i_users, n_items, caps)


@pytest.mark.parametrize("k", [0, 1])
def test_plan_routes_at_the_cap(k):
    cap = co.HASH_CAPS[k]
    assert cap % 64 == 0
    # ub(item 0) == cap: inside tier k
    tiers = _plan(*star(cap // 64, 64, 0))
    assert 0 in tiers[k].tolist()
    assert all(0 not in t.tolist() for j, t in enumerate(tiers) if j != k)
    # ub(item 0) == cap + 1: the next tier
    tiers = _plan(*star(cap // 64, 64, 1))
    assert 0 in tiers[k + 1].tolist()
    assert all(0 not in t.tolist() for j, t in enumerate(tiers) if j != k + 1)
    # every other item has one user with at most 65 items: the small tier
    assert sum(t.numel() for t in tiers[1:]) == 1


def test_plan_lists_live_rows_once_heaviest_first():
    n_users, n_items = 300, 200
    u, i = random_pairs(n_users, n_items, 2500, seed=3)
    u = torch.cat([u, torch.tensor([n_users])])      # a one-item user ...
    i = torch.cat([i, torch.tensor([n_items])])      # ... of its own item
    n_users, n_items = n_users + 1, n_items + 2      # and an unviewed item
    u_indptr, _, i_indptr, i_users = co.build_csrs(u, i, n_users, n_items)
    d = (u_indptr[1:] - u_indptr[:-1])
    deg = i_indptr[1:] - i_indptr[:-1]
    work = torch.tensor([int(d[i_users[s:e].long()].sum())
                         for s, e in zip(i_indptr[:-1], i_indptr[1:])])
    for caps in (co.HASH_CAPS, (0, 0), (0, co.HASH_CAPS[1]), (20, 60)):
        tiers = co.cooccurrence_plan(u_indptr, i_indptr, i_users, n_items,
                                     caps)
        listed = torch.cat(tiers).long()
        assert listed.unique().numel() == listed.numel()
        assert bool((deg[listed] > 0).all())
        live = (deg > 0) & (work - deg > 0)
        assert sorted(listed.tolist()) == live.nonzero().flatten().tolist()
        assert n_items - 1 not in listed.tolist()    # deg = 0
        assert n_items - 2 not in listed.tolist()    # ub = 0
        ub = torch.clamp(work - deg, max=n_items - 1)
        lo = (0, caps[0], max(caps))
        hi = (caps[0], caps[1], n_items)
        for t, rows in enumerate(tiers):
            rows = rows.long()
            assert rows.dtype == torch.int64 and tiers[t].dtype == torch.int32
            assert bool(((ub[rows] > lo[t]) & (ub[rows] <= hi[t])).all())
            assert bool((work[rows][1:] <= work[rows][:-1]).all())


def test_rejects_bad_arguments():
    u, i = random_pairs(10, 10, 30, seed=1)
    with pytest.raises(ValueError):
        co.cooccurrence_topn(u, i, 10, 10, 0)
    bad = i.clone()
    bad[3] = 10
    with pytest.raises(ValueError):
        co.cooccurrence_topn(u, bad, 10, 10, 5)
    with pytest.raises(ValueError):
        co.cooccurrence_topn(u, -bad, 10, 10, 5)


def test_template_train_equals_brute_force():
    from predictionio_amd.controller import Params
    from predictionio_amd.data.bimap import BiMap
    from predictionio_amd.templates.similarproduct.engine import (
        CooccurrenceAlgorithm, Item, PreparedData, Query, ViewEvent,
    )
    views = []
    for u in range(20):  # even users view even items, odd users odd ones
        for k in range(0, 8, 2):
            views.append(ViewEvent(f"u{u}", f"i{k + u % 2}", float(u)))
        views.append(ViewEvent(f"u{u}", f"i{u % 2}", 99.0))   # a repeat
        if u % 5 == 0:
            views.append(ViewEvent(f"u{u}", f"i{8 + u // 5}", 1.0))
    items = {f"i{k}": Item(categories=["c"]) for k in range(14)}
    pd_ = PreparedData(users={}, items=items, view_events=views)
    algo = CooccurrenceAlgorithm(Params({"n": 3}))
    model = algo.train(pd_)
    item_map = BiMap.string_int([v.item for v in views] + list(items))
    user_map = BiMap.string_int(v.user for v in views)
    want = brute_force(torch.tensor([user_map[v.user] for v in views]),
                       torch.tensor([item_map[v.item] for v in views]), 3)
    assert model.top_n == want
    assert all(type(j) is int and type(c) is int
               for row in model.top_n.values() for j, c in row)
    assert model.top_ids.shape == (len(item_map), 3)
    assert arrays_to_dict(torch.from_numpy(model.top_ids),
                          torch.from_numpy(model.top_cnt)) == want
    assert item_map["i13"] not in model.top_n     # never viewed
    r = algo.predict(model, Query(items=["i0"], num=3))
    assert {s.item for s in r.item_scores} <= {"i2", "i4", "i6"}
