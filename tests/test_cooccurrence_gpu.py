"""cooc_topn.hip on the GPU. Everything is integer, so every comparison
is exact equality of both result arrays with the torch reference (or,
where the reference would not fit, with dense per-row counts)."""

import functools

import pytest
import torch

from _cooc_oracle import (
    arrays_to_dict, brute_force, random_pairs, rising, star,
)
from predictionio_amd.ops import cooccurrence as co

pytestmark = pytest.mark.gpu

DEV = "cuda"
NS = (1, 10, 64)


def csrs(u, i, n_users, n_items):
    return co.build_csrs(u.to(DEV), i.to(DEV), n_users, n_items)


def assert_same(got, want):
    ids, cnt = got
    assert ids.dtype == torch.int32 and cnt.dtype == torch.int32
    assert ids.is_cuda and cnt.is_cuda
    assert torch.equal(ids.cpu(), want[0])
    assert torch.equal(cnt.cpu(), want[1])


@functools.lru_cache(maxsize=None)
def random_case():
    """U = 300, N = 200, 0-12 items per user: many count-1 ties, empty
    rows (the last item) and rows with fewer than 64 neighbours."""
    g = torch.Generator().manual_seed(11)
    n_users, n_items = 300, 200
    per = torch.randint(0, 13, (n_users,), generator=g)
    u = torch.repeat_interleave(torch.arange(n_users), per)
    i = torch.randint(0, n_items - 1, (u.numel(),), generator=g)
    ref = {n: co.cooccurrence_topn_ref(u, i, n_users, n_items, n)
           for n in NS}
    assert bool((ref[64][0][n_items - 1] == -1).all())        # an empty row
    assert bool((ref[64][0][:, -1] == -1).any())              # padded rows
    c10 = ref[10][1]
    assert bool(((c10[:, 1:] == c10[:, :-1]) & (c10[:, 1:] > 0)).any())
    return u, i, n_users, n_items, ref


@functools.lru_cache(maxsize=None)
def rising_case():
    """One item with 3 * SELECT_BUF + 17 distinct neighbours whose
    winners come last in its user list."""
    assert co.SELECT_BUF == 1024
    u, i, n_users, n_items = rising(47, 81)
    assert 47 * 64 + 81 == 3 * co.SELECT_BUF + 17
    ref = {n: co.cooccurrence_topn_ref(u, i, n_users, n_items, n)
           for n in (1, 64)}
    assert int((ref[64][0][0] >= 0).sum()) == 64
    assert ref[1][0][0, 0].item() == n_items - 1   # the last winner
    assert ref[1][1][0, 0].item() == 41
    assert ref[64][1][0, 1:3].tolist() == [40, 40]  # then ties, by id
    assert ref[64][0][0, 1:3].tolist() == [n_items - 3, n_items - 2]
    return u, i, n_users, n_items, ref


@pytest.mark.parametrize("n", NS)
def test_hash_tier_random(n):
    u, i, n_users, n_items, ref = random_case()
    got = co.cooccurrence_topn(u.to(DEV), i.to(DEV), n_users, n_items, n)
    assert_same(got, ref[n])
    if n == 10:
        assert arrays_to_dict(*got) == brute_force(u, i, n)


def test_ids_with_high_bits():
    g = torch.Generator().manual_seed(5)
    n_users, n_items = 200, 1 << 21
    pick = torch.randint(0, n_items, (300,), generator=g)
    pick[0], pick[1] = n_items - 1, 0
    u = torch.randint(0, n_users, (3000,), generator=g)
    i = pick[torch.randint(0, 300, (3000,), generator=g)]
    assert int(i.max()) == n_items - 1
    # the reference's sparse product is small: few hundred live items
    ref = co.cooccurrence_topn_ref(u, i, n_users, n_items, 10)
    c = csrs(u, i, n_users, n_items)
    assert_same(co.cooccurrence_topn_csr(*c, 10), ref)
    assert_same(co.cooccurrence_topn_csr(
        *c, 10, hash_caps=(0, co.HASH_CAPS[1])), ref)
    assert_same(co.cooccurrence_topn_csr(
        *c, 10, hash_caps=(0, 0), pool_slots=4, dense_lds=False), ref)


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("extra", [0, 1])
def test_table_at_capacity(k, extra):
    cap = co.HASH_CAPS[k]
    u, i, n_users, n_items = star(cap // 64, 64, extra)
    c = csrs(u, i, n_users, n_items)
    tiers = co.cooccurrence_plan(c[0], c[2], c[3], n_items, co.HASH_CAPS)
    assert 0 in tiers[k + extra].tolist()
    ref = co.cooccurrence_topn_ref(u, i, n_users, n_items, 10)
    assert ref[0][0].tolist() == list(range(1, 11))   # all count 1: by id
    # above the large cap the row is dense: once per counter home
    for dense_lds in ((False, True) if k + extra == 2 else (None,)):
        assert_same(co.cooccurrence_topn_csr(*c, 10, dense_lds=dense_lds),
                    ref)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dense_lds", [False, True])
def test_every_tier_gives_the_same_answer(n, dense_lds):
    u, i, n_users, n_items, ref = random_case()
    c = csrs(u, i, n_users, n_items)
    assert n_items <= co.DENSE_LDS_MAX
    assert_same(co.cooccurrence_topn_csr(*c, n), ref[n])
    assert_same(co.cooccurrence_topn_csr(
        *c, n, hash_caps=(0, co.HASH_CAPS[1])), ref[n])
    assert_same(co.cooccurrence_topn_csr(
        *c, n, hash_caps=(0, 0), dense_lds=dense_lds), ref[n])


def test_zero_invariant():
    u, i, n_users, n_items, ref = random_case()
    c = csrs(u, i, n_users, n_items)
    tiers = co.cooccurrence_plan(c[0], c[2], c[3], n_items, (0, 0))
    assert tiers[2].numel() >= 8       # all through the one counter row
    pool = torch.zeros((3, n_items), dtype=torch.int32, device=DEV)
    got = co.cooccurrence_topn_csr(*c, 10, hash_caps=(0, 0), pool=pool,
                                   pool_slots=1, dense_lds=False)
    assert_same(got, ref[10])
    assert not bool(pool.any())


@pytest.mark.parametrize("n", [1, 64])
@pytest.mark.parametrize("tier", ["hash", "dense", "dense_lds"])
def test_compaction(n, tier):
    u, i, n_users, n_items, ref = rising_case()
    c = csrs(u, i, n_users, n_items)
    if tier == "hash":
        tiers = co.cooccurrence_plan(c[0], c[2], c[3], n_items, co.HASH_CAPS)
        assert 0 in tiers[1].tolist()  # fits the large table
        got = co.cooccurrence_topn_csr(*c, n)
    else:
        got = co.cooccurrence_topn_csr(*c, n, hash_caps=(0, 0),
                                       dense_lds=tier == "dense_lds")
    assert_same(got, ref[n])


def test_memory_stays_bounded():
    """1000 users x 300 items of 40 000: the item x item product is
    >= 1.4 GB as COO; the op may use the pool plus O(nnz)."""
    g = torch.Generator().manual_seed(2)
    n_users, n_items, n = 1000, 40_000, 10
    pool_bytes = 64 << 20
    i = torch.randint(0, n_items, (n_users, 300), generator=g)
    u = torch.arange(n_users).unsqueeze(1).expand_as(i)
    u, i = u.reshape(-1).to(DEV), i.reshape(-1).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ids, cnt = co.cooccurrence_topn(u, i, n_users, n_items, n,
                                    pool_bytes=pool_bytes)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    print(f"peak above inputs: {used / 2 ** 20:.1f} MiB")
    assert used < pool_bytes + (32 << 20)
    assert ids.shape == (n_items, n) and cnt.shape == (n_items, n)
    # 50 sampled rows against dense counts of that row alone
    A = torch.zeros((n_users, n_items), dtype=torch.bool, device=DEV)
    A[u, i] = True
    col = torch.arange(n_items, device=DEV)
    for it in torch.randint(0, n_items, (50,), generator=g).tolist():
        c = A[A[:, it]].sum(0)
        c[it] = 0
        key = (c << 32) | (0xFFFFFFFF - col)
        top = torch.topk(key, n).values
        want_cnt = (top >> 32).to(torch.int32)
        want_ids = torch.where(want_cnt > 0,
                               (0xFFFFFFFF - (top & 0xFFFFFFFF)),
                               torch.full_like(top, -1)).to(torch.int32)
        assert torch.equal(ids[it], want_ids)
        assert torch.equal(cnt[it], want_cnt)


def test_validation_before_launch():
    u, i = random_pairs(20, 30, 100, seed=4)
    ud, idev = u.to(DEV), i.to(DEV)
    for n in (0, 65):
        with pytest.raises(ValueError):
            co.cooccurrence_topn(ud, idev, 20, 30, n)
    bad = idev.clone()
    bad[7] = 30
    with pytest.raises(ValueError):
        co.cooccurrence_topn(ud, bad, 20, 30, 10)
    c = list(csrs(u, i, 20, 30))
    for n in (0, 65):
        with pytest.raises(ValueError):
            co.cooccurrence_topn_csr(*c, n)
    items = c[1].clone()
    items[3] = 30
    with pytest.raises(ValueError):
        co.cooccurrence_topn_csr(c[0], items, c[2], c[3], 10)
    users = c[3].clone()
    users[3] = -1
    with pytest.raises(ValueError):
        co.cooccurrence_topn_csr(c[0], c[1], c[2], users, 10)
    indptr = c[0].clone()
    indptr[-1] += 1
    with pytest.raises(ValueError):
        co.cooccurrence_topn_csr(indptr, c[1], c[2], c[3], 10)
    with pytest.raises(ValueError):
        co.cooccurrence_topn_csr(*c, 10, hash_caps=(co.HASH_CAPS[0] + 1,
                                                    co.HASH_CAPS[1]))


def test_template_on_device():
    from predictionio_amd.controller import Params
    from predictionio_amd.data.bimap import BiMap
    from predictionio_amd.templates.similarproduct.engine import (
        CooccurrenceAlgorithm, Item, PreparedData, ViewEvent,
    )
    views = []
    for u in range(40):
        for j in range(6):
            views.append(ViewEvent(f"u{u}", f"i{(u * u + 3 * j) % 25}",
                                   float(u * 10 + j)))
    items = {f"i{k}": Item(categories=["c"]) for k in range(27)}
    pd_ = PreparedData(users={}, items=items, view_events=views)
    model = CooccurrenceAlgorithm(Params({"n": 10})).train(pd_)
    item_map = BiMap.string_int([v.item for v in views] + list(items))
    user_map = BiMap.string_int(v.user for v in views)
    want = brute_force(torch.tensor([user_map[v.user] for v in views]),
                       torch.tensor([item_map[v.item] for v in views]), 10)
    assert model.top_n == want
    assert arrays_to_dict(torch.from_numpy(model.top_ids),
                          torch.from_numpy(model.top_cnt)) == want
