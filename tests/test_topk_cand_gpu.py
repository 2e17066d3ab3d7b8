"""Candidate-list top-K (csrc/topk_cand.hip) against a float64 reference
on inputs whose scores are exact in fp32: equality is bit for bit."""

import pytest
import torch

from _topk_oracle import int_problem, reference_topk, valid_items
from predictionio_amd.ops import topk as topk_ops

pytestmark = pytest.mark.gpu

N = 256


def _csr(lists):
    ip = torch.tensor([0] + [len(c) for c in lists]).cumsum(0)
    ci = torch.tensor([j for c in lists for j in c], dtype=torch.int32)
    return ip, ci


def _lists(lens, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [sorted(torch.randperm(n, generator=g)[:c].tolist()) for c in lens]


def _member(lists, n):
    m = torch.zeros((len(lists), n), dtype=torch.bool)
    for b, c in enumerate(lists):
        m[b, c] = True
    return m


def _run(Xq, Y, K, lists, filters=None, **kw):
    filters = filters or {}  # -> (GPU result, float64 reference)
    ip, ci = _csr(lists)
    dev = {k: v.cuda() for k, v in filters.items()}
    got = topk_ops._topk_score_cands(Xq.cuda(), Y.cuda(), K, ip.cuda(),
                                     ci.cuda(), **dev, **kw)
    valid = valid_items(Xq.shape[0], Y.shape[0], **filters) \
        & _member(lists, Y.shape[0])
    return got, reference_topk(Xq, Y, K, valid)


def _same(got, want):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
    assert torch.equal(got[1].cpu(), want[1]), (got[1], want[1])
    assert torch.equal(got[0].cpu(), want[0])


def _filters(which, B, lists, want_top, W):
    """Each named filter removes want_top[b][0], query b's unfiltered
    best (cats: of the even b), and every candidate of the last query."""
    f = {}
    tops = [(b, int(t[0])) for b, t in enumerate(want_top) if t[0] >= 0]
    if "mask" in which:
        f["item_mask"] = torch.zeros(N, dtype=torch.uint8)
        f["item_mask"][[j for b, j in tops if b % 3 == 0]] = 1
        f["item_mask"][lists[-1]] = 1
    if "bans" in which:
        bans = [sorted({j for q, j in tops if q == b} | {b, N - 1 - b})
                for b in range(B - 1)] + [lists[-1]]
        f["ban_indptr"], f["ban_indices"] = _csr(bans)
    if "cats" in which:
        # item j: bit j % 5 of word j % W; even b drops its best's bit
        ic = torch.zeros((N, W), dtype=torch.int32)
        j = torch.arange(N)
        ic[j, j % W] = (1 << (j % 5)).int()
        qc = torch.full((B, W), 31, dtype=torch.int32)
        for b, t in tops:
            if b % 2 == 0:
                qc[b] = 31 & ~(1 << (t % 5))
        qc[B - 1] = 0
        f["item_cats"], f["query_cats"] = ic, qc
    return f


@pytest.mark.parametrize("f", [10, 64, 128])
@pytest.mark.parametrize("K", [1, 20, 64])
@pytest.mark.parametrize("which,W", [("", 1), ("mask", 1), ("bans", 1),
                                     ("cats", 1), ("cats", 4),
                                     ("mask bans cats", 4)])
def test_lengths_filters_tiers(f, K, which, W):
    """Mixed lengths; both instantiations and a 7-segment cut agree."""
    lens = [0, 1, K - 1, K, 15, 16, 17, 65, 200]
    B = len(lens) + 1
    Xq, Y = int_problem(B, N, f, seed=K)
    lists = _lists(lens + [40], N, seed=f + K)
    top = reference_topk(Xq, Y, 1, _member(lists, N))[1]
    flt = _filters(which, B, lists, top, W)
    got, want = _run(Xq, Y, K, lists, flt)
    _same(got, want)
    assert not which or (got[1][-1] == -1).all()
    for kw in (dict(wave_max=0), dict(seg_len=32), dict(seg_len=32,
                                                        wave_max=16)):
        _same(_run(Xq, Y, K, lists, flt, **kw)[0], want)


def test_segment_count_and_stats():
    Xq, Y = int_problem(1, N, 64)
    lists = _lists([200], N, 3)
    before = topk_ops.cand_stats()["segments"]
    _same(*_run(Xq, Y, 20, lists, seg_len=32))
    assert topk_ops.cand_stats()["segments"] - before == 7


@pytest.mark.parametrize("wave_max", [0, 1 << 20])
def test_mid_list_compaction(wave_max):
    """Scores ascend along the list, so every candidate beats the
    threshold and is appended. The selection buffer holds TC_BUF = 512
    keys and a step appends S = 8 trips * THREADS / 16 keys: 128 with 256
    threads, 32 with one wave. A compaction runs once more than 512 - S
    keys are held, i.e. after 512 candidates in both (4 steps of 128, 16
    of 32); 1100 candidates compact twice mid-list."""
    n, f, K = 1100, 10, 20
    Y = torch.zeros((n, f))
    Y[:, 0] = torch.arange(n).float()
    Y[:, 3] = 1.0
    Xq = torch.zeros((1, f))
    Xq[0, 0] = 2.0
    Xq[0, 3] = -5.0
    got, want = _run(Xq, Y, K, [list(range(n))], seg_len=1 << 20,
                     wave_max=wave_max)
    _same(got, want)
    assert got[1][0].tolist() == list(range(n - 1, n - 1 - K, -1))


@pytest.mark.parametrize("kw", [dict(), dict(seg_len=4), dict(wave_max=0)])
def test_ties_by_hand(kw):
    """Duplicate rows at different ids: equal scores go id ascending,
    inside a segment and across one (seg_len = 4 splits 3 | 5, 9 | 11)."""
    Y = torch.zeros((16, 12))
    Y[:, 0] = torch.tensor([1, 7, 7, 5, 0, 5, 5, 2, 9, 3, 0, 3, 0, 0, 7, 9.])
    Xq = torch.zeros((1, 12))
    Xq[0, 0] = 1.0
    cands = [1, 2, 3, 5, 6, 7, 8, 9, 11, 14, 15]
    ip, ci = _csr([cands])
    v, i = topk_ops._topk_score_cands(Xq.cuda(), Y.cuda(), 10, ip.cuda(),
                                      ci.cuda(), **kw)
    assert i[0].tolist() == [8, 15, 1, 2, 14, 3, 5, 6, 9, 11]
    assert v[0].tolist() == [9, 9, 7, 7, 7, 5, 5, 5, 3, 3]


@pytest.mark.parametrize("K", [65, 300])
def test_scores_mode_large_k(K):
    lens = [0, 1, 64, 65, 200, 256]   # scores mode; K above some lists
    Xq, Y = int_problem(len(lens), N, 64, seed=2)
    lists = _lists(lens, N, 11)
    top = reference_topk(Xq, Y, 1, _member(lists, N))[1]
    flt = _filters("mask bans cats", len(lens), lists, top, 2)
    for kw in (dict(), dict(seg_len=48)):
        _same(*_run(Xq, Y, K, lists, flt, **kw))


def test_views_and_alignment():
    """A contiguous view whose base is 4 bytes off a 16-byte boundary
    takes the one-float-per-lane loads; a strided view is refused."""
    Xq, Y = int_problem(3, N, 64, seed=4)
    lists = _lists([17, 65, 200], N, 5)
    ip, ci = _csr(lists)
    buf = torch.zeros(N * 64 + 1, device="cuda")
    Yv = buf[1:].view(N, 64)
    Yv.copy_(Y)
    assert Yv.data_ptr() % 16 == 4
    got = topk_ops._topk_score_cands(Xq.cuda(), Yv, 20, ip.cuda(), ci.cuda())
    _same(got, reference_topk(Xq, Y, 20, _member(lists, N)))
    Yw = torch.zeros((N, 65), device="cuda")
    with pytest.raises(ValueError):
        topk_ops.topk_score(Xq.cuda(), Yw[:, 1:], 20, cand_indptr=ip.cuda(),
                            cand_indices=ci.cuda())


def test_row_offsets_past_4gib():
    """Rows beyond the 2^31 and 2^32 byte offsets of Y, with the rows 2
    and 4 GiB above row 5 planted too: 64-bit row addressing. (Both
    tiers and scores mode: test_large_offsets_gpu.py.)"""
    n, f = 2 ** 24 + 64, 64
    Y = torch.zeros((n, f), device="cuda")
    rows = [5, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 5, 2 ** 24 - 1, 2 ** 24,
            2 ** 24 + 5, 2 ** 24 + 7, n - 1]
    for r, j in enumerate(rows):
        Y[j, r] = float(r + 1)
        Y[j, 63] = 1.0
    Xq = torch.ones((1, f), device="cuda")
    ip, ci = _csr([rows])
    v, i = topk_ops.topk_score(Xq, Y, 9, cand_indptr=ip.cuda(),
                               cand_indices=ci.cuda())
    assert i[0].tolist() == rows[::-1]
    assert v[0].tolist() == [float(r + 2) for r in range(8, -1, -1)]


@pytest.mark.parametrize("ip,ci", [
    ([0, 3], [1, 2, N]),          # out of range
    ([0, 3], [-1, 2, 3]),         # negative
    ([0, 3], [1, 3, 2]),          # unsorted
    ([0, 3], [1, 2, 2]),          # duplicated
    ([0, 2], [1, 2, 3]),          # indptr does not end at nnz
    ([0, 3], None),               # one of the two
])
def test_validation(ip, ci):
    Xq, Y = int_problem(1, N, 10)
    kw = dict(cand_indptr=torch.tensor(ip).cuda())
    if ci is not None:
        kw["cand_indices"] = torch.tensor(ci, dtype=torch.int32).cuda()
    before = topk_ops.cand_stats()
    with pytest.raises(ValueError):
        topk_ops.topk_score(Xq.cuda(), Y.cuda(), 5, **kw)
    assert topk_ops.cand_stats() == before      # nothing was launched


# ------------------------------------------------------------ templates

def _seed_items(mem_storage, name, event, n_items, target_type):
    import random
    from predictionio_amd.data.events import DataMap, Event, utcnow
    from predictionio_amd.data.storage.base import App
    app_id = mem_storage.get_meta_data_apps().insert(App(id=0, name=name))
    lev = mem_storage.get_l_events()
    lev.init(app_id)

    def insert(ev, uid, iid=None, props=None, entity_type="user"):
        lev.insert(Event(
            event=ev, entity_type=entity_type, entity_id=uid,
            target_entity_type=target_type if iid else None,
            target_entity_id=iid, properties=DataMap(props or {}),
            event_time=utcnow()), app_id)

    rng = random.Random(2)
    for i in range(n_items):
        insert("$set", f"i{i}", None, {"categories": [f"c{i % 4}"]},
               entity_type="item")
    for u in range(50):
        liked = [i for i in range(n_items) if i % 3 == u % 3]
        for i in rng.sample(liked, 5) + rng.sample(range(n_items), 2):
            insert(event, f"u{u}", f"i{i}")
    return insert


def _same_results(batched, single):
    for (i, rb), (j, rs) in zip(batched, single):
        assert i == j and [s.item for s in rb.item_scores] == \
            [s.item for s in rs.item_scores], f"query {i}"
        assert all(abs(a.score - b.score) <= 1e-4 for a, b in
                   zip(rb.item_scores, rs.item_scores)), f"query {i}"


def test_ecomm_batch_keeps_white_lists(mem_storage):
    from predictionio_amd.controller import EngineParams, Params
    from predictionio_amd.templates.ecommercerecommendation import (
        ECommAlgorithm, ECommerceRecommendationEngine, Query,
    )
    insert = _seed_items(mem_storage, "MyTestApp", "view", 60, "item")
    for u in range(0, 50, 3):
        insert("buy", f"u{u}", f"i{u % 8}")
    ep = EngineParams(
        data_source_params=Params({"appName": "MyTestApp"}),
        algorithms_params=[("ecomm", Params(
            {"appName": "MyTestApp", "unseenOnly": False,
             "similarEvents": ["view"], "rank": 8, "numIterations": 4,
             "seed": 3}))])
    model = ECommerceRecommendationEngine.apply().train(ep)[0]
    for i in (5, 9, 21):
        insert("view", "late_user", f"i{i}")
    algo = ECommAlgorithm(ep.algorithms_params[0][1])
    white = [f"i{i}" for i in range(0, 60, 2)] + ["nope"]
    qs = list(enumerate([
        Query(user="u0", num=5),
        Query(user="u1", num=6, white_list=white),
        Query(user="u2", num=4, white_list=white, categories=["c0"],
              black_list=["i0", "i8"]),
        Query(user="u3", num=4, categories=["c1"]),
        Query(user="u4", num=3, white_list=["i3"]),
        Query(user="late_user", num=5, white_list=white,
              black_list=["i10"]),
        Query(user="late_user", num=5, white_list=white,
              categories=["c2"]),
        Query(user="late_user", num=5)]))
    single = [(i, algo.predict(model, q)) for i, q in qs]
    before = topk_ops.cand_stats()["calls"]
    batched = algo.batch_predict(model, qs)
    # one candidate call per group (known, cold), not one per query
    assert topk_ops.cand_stats()["calls"] - before == 2
    _same_results(batched, single)
    assert {s.item for s in single[2][1].item_scores} <= \
        {f"i{i}" for i in range(4, 60, 4)} - {"i8"}


def test_similar_batch_keeps_white_lists(mem_storage):
    from predictionio_amd.controller import EngineParams, Params
    from predictionio_amd.templates.similarproduct import (
        ALSAlgorithm, Query, SimilarProductEngine,
    )
    _seed_items(mem_storage, "MyTestApp", "view", 60, "item")
    ep = EngineParams(
        data_source_params=Params({"appName": "MyTestApp"}),
        algorithms_params=[("als", Params(
            {"rank": 8, "numIterations": 4, "seed": 7}))])
    model = SimilarProductEngine.apply().train(ep)[0]
    algo = ALSAlgorithm(ep.algorithms_params[0][1])
    white = [f"i{i}" for i in range(1, 60, 2)]
    qs = list(enumerate([
        Query(items=["i0"], num=5),
        Query(items=["i1", "i4"], num=6, white_list=white),
        Query(items=["i2"], num=4, white_list=white, categories=["c1"],
              black_list=["i5", "i9"]),
        Query(items=["i3"], num=4, categories=["c3"]),
        Query(items=["i7"], num=3, white_list=["i7", "i8"])]))
    single = [(i, algo.predict(model, q)) for i, q in qs]
    before = topk_ops.cand_stats()["calls"]
    batched = algo.batch_predict(model, qs)
    assert topk_ops.cand_stats()["calls"] - before == 1
    _same_results(batched, single)
    assert [s.item for s in single[4][1].item_scores] == ["i8"]
