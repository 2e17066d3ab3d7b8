"""indicator_topk_ref (the CPU path of indicator_topk) against a brute
force, every validation error, and the template's batch_predict."""

import pytest
import torch

from predictionio_amd.ops.cooccurrence import (
    indicator_topk, indicator_topk_ref,
)


def brute(ids, sc, queries, K, own=True, ban=None, allow=None, icats=None,
          qcats=None):
    """Dict of sums (int, or fp64 for float tables) per query, filtered,
    ordered by (-score, id), padded to K with -1 / 0. Plain lists in."""
    out_ids, out_sc = [], []
    for b, items in enumerate(queries):
        s = {}
        for i in items:
            for j, v in zip(ids[i], sc[i]):
                if j >= 0:
                    s[j] = s.get(j, 0) + v
        keep = [j for j in s
                if not (own and j in items)
                and not (ban is not None and j in ban[b])
                and (allow is None or j in allow[b])
                and (icats is None
                     or any(a & c for a, c in zip(icats[j], qcats[b])))]
        top = sorted(keep, key=lambda j: (-s[j], j))[:K]
        out_ids.append(top + [-1] * (K - len(top)))
        out_sc.append([s[j] for j in top] + [0] * (K - len(top)))
    return out_ids, out_sc


def csr(lists, device="cpu"):
    indptr = torch.tensor([0] + [len(x) for x in lists]).cumsum(0)
    flat = torch.tensor([x for y in lists for x in y], dtype=torch.int32)
    return indptr.to(device), flat.to(device)


def table(nr, n, n_cols, dtype, seed):
    """Random table: distinct ids per row, a random number of -1 pads at
    the row's end; counts in [0, 40] or multiples of 1/8 in [0, 64]."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(n_cols, generator=g)[:n]
                       for _ in range(nr)]).to(torch.int32)
    fill = torch.randint(0, n + 1, (nr, 1), generator=g)
    ids[torch.arange(n).unsqueeze(0) >= fill] = -1
    if dtype == torch.int32:
        sc = torch.randint(0, 41, (nr, n), generator=g, dtype=torch.int32)
    else:
        sc = torch.randint(0, 513, (nr, n), generator=g).float() / 8
    sc[ids < 0] = 0
    return ids, sc


NR, N, W = 40, 6, 4
# an empty query, single rows, a long one; query 5 gets an empty allow
# list (all candidates filtered) wherever an allow list is given
QUERIES = [[], [3], [0, 1, 2], [5, 9, 17, 30, 39], list(range(10, 30)), [7, 8]]
BAN = [[], [1, 2], [4, 5, 6, 7], list(range(0, 40, 2)), [11], [0]]
ALLOW = [[1], list(range(40)), list(range(20)), [2, 3, 31], list(range(5, 35)),
         []]
FILTERS = ["none", "own_off", "ban", "allow", "cats1", "cats4", "all"]


def filter_kw(name, device="cpu"):
    """(kwargs for the op, kwargs for brute) of one filter configuration."""
    op, br = {}, {}
    if name == "own_off":
        op["exclude_query"], br["own"] = False, False
    if name in ("ban", "all"):
        op["ban_indptr"], op["ban_indices"] = csr(BAN, device)
        br["ban"] = BAN
    if name in ("allow", "all"):
        op["allow_indptr"], op["allow_indices"] = csr(ALLOW, device)
        br["allow"] = ALLOW
    if name in ("cats1", "cats4", "all"):
        w = 1 if name == "cats1" else W
        g = torch.Generator().manual_seed(5)
        icats = torch.randint(-2 ** 31, 2 ** 31, (NR, w), generator=g,
                              dtype=torch.int64).to(torch.int32)
        icats &= torch.randint(-2 ** 31, 2 ** 31, (NR, w), generator=g,
                               dtype=torch.int64).to(torch.int32)
        qcats = (torch.ones((len(QUERIES), w), dtype=torch.int64)
                 << torch.randint(0, 32, (len(QUERIES), w), generator=g)
                 ).to(torch.int32)
        op["item_cats"], op["query_cats"] = icats.to(device), qcats.to(device)
        br["icats"], br["qcats"] = icats.tolist(), qcats.tolist()
    return op, br


@pytest.mark.parametrize("dtype", [torch.int32, torch.float32])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("K", [3, 64])  # 64: more than the candidates
def test_ref_matches_brute(dtype, filt, K):
    ids, sc = table(NR, N, NR, dtype, seed=1)
    op, br = filter_kw(filt)
    want_ids, want_sc = brute(ids.tolist(), sc.tolist(), QUERIES, K, **br)
    got_ids, got_sc = indicator_topk(ids, sc, *csr(QUERIES), K, **op)
    assert got_sc.dtype == dtype and got_ids.dtype == torch.int32
    assert got_ids.tolist() == want_ids
    assert got_sc.tolist() == want_sc   # eighths up to 64: fp32 sums exact
    assert got_ids[0].tolist() == [-1] * K            # the empty query
    if "allow" in op:
        assert got_ids[5].tolist() == [-1] * K        # all filtered
    # one query per chunk gives the same rows
    ch_ids, ch_sc = indicator_topk_ref(ids, sc, *csr(QUERIES), K, chunk=1,
                                       **op)
    assert torch.equal(ch_ids, got_ids) and torch.equal(ch_sc, got_sc)


def test_cross_table_ids_beyond_rows():
    ids, sc = table(8, 5, 1000, torch.float32, seed=2)
    qs = [[0, 1, 2, 3], [4, 7]]
    want = brute(ids.tolist(), sc.tolist(), qs, 8, own=False)
    got = indicator_topk(ids, sc, *csr(qs), 8, n_cols=1000,
                         exclude_query=False)
    assert (got[0].tolist(), got[1].tolist()) == want


def _bad(**kw):
    """Arguments of one valid call with some replaced."""
    ids, sc = table(NR, N, NR, torch.int32, seed=1)
    qp, qi = csr(QUERIES)
    a = dict(top_ids=ids, top_scores=sc, q_indptr=qp, q_items=qi, K=4)
    a.update(kw)
    return a


I32 = torch.int32
VALIDATION = {
    "K low": lambda: _bad(K=0),
    "K high": lambda: _bad(K=1025),
    "indptr start": lambda: _bad(q_indptr=torch.tensor([1, 2]),
                                 q_items=torch.tensor([0, 1], dtype=I32)),
    "indptr end": lambda: _bad(q_indptr=torch.tensor([0, 3]),
                               q_items=torch.tensor([0, 1], dtype=I32)),
    "indptr decreases": lambda: _bad(q_indptr=torch.tensor([0, 2, 1, 2]),
                                     q_items=torch.tensor([0, 1], dtype=I32)),
    "query not ascending": lambda: _bad(q_indptr=torch.tensor([0, 2]),
                                        q_items=torch.tensor([1, 1], dtype=I32)),
    "query item range": lambda: _bad(q_indptr=torch.tensor([0, 1]),
                                     q_items=torch.tensor([NR], dtype=I32)),
    "query dtype": lambda: _bad(q_items=csr(QUERIES)[1].long()),
    "ban range": lambda: _bad(ban_indptr=csr(BAN)[0],
                              ban_indices=csr(BAN)[1] + NR),
    "ban unsorted": lambda: _bad(ban_indptr=csr(BAN)[0],
                                 ban_indices=csr(BAN)[1].flip(0)),
    "ban half": lambda: _bad(ban_indptr=csr(BAN)[0]),
    "ban length": lambda: _bad(ban_indptr=csr(BAN[:-1])[0],
                               ban_indices=csr(BAN[:-1])[1]),
    "allow range": lambda: _bad(allow_indptr=csr(ALLOW)[0],
                                allow_indices=csr(ALLOW)[1] - 1),
    "cats half": lambda: _bad(item_cats=torch.ones((NR, 1), dtype=I32)),
    "cats W": lambda: _bad(item_cats=torch.ones((NR, 3), dtype=I32),
                           query_cats=torch.ones((6, 3), dtype=I32)),
    "cats rows": lambda: _bad(item_cats=torch.ones((NR + 1, 1), dtype=I32),
                              query_cats=torch.ones((6, 1), dtype=I32)),
    "cats dtype": lambda: _bad(item_cats=torch.ones((NR, 1)),
                               query_cats=torch.ones((6, 1))),
    "own needs square": lambda: _bad(n_cols=NR + 1),
    "count overflow": lambda: _bad(
        top_scores=torch.full((NR, N), 2 ** 31 // 20 + 1, dtype=I32)),
    "table id range": lambda: _bad(top_ids=torch.full((NR, N), NR, dtype=I32)),
    "table id below -1": lambda: _bad(
        top_ids=torch.full((NR, N), -2, dtype=I32)),
    "negative score": lambda: _bad(
        top_scores=torch.full((NR, N), -1, dtype=I32)),
    "nan score": lambda: _bad(
        top_scores=torch.full((NR, N), float("nan"))),
    "inf score": lambda: _bad(
        top_scores=torch.full((NR, N), float("inf"))),
    "score dtype": lambda: _bad(top_scores=torch.zeros((NR, N),
                                                       dtype=torch.float64)),
    "score shape": lambda: _bad(top_scores=torch.zeros((NR, N + 1),
                                                       dtype=I32)),
}


@pytest.mark.parametrize("case", list(VALIDATION))
@pytest.mark.parametrize("fn", [indicator_topk, indicator_topk_ref])
def test_validation_errors(case, fn):
    a = VALIDATION[case]()
    pos = [a.pop(k) for k in ("top_ids", "top_scores", "q_indptr", "q_items",
                              "K")]
    with pytest.raises(ValueError):
        fn(*pos, **a)


def test_check_table_off_skips_the_table_scan():
    a = _bad(top_ids=torch.full((NR, N), -2, dtype=I32))
    ids, _ = indicator_topk(a["top_ids"], a["top_scores"], a["q_indptr"],
                            a["q_items"], 4, check_table=False)
    assert (ids == -1).all()


def cooc_model(device=None):
    """A trained llr model on a small seeded event set, and queries that
    use every filter."""
    from predictionio_amd.controller import Params
    from predictionio_amd.templates.similarproduct.engine import (
        CooccurrenceAlgorithm, Item, PreparedData, Query, ViewEvent,
    )
    g = torch.Generator().manual_seed(2)  # no tied sums: asserted below
    pairs = torch.randint(0, 10 ** 6, (900, 2), generator=g)
    # 0.7 power: skewed item popularity, so LLR values spread out
    views = [ViewEvent(f"u{int(u) % 60}", f"i{int((int(i) % 1000) ** 0.7) % 45}",
                       0.0) for u, i in pairs.tolist()]
    items = {f"i{k}": Item(categories=[f"c{k % 3}", f"d{k % 5}"])
             for k in range(48)}
    algo = CooccurrenceAlgorithm(Params({"n": 8, "scoring": "llr"}))
    model = algo.train(PreparedData(users={}, items=items, view_events=views))
    if device is not None:
        model.to(device)
    queries = [
        Query(items=["i1", "i2", "i3"], num=5),
        Query(items=["i4", "nope", "i9"], num=4, categories=["c1"]),
        Query(items=["i10"], num=6, black_list=["i11", "i12", "zzz"]),
        Query(items=["i5", "i6", "i7", "i8"], num=3,
              white_list=[f"i{k}" for k in range(0, 40, 2)]),
        Query(items=["i20", "i21"], num=5, categories=["d2", "c0"],
              white_list=[f"i{k}" for k in range(30)], black_list=["i3"]),
        Query(items=["unknown"], num=3),
        Query(items=["i30", "i30", "i31"], num=4),   # repeated: via predict
        Query(items=["i40", "i41"], num=50),         # more than there are
        Query(items=["i2"], num=3, categories=["none"]),
    ]
    return algo, model, queries


def test_batch_predict_matches_predict():
    algo, model, queries = cooc_model()
    got = dict(algo.batch_predict(model, list(enumerate(queries))))
    assert len(got) == len(queries)
    nonempty = 0
    for i, q in enumerate(queries):
        # one more than asked for: the seed leaves no tied sum at the cut
        full = algo.predict(model, type(q)(**{**q.__dict__, "num": q.num + 1}))
        sc = [s.score for s in full.item_scores]
        assert len(set(sc)) == len(sc), "seed gives tied sums: pick another"
        want = full.item_scores[:q.num]
        assert [s.item for s in got[i].item_scores] == [s.item for s in want]
        m = len(q.items)
        for a, b in zip(got[i].item_scores, want):
            # ordered fp32 sum of m non-negative terms vs the fp64 sum
            assert abs(a.score - b.score) <= (m - 1) * 2.0 ** -24 * b.score
        nonempty += bool(want)
    assert nonempty >= 6
