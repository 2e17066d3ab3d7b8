"""GPU tests of the bf16 shortlist contract of `topk_score` at the K cut:
an item of the fp32 top K must be served when its bf16 rank among the
valid items is at most the route's depth D, on every route, at the
shapes the larger random tests never reach (B = 1, N < 64, slices
without a full chunk, an fp32/bf16 inversion placed exactly at the cut).

Routes: "default" (eager mfma), "union" (mode="union"), "list0" /
"list1" (PIO_TOPK_UNION=0, the list kernel, with the cross-slice
threshold off / on) and "fp32". Depths, by hand: fp32 is exact (D = N);
K <= 32 has D = 2K everywhere; 32 < K <= 64 has D = 2K where the union
path served the call and D = 64 where the list kernel did.

Run on an MI355X:
    python -m pytest tests/test_topk_shortlist_gpu.py -m gpu -q
"""

import numpy as np
import pytest
import torch

import _topk_oracle as orc

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

ROUTES = ["default", "union", "list0", "list1", "fp32"]


def _dev(t):
    return None if t is None else t.cuda()


def run_route(route, monkeypatch, Xq, Y, K, n_slices=None, **filters):
    """(values, indices, D) of `topk_score` on one route, on the CPU."""
    from predictionio_amd.ops import topk as topk_ops
    mode = None
    if route.startswith("list"):
        monkeypatch.setenv("PIO_TOPK_UNION", "0")
        monkeypatch.setenv("PIO_TOPK_GTH", route[-1])
    elif route != "default":
        mode = route
    calls = topk_ops.union_stats()["calls"]
    gv, gi = topk_ops.topk_score(
        Xq.cuda(), Y.cuda(), K, n_slices=n_slices, mode=mode,
        **{k: _dev(v) for k, v in filters.items()})
    torch.cuda.synchronize()
    served_by_union = topk_ops.union_stats()["calls"] == calls + 1
    if route == "union":
        assert served_by_union
    if route.startswith("list") or route == "fp32":
        assert not served_by_union
    N = Y.shape[0]
    if route == "fp32":
        D = N
    elif K <= 32 or served_by_union:
        D = 2 * K
    else:
        D = 64
    return gv.cpu(), gi.cpu(), D


def expect_no_union_plan(Xq, Y, K, n_slices=None):
    from predictionio_amd.ops import topk as topk_ops
    with pytest.raises(ValueError):
        topk_ops.topk_score(Xq.cuda(), Y.cuda(), K, n_slices=n_slices,
                            mode="union")


# ------------------------------------------------------ inversion at the cut

def _placement(name, K, d):
    """(N, n_slices, rows)."""
    if name == "n40":        # one contiguous slice (rows 20..39), to N - 1
        assert K + d <= 20
        N, rows = orc.place_tail(40, K, d)
        return N, 2, rows
    if name == "chunks":     # one special row per 64-item chunk
        N, rows = orc.place_per_chunk(K, d)
        assert N <= 1000
        return N, 3, rows
    if name == "n200":
        # the last of three contiguous slices (rows 134..199) while
        # K + d <= 66; K + d <= 8 is the 64-aligned tail chunk 192..199
        N, rows = orc.place_tail(200, K, d)
        return N, 3, rows
    if name == "n1000":      # default slicing; room for a K = 64 union plan
        N, rows = orc.place_tail(1000, K, d)
        return N, None, rows
    raise KeyError(name)


INVERSIONS = [
    # K, d, f, placement, B (the designed query is the last row)
    (1, 1, 32, "n40", 1),
    (4, 1, 8, "n40", 1),
    (4, 4, 32, "n40", 65),
    (4, 1, 64, "n40", 65),
    (4, 4, 128, "n40", 1),
    (1, 1, 64, "chunks", 65),
    (1, 1, 8, "chunks", 1),
    (4, 4, 32, "chunks", 1),
    (4, 1, 128, "chunks", 65),
    (1, 1, 128, "n200", 1),
    (4, 4, 8, "n200", 65),
    (20, 1, 32, "n200", 1),
    (20, 20, 64, "n200", 65),
    (32, 1, 8, "n200", 1),
    (32, 32, 128, "n200", 65),
    (32, 32, 32, "n200", 1),
    (33, 1, 64, "n200", 1),
    (33, 1, 128, "n200", 65),
    (64, 1, 32, "n200", 65),
    (64, 1, 8, "n200", 1),
    (64, 1, 128, "n1000", 1),
    (33, 33, 64, "n1000", 1),
    (64, 64, 32, "n1000", 65),
    # d = K + 1: beyond the contract of the bf16 routes
    (4, 5, 32, "n40", 1),
    (20, 21, 64, "n200", 65),
]

_inversions = {}


def _inversion(K, d, f, place, B):
    key = (K, d, f, place, B)
    if key not in _inversions:
        N, ns, rows = _placement(place, K, d)
        Xq, Y, info = orc.designed_inversion(K, d, f, N, rows, B=B,
                                             qrow=B - 1, seed=K + d)
        _inversions[key] = (Xq, Y, info, ns, {})
    return _inversions[key]


def _oracle(cache, Xq, Y, K, D, **filters):
    if (K, D) not in cache:
        cache[(K, D)] = orc.Oracle(Xq, Y, K, D, **filters)
    return cache[(K, D)]


@requires_gpu
class TestInversionAtTheCut:
    @pytest.mark.parametrize("route", ROUTES)
    @pytest.mark.parametrize("K,d,f,place,B", INVERSIONS)
    def test_target_is_served_at_rank_k(self, K, d, f, place, B, route,
                                        monkeypatch):
        """The target has fp32 rank K and bf16 rank K + d. Whenever
        K + d is within the route's depth it comes back at rank K behind
        the leaders. (K = 64, d = 1 on the list kernel has K + d = 65 >
        D = 64: there, as for d = K + 1, only the oracle's checks
        apply.)"""
        Xq, Y, info, ns, cache = _inversion(K, d, f, place, B)
        N = Y.shape[0]
        if route == "union" and (N <= 64 or (K == 64 and N == 200)):
            # one chunk; or four chunks, too few for 128 candidates in
            # lists short enough never to fill by chance
            expect_no_union_plan(Xq, Y, K, ns)
            return
        gv, gi, D = run_route(route, monkeypatch, Xq, Y, K, n_slices=ns)
        o = _oracle(cache, Xq, Y, K, D)
        q = info["qrow"]
        print(f"K={K} d={d} f={f} {place} B={B} {route}: D={D}, "
              f"served {gi[q].tolist()[-3:]}, target {info['target']}")
        o.check(gv, gi)
        assert gi[q, :K - 1].tolist() == info["leaders"]
        if K + d <= D:
            assert o.must[q, info["target"]]
            assert gi[q].tolist() == info["fp32_top"]
            assert gv[q, K - 1].item() == 2 + 6 / 1024


# ------------------------------------------------ filtered items, no depth

def _blocked(K, f, B, how, W):
    """The d = K inversion in the last rows of N = 200, plus 2K items
    that outscore everything: K in rows 0..K-1 (another slice) and K
    right before the special rows (the same slice). `how` says which
    filter removes them; "all" deals them round-robin to the three."""
    N, rows = orc.place_tail(200, K, K)
    Xq, Y, info = orc.designed_inversion(K, K, f, N, rows, B=B, qrow=B - 1,
                                         seed=77)
    q = info["qrow"]
    blockers = list(range(K)) + list(range(N - 3 * K, N - 2 * K))
    for i, r in enumerate(blockers):
        Y[r, :2] = 100.0 + i
    kinds = {"mask": ["mask"], "bans": ["bans"], "cats": ["cats"],
             "all": ["mask", "bans", "cats"]}[how]
    by = {k: [r for i, r in enumerate(blockers)
              if kinds[i % len(kinds)] == k] for k in kinds}
    filters = {}
    if "mask" in by:
        mask = torch.zeros(N, dtype=torch.uint8)
        mask[by["mask"]] = 1
        filters["item_mask"] = mask
    if "bans" in by:
        # only the designed query bans them
        n = len(by["bans"])
        indptr = torch.zeros(B + 1, dtype=torch.int64)
        indptr[q + 1:] = n
        filters["ban_indptr"] = indptr
        filters["ban_indices"] = torch.tensor(sorted(by["bans"]),
                                              dtype=torch.int32)
    if "cats" in by:
        # blockers carry the top bit of the last word only; every other
        # item carries bit 0 of word 0 too; queries accept bit 0
        words = np.zeros((N, W), dtype=np.uint32)
        words[:, 0] = 1
        words[:, W - 1] |= np.uint32(1 << 31)
        words[by["cats"], 0] &= ~np.uint32(1)
        qwords = np.zeros((B, W), dtype=np.uint32)
        qwords[:, 0] = 1
        filters["item_cats"] = torch.from_numpy(words.view(np.int32))
        filters["query_cats"] = torch.from_numpy(qwords.view(np.int32))
    return Xq, Y, info, filters


BLOCKED = [
    # K, f, B, how, W
    (4, 64, 1, "mask", 1),
    (4, 8, 65, "bans", 1),
    (4, 64, 65, "cats", 1),
    (4, 32, 1, "cats", 4),
    (4, 64, 65, "all", 4),
    (20, 64, 65, "mask", 1),
    (20, 128, 1, "bans", 1),
    (20, 8, 1, "cats", 1),
    (20, 64, 65, "cats", 4),
    (20, 32, 1, "all", 1),
]

_blocked_cache = {}


@requires_gpu
class TestFilteredItemsTakeNoDepth:
    @pytest.mark.parametrize("route", ROUTES)
    @pytest.mark.parametrize("K,f,B,how,W", BLOCKED)
    def test_target_survives_2k_filtered_leaders(self, K, f, B, how, W,
                                                 route, monkeypatch):
        key = (K, f, B, how, W)
        if key not in _blocked_cache:
            _blocked_cache[key] = _blocked(*key) + ({},)
        Xq, Y, info, filters, cache = _blocked_cache[key]
        gv, gi, D = run_route(route, monkeypatch, Xq, Y, K, n_slices=3,
                              **filters)
        o = _oracle(cache, Xq, Y, K, D, **filters)
        q = info["qrow"]
        assert o.must[q].nonzero().flatten().tolist() == \
            sorted(info["fp32_top"])
        o.check(gv, gi)
        assert gi[q].tolist() == info["fp32_top"]


# ------------------------------------------- same query, different company

@requires_gpu
class TestSameQueryDifferentCompany:
    @pytest.mark.parametrize("route", ["default", "list0", "list1", "fp32"])
    def test_alone_and_in_a_batch(self, route, monkeypatch):
        """The designed query alone at K = 4, then as row 5 of a 9-row
        batch at K = 10 (a batch is served at its largest `num`): the
        first four (item, score) pairs are the same."""
        K, d = 4, 4
        N, rows = orc.place_tail(40, K, d)
        Xq9, Y, info = orc.designed_inversion(K, d, 32, N, rows, B=9,
                                              qrow=5, seed=3)
        x1 = Xq9[5:6].clone()
        v1, i1, _ = run_route(route, monkeypatch, x1, Y, K)
        v9, i9, D9 = run_route(route, monkeypatch, Xq9, Y, 10)
        orc.Oracle(Xq9, Y, 10, D9).check(v9, i9)
        assert i1[0].tolist() == info["fp32_top"]
        assert torch.equal(i9[5, :K], i1[0])
        assert torch.equal(v9[5, :K], v1[0])


# ------------------------------------------------------- clustered catalog

CLUSTERED = [(70, 1000, 32, 5, 1), (70, 1000, 64, 20, 2),
             (130, 333, 128, 32, 4)]
_clustered = {}


@requires_gpu
class TestClusteredCatalog:
    @pytest.mark.parametrize("route", ["default", "list0", "list1"])
    @pytest.mark.parametrize("B,N,f,K,seed", CLUSTERED)
    def test_contract_on_clustered_factors(self, B, N, f, K, seed, route,
                                           monkeypatch):
        key = (B, N, f, K, seed)
        if key not in _clustered:
            Xq, Y = orc.clustered_catalog(B, N, f, seed)
            _clustered[key] = (Xq, Y, orc.Oracle(Xq, Y, K, 2 * K))
        Xq, Y, o = _clustered[key]
        gv, gi, D = run_route(route, monkeypatch, Xq, Y, K)
        assert D == 2 * K
        share = o.check(gv, gi)
        top = torch.topk(o.s, K, dim=1).indices
        hits = (gi.unsqueeze(2) == top.unsqueeze(1)).any(dim=1).sum().item()
        print(f"clustered B={B} N={N} f={f} K={K} {route}: excluded share "
              f"{100 * share:.2f}%, recall {hits / (B * K):.4f}")
        assert share <= 0.01


# ------------------------------------------ tiny catalogs, integer problem

@requires_gpu
class TestTinyCatalogs:
    @pytest.mark.parametrize("route", ROUTES)
    @pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 129])
    def test_exact_on_integers(self, N, route, monkeypatch):
        """Distinct integer scores: values and indices equal the float64
        reference exactly, with -1 / -inf exactly where K > N."""
        from predictionio_amd.ops import topk as topk_ops
        f = 20
        Xq3, Y = orc.int_problem(3, N, f)
        for B in (1, 3):
            Xq = Xq3[:B]
            for K in (1, 5, 64):
                rv, ri = orc.reference_topk(Xq, Y, K)
                assert (ri[:, min(K, N):] == -1).all()
                assert (ri[:, :min(K, N)] >= 0).all()
                for ns in (None, 2, 7):
                    if route == "union":
                        if N <= 64:
                            expect_no_union_plan(Xq, Y, K, ns)
                            continue
                        try:
                            gv, gi = topk_ops.topk_score(
                                Xq.cuda(), Y.cuda(), K, n_slices=ns,
                                mode="union")
                        except ValueError:
                            continue        # no plan for this K at this N
                        gv, gi = gv.cpu(), gi.cpu()
                    else:
                        gv, gi, _ = run_route(route, monkeypatch, Xq, Y, K,
                                              n_slices=ns)
                    what = f"N={N} B={B} K={K} n_slices={ns} {route}"
                    assert torch.equal(gi, ri), what
                    assert torch.equal(gv, rv), what

    @pytest.mark.parametrize("route", ["default", "list0", "list1", "fp32"])
    def test_filters_leave_fewer_than_k(self, route, monkeypatch):
        """N = 65 with 60 items masked and one more banned per query:
        four or five valid items for K = 5 and K = 64."""
        N, f, B = 65, 20, 3
        Xq, Y = orc.int_problem(B, N, f, seed=1)
        mask = torch.ones(N, dtype=torch.uint8)
        mask[[0, 31, 63, 64, 40]] = 0
        indptr = torch.tensor([0, 1, 1, 2], dtype=torch.int64)
        indices = torch.tensor([64, 0], dtype=torch.int32)
        filters = dict(item_mask=mask, ban_indptr=indptr,
                       ban_indices=indices)
        for K in (5, 64):
            o = orc.Oracle(Xq, Y, K, N, **filters)
            assert o.n_valid.tolist() == [4, 5, 4]
            rv, ri = orc.reference_topk(Xq, Y, K, o.valid)
            for ns in (None, 2, 7):
                gv, gi, _ = run_route(route, monkeypatch, Xq, Y, K,
                                      n_slices=ns, **filters)
                o.check(gv, gi)
                assert torch.equal(gi, ri) and torch.equal(gv, rv)
