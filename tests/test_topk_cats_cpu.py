"""Per-query category filters, CPU side: the torch reference against a
brute-force filter, CategoryBits against CategoryMasks, and the batched
`batch_predict` of the two filter-carrying templates against per-query
`predict` (including how many fused launches a batch costs)."""

import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from predictionio_amd.data.bimap import BiMap
from predictionio_amd.data.events import DataMap, Event, utcnow
from predictionio_amd.data.storage.base import App
from predictionio_amd.ops import topk as topk_ops
from predictionio_amd.templates.common import CategoryBits, CategoryMasks


def _words(bits_per_row, W):
    """rows of bit positions -> int32 [rows, W] (built as uint32 so bit
    31 is an ordinary bit)."""
    out = np.zeros((len(bits_per_row), W), dtype=np.uint32)
    for r, bits in enumerate(bits_per_row):
        for b in bits:
            out[r, b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    return torch.from_numpy(out.view(np.int32))


class TestRefAgainstBruteForce:
    @pytest.mark.parametrize("W", [1, 2, 4])
    def test_brute_force(self, W):
        g = torch.Generator().manual_seed(10 + W)
        rng = random.Random(W)
        B, N, f, K = 5, 200, 8, 10
        Xq = torch.randn((B, f), generator=g)
        Y = torch.randn((N, f), generator=g)
        ncat = 32 * W - 1           # category c owns bit c + 1
        top_bit = 32 * W - 1        # lives in word W-1 only
        rare, rare_members = 5, [3, 77, 150]   # fewer than K members
        item_bits = []
        for j in range(N):
            cats = {c for c in rng.sample(range(ncat), 2) if c != rare}
            if j in rare_members:
                cats.add(rare)
            if j % 9 == 0:
                cats.add(30)                    # bit 31 of word 0
            if j % 7 == 0:
                cats.add(top_bit - 1)           # bit in word W-1
            item_bits.append([0] + [c + 1 for c in cats])
        item_cats = _words(item_bits, W)
        query_bits = [[31],          # the category on bit 31
                      [top_bit],     # a category living in word W-1 only
                      [],            # zero words: nothing passes
                      [0],           # ANY only: unfiltered
                      [rare + 1]]    # fewer than K members
        query_cats = _words(query_bits, W)
        rv, ri = topk_ops.topk_score_ref(Xq, Y, K, item_cats=item_cats,
                                         query_cats=query_cats)
        scores = (Xq @ Y.t()).tolist()
        for b in range(B):
            want = set(query_bits[b])
            cand = sorted(((scores[b][j], j) for j in range(N)
                           if want & set(item_bits[j])), reverse=True)[:K]
            exp_i = [j for _, j in cand] + [-1] * (K - len(cand))
            exp_v = [s for s, _ in cand] + [float("-inf")] * (K - len(cand))
            assert ri[b].tolist() == exp_i, f"query {b}"
            assert torch.allclose(rv[b], torch.tensor(exp_v), atol=1e-6)
        assert (ri[2] == -1).all() and torch.isinf(rv[2]).all()
        uv, ui = topk_ops.topk_score_ref(Xq, Y, K)
        assert torch.equal(ri[3], ui[3]) and torch.equal(rv[3], uv[3])
        assert sorted(ri[4][:3].tolist()) == rare_members
        assert (ri[4][3:] == -1).all() and torch.isinf(rv[4][3:]).all()
        # bit 31 / word W-1 queries really select something
        assert (ri[0] >= 0).any() and (ri[1] >= 0).any()

    def test_contract_violations_raise(self):
        Xq, Y = torch.randn(3, 8), torch.randn(20, 8)
        ic = torch.ones((20, 1), dtype=torch.int32)
        qc = torch.ones((3, 1), dtype=torch.int32)
        with pytest.raises(ValueError):
            topk_ops.topk_score(Xq, Y, 4, item_cats=ic)
        with pytest.raises(ValueError):
            topk_ops.topk_score(Xq, Y, 4, item_cats=ic.long(), query_cats=qc)
        with pytest.raises(ValueError):
            topk_ops.topk_score(Xq, Y, 4, item_cats=ic,
                                query_cats=torch.ones((3, 2),
                                                      dtype=torch.int32))
        with pytest.raises(ValueError):
            topk_ops.topk_score(
                Xq, Y, 4,
                item_cats=torch.ones((20, 3), dtype=torch.int32),
                query_cats=torch.ones((3, 3), dtype=torch.int32))
        with pytest.raises(ValueError):
            topk_ops.topk_score(Xq, Y, 4, item_cats=ic[:19], query_cats=qc)


class TestCategoryBits:
    def _catalog(self, n_items, n_cats, seed=3):
        rng = random.Random(seed)
        names = [f"c{c}" for c in range(n_cats)]
        items = {}
        for j in range(n_items):
            if j < n_cats:
                cats = [names[j]]              # every category is used
            elif j % 13 == 0:
                cats = None                    # item without categories
            else:
                cats = rng.sample(names, rng.randint(1, 3))
            items[f"i{j}"] = SimpleNamespace(categories=cats)
        items["ghost"] = SimpleNamespace(categories=[names[0]])  # unmapped
        item_map = BiMap.string_int([f"i{j}" for j in range(n_items)])
        return items, item_map

    def test_matches_category_masks(self):
        items, item_map = self._catalog(300, 40)
        dev = torch.device("cpu")
        bits = CategoryBits.build(items, item_map, dev)
        masks = CategoryMasks.build(items, item_map, dev)
        assert bits.W == 2
        assert bits.item_words.shape == (300, 2)
        assert bits.item_words.dtype == torch.int32
        for cats in (None, [], ["nope"], ["c7"], ["c1", "c33", "c39"],
                     ["c39", "nope"]):
            qw = torch.from_numpy(bits.query_words(cats))
            assert qw.dtype == torch.int32 and qw.shape == (2,)
            hit = ((bits.item_words & qw.unsqueeze(0)) != 0).any(dim=1)
            if cats is None:
                assert hit.all()
            else:
                assert torch.equal(hit, masks.banned_outside(cats) == 0), cats
        assert not torch.from_numpy(bits.query_words([])).any()
        assert not torch.from_numpy(bits.query_words(["nope"])).any()

    @pytest.mark.parametrize("n_cats,W", [(31, 1), (32, 2), (63, 2),
                                          (64, 4), (127, 4)])
    def test_word_count(self, n_cats, W):
        items, item_map = self._catalog(140, n_cats)
        bits = CategoryBits.build(items, item_map, torch.device("cpu"))
        assert bits.W == W
        # the last category owns the top bit in use, bit 31 included
        last = torch.from_numpy(bits.query_words([f"c{n_cats - 1}"]))
        hit = ((bits.item_words & last.unsqueeze(0)) != 0).any(dim=1)
        want = torch.tensor([bool(items[f"i{j}"].categories)
                             and f"c{n_cats - 1}" in items[f"i{j}"].categories
                             for j in range(140)])
        assert torch.equal(hit, want)

    def test_too_many_categories(self):
        items, item_map = self._catalog(200, 128)
        assert CategoryBits.build(items, item_map,
                                  torch.device("cpu")) is None


# ------------------------------------------------------------ templates

N_USERS, N_ITEMS, N_CATS = 60, 40, 5


def _mk_app(storage, name="MyTestApp"):
    app_id = storage.get_meta_data_apps().insert(App(id=0, name=name))
    storage.get_l_events().init(app_id)
    return app_id


def _insert(storage, app_id, event, uid, iid=None, props=None,
            entity_type="user", target_type="item"):
    e = Event(event=event, entity_type=entity_type, entity_id=uid,
              target_entity_type=target_type if iid else None,
              target_entity_id=iid, properties=DataMap(props or {}),
              event_time=utcnow())
    storage.get_l_events().insert(e, app_id)


def _seed(storage, app_id, buys):
    rng = random.Random(5)
    for i in range(N_ITEMS):
        cats = [f"c{i % N_CATS}"] + (["c0"] if i % 7 == 0 else [])
        _insert(storage, app_id, "$set", f"i{i}", None,
                {"categories": cats}, entity_type="item")
    for u in range(N_USERS):
        liked = [i for i in range(N_ITEMS) if i % 3 == u % 3]
        for i in rng.sample(liked, 5) + rng.sample(range(N_ITEMS), 2):
            _insert(storage, app_id, "view", f"u{u}", f"i{i}")
        if buys:
            _insert(storage, app_id, "buy", f"u{u}", f"i{rng.randrange(8)}")


def _assert_same(batched, single):
    assert [i for i, _ in batched] == [i for i, _ in single]
    for (i, rb), (_, rs) in zip(batched, single):
        assert [s.item for s in rb.item_scores] == \
            [s.item for s in rs.item_scores], f"query {i}"
        for a, b in zip(rb.item_scores, rs.item_scores):
            assert abs(a.score - b.score) <= 1e-5, f"query {i}"


def _count_topk(monkeypatch):
    calls = []
    real = topk_ops.topk_score

    def counting(*a, **kw):
        calls.append(a[0].shape[0])
        return real(*a, **kw)

    monkeypatch.setattr(topk_ops, "topk_score", counting)
    return calls


class TestECommBatchPredict:
    def _train(self, storage, extra=None):
        from predictionio_amd.controller import EngineParams, Params
        from predictionio_amd.templates.ecommercerecommendation import (
            ECommAlgorithm, ECommerceRecommendationEngine,
        )
        app_id = _mk_app(storage)
        _seed(storage, app_id, buys=True)
        p = {"appName": "MyTestApp", "unseenOnly": True,
             "seenEvents": ["buy", "view"], "similarEvents": ["view"],
             "rank": 8, "numIterations": 6, "seed": 11}
        p.update(extra or {})
        ep = EngineParams(
            data_source_params=Params({"appName": "MyTestApp"}),
            algorithms_params=[("ecomm", Params(p))])
        model = ECommerceRecommendationEngine.apply().train(ep)[0]
        # events after training: late_user is unknown to the model but has
        # recent views; then the unavailable-items constraint
        for i in (5, 9, 5, 21):
            _insert(storage, app_id, "view", "late_user", f"i{i}")
        _insert(storage, app_id, "$set", "unavailableItems", None,
                {"items": ["i2", "i4", "i17", "not-an-item"]},
                entity_type="constraint")
        return ECommAlgorithm(ep.algorithms_params[0][1]), model

    def _queries(self):
        from predictionio_amd.templates.ecommercerecommendation import Query
        return [
            Query(user="u0", num=5),
            Query(user="u1", num=8, categories=["c1"]),
            Query(user="u2", num=4, categories=["c0", "c3"]),
            Query(user="u3", num=6, black_list=["i1", "i6", "i30", "zzz"]),
            Query(user="u4", num=5, white_list=["i1", "i8", "i9", "i20"]),
            Query(user="late_user", num=5),                 # cold + recent
            Query(user="late_user", num=3, categories=["c2"]),
            Query(user="ghost", num=4),                     # cold, default
            Query(user="ghost", num=3, categories=["c1"]),
            Query(user="u5", num=7, categories=["unknown"]),
            Query(user="u6", num=3, categories=[]),
            Query(user="u7", num=10, categories=["c4"],
                  black_list=["i4", "i9"]),
            {"user": "u8", "num": 2, "categories": ["c2"]},
        ]

    def test_matches_predict(self, mem_storage):
        algo, model = self._train(mem_storage)
        qs = list(enumerate(self._queries()))
        single = [(i, algo.predict(model, q)) for i, q in qs]
        _assert_same(algo.batch_predict(model, qs), single)
        # the mix really exercises the filters
        assert single[0][1].item_scores and single[5][1].item_scores
        assert single[7][1].item_scores
        assert single[9][1].item_scores == []

    def test_matches_predict_weighted(self, mem_storage):
        algo, model = self._train(mem_storage, {"weightedItems": [
            {"items": ["i0", "i3", "i6", "i9"], "weight": 0.01},
            {"items": ["i1", "i9"], "weight": 5.0}]})
        qs = list(enumerate(self._queries()))
        _assert_same(algo.batch_predict(model, qs),
                     [(i, algo.predict(model, q)) for i, q in qs])

    def test_launch_count(self, mem_storage, monkeypatch):
        from predictionio_amd.templates.ecommercerecommendation import Query
        algo, model = self._train(mem_storage)
        qs = list(enumerate(
            [Query(user=f"u{u}", num=4 + u % 3,
                   categories=[f"c{u % N_CATS}"] if u % 2 else None)
             for u in range(9)]
            + [Query(user="late_user", num=5),
               Query(user="late_user", num=2, categories=["c1"]),
               Query(user="ghost", num=3)]))
        assert len(qs) == 12
        calls = _count_topk(monkeypatch)
        res = algo.batch_predict(model, qs)
        assert len(calls) <= 2, calls
        assert sorted(calls) == [2, 9]
        assert [i for i, _ in res] == list(range(12))

    def test_no_bits_falls_back(self, mem_storage, monkeypatch):
        algo, model = self._train(mem_storage)
        model.category_bits = None          # e.g. more than 127 categories
        qs = list(enumerate(self._queries()))
        single = [(i, algo.predict(model, q)) for i, q in qs]
        calls = _count_topk(monkeypatch)
        _assert_same(algo.batch_predict(model, qs), single)
        assert calls and set(calls) == {1}

    def test_lazy_rebuild(self, mem_storage):
        algo, model = self._train(mem_storage)
        assert model.category_bits is not None
        del model.__dict__["category_bits"]       # a model pickled before
        del model.__dict__["_cat_bits_built"]
        assert model.cat_bits().W == 1


class TestSimilarBatchPredict:
    def _train(self, storage):
        from predictionio_amd.controller import EngineParams, Params
        from predictionio_amd.templates.similarproduct import (
            ALSAlgorithm, SimilarProductEngine,
        )
        app_id = _mk_app(storage)
        _seed(storage, app_id, buys=False)
        ep = EngineParams(
            data_source_params=Params({"appName": "MyTestApp"}),
            algorithms_params=[("als", Params(
                {"rank": 8, "numIterations": 6, "seed": 7}))])
        model = SimilarProductEngine.apply().train(ep)[0]
        return ALSAlgorithm(ep.algorithms_params[0][1]), model

    def _queries(self):
        from predictionio_amd.templates.similarproduct import Query
        return [
            Query(items=["i0"], num=5),
            Query(items=["i1", "i4"], num=8, categories=["c1"]),
            Query(items=["i2", "i2", "nope"], num=4,
                  categories=["c0", "c3"]),
            Query(items=["i3"], num=6, black_list=["i6", "i9", "zzz"]),
            Query(items=["i5"], num=5, white_list=["i1", "i8", "i9", "i5"]),
            Query(items=["nope"], num=5),
            Query(items=["i7"], num=3, categories=["unknown"]),
            Query(items=["i8"], num=3, categories=[]),
            Query(items=["i9", "i10"], num=10, categories=["c4"],
                  black_list=["i4", "i14"]),
            {"items": ["i11"], "num": 2, "categories": ["c2"]},
        ]

    def test_matches_predict(self, mem_storage):
        algo, model = self._train(mem_storage)
        qs = list(enumerate(self._queries()))
        single = [(i, algo.predict(model, q)) for i, q in qs]
        _assert_same(algo.batch_predict(model, qs), single)
        assert single[0][1].item_scores and single[1][1].item_scores
        assert single[5][1].item_scores == []

    def test_launch_count(self, mem_storage, monkeypatch):
        from predictionio_amd.templates.similarproduct import Query
        algo, model = self._train(mem_storage)
        qs = list(enumerate(
            [Query(items=[f"i{j}", f"i{(j * 3) % N_ITEMS}"], num=3 + j % 4,
                   categories=[f"c{j % N_CATS}"] if j % 2 else None,
                   black_list=[f"i{j + 1}"] if j % 3 == 0 else None)
             for j in range(12)]))
        calls = _count_topk(monkeypatch)
        res = algo.batch_predict(model, qs)
        assert calls == [12]
        assert [i for i, _ in res] == list(range(12))


class TestRecommendedUserBatchPredict:
    """The recommended-user variant inherits the batched path: it has its
    own query type, and its per-query fallbacks (whiteList, no category
    bits) must not re-enter the subclass's predict with a parsed Query."""

    def _train(self, storage):
        from predictionio_amd.controller import EngineParams, Params
        from predictionio_amd.templates.similarproduct.engine import (
            RecommendedUserAlgorithm, RecommendedUserEngine,
        )
        app_id = _mk_app(storage, "FollowApp")
        rng = random.Random(8)
        for u in range(40):
            liked = [t for t in range(20) if t % 2 == u % 2]
            for t in rng.sample(liked, 4) + rng.sample(range(20), 1):
                _insert(storage, app_id, "follow", f"u{u}", f"s{t}",
                        target_type="user")
        ep = EngineParams(
            data_source_params=Params({"appName": "FollowApp"}),
            algorithms_params=[("als", Params(
                {"rank": 8, "numIterations": 6, "seed": 4}))])
        model = RecommendedUserEngine.apply().train(ep)[0]
        return RecommendedUserAlgorithm(ep.algorithms_params[0][1]), model

    def _queries(self):
        from predictionio_amd.templates.similarproduct.engine import (
            UserQuery,
        )
        return [
            UserQuery(users=["s0"], num=3),
            UserQuery(users=["s2"], num=3, white_list=["s3", "s4", "s6"]),
            UserQuery(users=["s1", "s5"], num=5, black_list=["s3", "s7"]),
            UserQuery(users=["nobody"], num=4),
            {"users": ["s4"], "num": 2, "whiteList": ["s0", "s8"]},
            {"users": ["s6", "s6"], "num": 6},
        ]

    def test_matches_predict(self, mem_storage, monkeypatch):
        algo, model = self._train(mem_storage)
        qs = list(enumerate(self._queries()))
        single = [(i, algo.predict(model, q)) for i, q in qs]
        calls = _count_topk(monkeypatch)
        _assert_same(algo.batch_predict(model, qs), single)
        assert sorted(calls) == [1, 1, 3]     # two whiteLists + one batch
        assert single[0][1].item_scores and single[1][1].item_scores
        assert {s.item for s in single[1][1].item_scores} <= \
            {"s3", "s4", "s6"}
        assert single[3][1].item_scores == []

    def test_no_bits_falls_back(self, mem_storage):
        algo, model = self._train(mem_storage)
        model.category_bits = None
        qs = list(enumerate(self._queries()))
        _assert_same(algo.batch_predict(model, qs),
                     [(i, algo.predict(model, q)) for i, q in qs])


class TestModelBitsFlag:
    def test_constructed_without_bits_builds_lazily(self):
        from predictionio_amd.templates.similarproduct.engine import (
            Item, SimilarModel,
        )
        items = {f"i{j}": Item(categories=[f"c{j % 3}"]) for j in range(9)}
        item_map = BiMap.string_int(list(items))
        Yn = torch.nn.functional.normalize(torch.randn(9, 8), dim=1)
        lazy = SimilarModel(Yn, item_map, items)
        assert lazy.category_bits is None and lazy.cat_bits().W == 1
        final = SimilarModel(Yn, item_map, items, None, None,
                             category_bits_built=True)
        assert final.cat_bits() is None       # "too many categories" stays
