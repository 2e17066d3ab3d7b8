"""GPU tests of the per-query category filter in the fused top-K kernels
(`topk_score(..., item_cats=, query_cats=)`), both kernel modes, against
the torch reference and the filter definition itself.

Run on an MI355X: python -m pytest tests/test_topk_cats_gpu.py -m gpu -q
"""

import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

RARE_CAT = 1  # the category of query 1, cut down to RARE_MEMBERS below


def _pack(bit_rows, W):
    out = np.zeros((len(bit_rows), W), dtype=np.uint32)
    for r, bits in enumerate(bit_rows):
        for b in bits:
            out[r, b >> 5] |= np.uint32(1) << np.uint32(b & 31)
    return torch.from_numpy(out.view(np.int32))


def _rare_members(N):
    # first and last item, and items around the slice seams of n_slices=7
    return sorted({0, 1, 714, 715, 2859, N - 2, N - 1})


_problems = {}


def _problem(B, N, f, W):
    """Seeded inputs + the filter as a dense bool matrix, built once per
    shape and shared (never modified) by the tests that use it."""
    key = (B, N, f, W)
    if key in _problems:
        return _problems[key]
    g = torch.Generator().manual_seed(1000 * W + f + B)
    rng = random.Random(7 * W + f + B)
    Xq = torch.randn((B, f), generator=g).float()
    Y = torch.randn((N, f), generator=g).float()
    ncat = 32 * W - 1                      # category c owns bit c + 1
    rare = set(_rare_members(N))
    item_bits = []
    for j in range(N):
        cats = set(rng.sample(range(ncat), rng.randint(1, 2)))
        cats.discard(RARE_CAT)
        if j in rare:
            cats.add(RARE_CAT)
        item_bits.append([0] + [c + 1 for c in cats])   # bit 0 = ANY
    query_bits = []
    for b in range(B):
        if b % 11 == 0:
            query_bits.append([])           # zero words: nothing passes
        elif b % 5 == 0:
            query_bits.append([0])          # ANY only: no filter
        else:
            query_bits.append([b % ncat + 1])
    item_cats = _pack(item_bits, W)
    query_cats = _pack(query_bits, W)
    hit = torch.zeros((B, N), dtype=torch.bool)
    for w in range(W):
        hit |= (item_cats[:, w].unsqueeze(0)
                & query_cats[:, w].unsqueeze(1)) != 0
    p = dict(Xq=Xq, Y=Y, item_cats=item_cats, query_cats=query_cats,
             hit=hit, scores=Xq @ Y.t(), refs={})
    _problems[key] = p
    return p


def _ref(p, K):
    from predictionio_amd.ops import topk as topk_ops
    if K not in p["refs"]:
        p["refs"][K] = topk_ops.topk_score_ref(
            p["Xq"], p["Y"], K, item_cats=p["item_cats"],
            query_cats=p["query_cats"])
    return p["refs"][K]


def _check(p, K, gv, gi):
    B, N = p["hit"].shape
    valid = gi >= 0
    # every returned item passes its own query's filter — no exceptions
    assert p["hit"].gather(1, gi.clamp_min(0))[valid].all()
    # returned values are the fp32 dots of the returned items
    chosen = p["scores"].gather(1, gi.clamp_min(0))
    assert torch.allclose(gv[valid], chosen[valid], atol=1e-5, rtol=1e-5), \
        f"max |value - dot| {(gv[valid] - chosen[valid]).abs().max()}"
    # and they are the reference's top-K values
    rv, _ = _ref(p, K)
    assert torch.allclose(gv, rv, atol=1e-4, rtol=1e-4), \
        f"max val diff {(gv[valid] - rv[valid]).abs().max()}"
    # each query returns min(K, candidates) distinct items, then padding
    n_cand = p["hit"].sum(dim=1)
    assert torch.equal(valid.sum(dim=1), n_cand.clamp(max=K))
    for b in range(B):
        got = gi[b][valid[b]].tolist()
        assert len(set(got)) == len(got)
        assert not valid[b][len(got):].any()          # padding at the tail
        if b % 11 == 0:                               # zero-word query
            assert (gi[b] == -1).all() and torch.isinf(gv[b]).all()
    # query 1 filters on the rare category: exactly its members come back
    members = _rare_members(N)
    got1 = gi[1][valid[1]].tolist()
    if K >= len(members):
        assert sorted(got1) == members
    else:
        assert set(got1) <= set(members)


MFMA_CASES = [(32, 20), (64, 20), (128, 20), (64, 1)]
FP32_CASES = [(16, 20), (64, 20)]
CASES = ([("mfma", f, K) for f, K in MFMA_CASES]
         + [("fp32", f, K) for f, K in FP32_CASES])


@requires_gpu
class TestTopKCategoryFilter:
    @pytest.mark.parametrize("W", [1, 2, 4])
    @pytest.mark.parametrize("mode,f,K", CASES)
    def test_sliced(self, mode, f, K, W):
        """B=37, N=5000, 7 slices of 715: a tail chunk in every slice."""
        from predictionio_amd.ops import topk as topk_ops
        p = _problem(37, 5000, f, W)
        gv, gi = topk_ops.topk_score(
            p["Xq"].cuda(), p["Y"].cuda(), K, n_slices=7, mode=mode,
            item_cats=p["item_cats"].cuda(),
            query_cats=p["query_cats"].cuda())
        _check(p, K, gv.cpu(), gi.cpu())

    @pytest.mark.parametrize("W", [1, 2, 4])
    @pytest.mark.parametrize("mode,f,K", CASES)
    def test_query_blocks(self, mode, f, K, W):
        """B=130, default slices: three query blocks, the last partial."""
        from predictionio_amd.ops import topk as topk_ops
        p = _problem(130, 5000, f, W)
        gv, gi = topk_ops.topk_score(
            p["Xq"].cuda(), p["Y"].cuda(), K, mode=mode,
            item_cats=p["item_cats"].cuda(),
            query_cats=p["query_cats"].cuda())
        _check(p, K, gv.cpu(), gi.cpu())

    @pytest.mark.parametrize("mode", ["fp32", "mfma"])
    def test_with_mask_and_bans(self, mode):
        """cats + item_mask (30% banned) + 20 bans per query compose: an
        item must pass all three."""
        from predictionio_amd.ops import topk as topk_ops
        B, N, f, K, W = 16, 3000, 64, 10, 2
        p = _problem(B, N, f, W)
        g = torch.Generator().manual_seed(77)
        mask = (torch.rand(N, generator=g) < 0.3).to(torch.uint8)
        bans = [torch.randperm(N, generator=g)[:20].sort().values
                for _ in range(B)]
        indptr = torch.arange(0, 20 * B + 1, 20, dtype=torch.int64)
        indices = torch.cat(bans).to(torch.int32)
        rv, _ = topk_ops.topk_score_ref(
            p["Xq"], p["Y"], K, mask, indptr, indices,
            item_cats=p["item_cats"], query_cats=p["query_cats"])
        gv, gi = topk_ops.topk_score(
            p["Xq"].cuda(), p["Y"].cuda(), K, item_mask=mask.cuda(),
            ban_indptr=indptr.cuda(), ban_indices=indices.cuda(), mode=mode,
            item_cats=p["item_cats"].cuda(),
            query_cats=p["query_cats"].cuda())
        gv, gi = gv.cpu(), gi.cpu()
        assert torch.allclose(gv, rv, atol=1e-4, rtol=1e-4)
        for b in range(B):
            got = gi[b][gi[b] >= 0]
            assert p["hit"][b][got].all()
            assert not mask[got].any()
            assert not set(got.tolist()) & set(bans[b].tolist())
        assert (gi[0] == -1).all()                     # zero-word query
        assert (gi[2] >= 0).all()

    def test_large_k(self):
        """K=100 takes the materialized device fallback, with cats."""
        from predictionio_amd.ops import topk as topk_ops
        p = _problem(37, 5000, 64, 2)
        gv, gi = topk_ops.topk_score(
            p["Xq"].cuda(), p["Y"].cuda(), 100,
            item_cats=p["item_cats"].cuda(),
            query_cats=p["query_cats"].cuda())
        _check(p, 100, gv.cpu(), gi.cpu())

    @pytest.mark.parametrize("mode", ["fp32", "mfma"])
    def test_any_only_equals_unfiltered(self, mode):
        from predictionio_amd.ops import topk as topk_ops
        p = _problem(37, 5000, 64, 2)
        any_only = torch.zeros((37, 2), dtype=torch.int32)
        any_only[:, 0] = 1
        Xq, Y = p["Xq"].cuda(), p["Y"].cuda()
        fv, fi = topk_ops.topk_score(
            Xq, Y, 20, n_slices=7, mode=mode,
            item_cats=p["item_cats"].cuda(), query_cats=any_only.cuda())
        uv, ui = topk_ops.topk_score(Xq, Y, 20, n_slices=7, mode=mode)
        assert torch.equal(fi, ui)
        assert torch.equal(fv, uv)

    def test_contract_violations_raise(self):
        from predictionio_amd.ops import hip_ext
        p = _problem(37, 5000, 64, 2)
        Xq = p["Xq"].cuda().to(torch.bfloat16)
        Y = p["Y"].cuda().to(torch.bfloat16)
        ic, qc = p["item_cats"].cuda(), p["query_cats"].cuda()
        ext = hip_ext()
        with pytest.raises(RuntimeError):
            ext.topk_score_mfma(Xq, Y, 20, 7, item_cats=ic)
        with pytest.raises(RuntimeError):
            ext.topk_score_mfma(Xq, Y, 20, 7, item_cats=ic[:4999],
                                query_cats=qc)
        with pytest.raises(RuntimeError):
            ext.topk_score_mfma(Xq, Y, 20, 7, item_cats=ic.long(),
                                query_cats=qc)
        with pytest.raises(RuntimeError):
            ext.topk_score_mfma(Xq, Y, 20, 7, item_cats=ic,
                                query_cats=qc[:, :1].contiguous())
        with pytest.raises(RuntimeError):
            ext.topk_score_mfma(Xq, Y, 20, 7, item_cats=ic.t(),
                                query_cats=qc)
        prof = torch.zeros(5, dtype=torch.uint64, device="cuda")
        with pytest.raises(RuntimeError):
            ext.topk_score_mfma(Xq, Y, 20, 7, prof=prof, item_cats=ic,
                                query_cats=qc)


@requires_gpu
class TestECommBatchOnDevice:
    def test_batch_predict_matches_predict(self, mem_storage):
        from predictionio_amd.controller import EngineParams, Params
        from predictionio_amd.data.events import DataMap, Event, utcnow
        from predictionio_amd.data.storage.base import App
        from predictionio_amd.templates.ecommercerecommendation import (
            ECommAlgorithm, ECommerceRecommendationEngine, Query,
        )
        n_users, n_items, n_cats = 200, 300, 6
        app_id = mem_storage.get_meta_data_apps().insert(
            App(id=0, name="MyTestApp"))
        levents = mem_storage.get_l_events()
        levents.init(app_id)

        def insert(event, uid, iid=None, props=None, entity_type="user"):
            levents.insert(Event(
                event=event, entity_type=entity_type, entity_id=uid,
                target_entity_type="item" if iid else None,
                target_entity_id=iid, properties=DataMap(props or {}),
                event_time=utcnow()), app_id)

        rng = random.Random(9)
        for i in range(n_items):
            insert("$set", f"i{i}", None,
                   {"categories": [f"c{i % n_cats}"]}, entity_type="item")
        for u in range(n_users):
            liked = [i for i in range(n_items) if i % 4 == u % 4]
            for i in rng.sample(liked, 6) + rng.sample(range(n_items), 2):
                insert("view", f"u{u}", f"i{i}")
            if u % 3 == 0:
                insert("buy", f"u{u}", f"i{rng.randrange(20)}")
        ep = EngineParams(
            data_source_params=Params({"appName": "MyTestApp"}),
            algorithms_params=[("ecomm", Params(
                {"appName": "MyTestApp", "unseenOnly": True,
                 "seenEvents": ["buy", "view"], "similarEvents": ["view"],
                 "rank": 16, "numIterations": 5, "seed": 3}))])
        model = ECommerceRecommendationEngine.apply().train(ep)[0]
        assert model.item_factors.is_cuda
        for i in (5, 9, 21):
            insert("view", "late_user", f"i{i}")
        insert("$set", "unavailableItems", None,
               {"items": [f"i{i}" for i in range(0, n_items, 17)]},
               entity_type="constraint")
        algo = ECommAlgorithm(ep.algorithms_params[0][1])
        qs = [Query(user=f"u{u}", num=5 + u % 6,
                    categories=([f"c{u % n_cats}"] if u % 3 else None),
                    black_list=([f"i{u}", f"i{u + 1}"] if u % 4 == 0
                                else None))
              for u in range(0, n_users, 5)]
        qs += [Query(user="late_user", num=6),
               Query(user="late_user", num=4, categories=["c2", "c3"]),
               Query(user="ghost", num=3),
               Query(user="u1", num=5, categories=["unknown"]),
               Query(user="u2", num=5, white_list=["i1", "i2", "i30"])]
        qs = list(enumerate(qs))
        single = [(i, algo.predict(model, q)) for i, q in qs]
        batched = algo.batch_predict(model, qs)
        assert [i for i, _ in batched] == [i for i, _ in single]
        for (i, rb), (_, rs) in zip(batched, single):
            assert [s.item for s in rb.item_scores] == \
                [s.item for s in rs.item_scores], f"query {i}"
            for a, b in zip(rb.item_scores, rs.item_scores):
                assert abs(a.score - b.score) <= 1e-4, f"query {i}"
        assert sum(len(r.item_scores) for _, r in single) > 100
