"""GPU numerics tests: HIP kernels vs the plain-torch fp32 references.

Run on an MI355X via gpurun: python -m pytest tests -m gpu -x -q
"""

import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")


@requires_gpu
class TestALSKernel:
    @pytest.mark.parametrize("f", [16, 32, 64, 128])
    @pytest.mark.parametrize("implicit", [False, True])
    def test_matches_reference(self, f, implicit):
        from predictionio_amd.ops import als as als_ops
        g = torch.Generator().manual_seed(42 + f)
        n_rows, n_cols = 300, 200
        nnz = 3000
        rows = torch.randint(0, n_rows, (nnz,), generator=g,
                             dtype=torch.int32)
        cols = torch.randint(0, n_cols, (nnz,), generator=g,
                             dtype=torch.int32)
        vals = (torch.rand(nnz, generator=g) * 4 + 1).float()
        rows, cols, vals = als_ops.aggregate_ratings(rows, cols, vals,
                                                     n_cols, "sum")
        Y = (torch.randn((n_cols, f), generator=g) / math.sqrt(f)).float()
        indptr, indices, values = als_ops.build_csr(rows, cols, vals, n_rows)
        lam, alpha = 0.05, 2.0
        X_ref = als_ops.als_solve_ref(
            indptr, indices, values, Y, lam=lam, alpha=alpha,
            implicit=implicit,
            YtY=als_ops.gramian(Y) if implicit else None)
        X_gpu = als_ops.als_solve(
            indptr.cuda(), indices.cuda(), values.cuda(), Y.cuda(),
            lam=lam, alpha=alpha, implicit=implicit).cpu()
        assert torch.allclose(X_gpu, X_ref, atol=2e-3, rtol=2e-3), \
            f"max abs diff {(X_gpu - X_ref).abs().max().item()}"

    def test_empty_rows(self):
        from predictionio_amd.ops import als as als_ops
        f = 64
        Y = torch.randn((50, f)).float()
        # rows 0 and 2 empty
        indptr = torch.tensor([0, 0, 3, 3], dtype=torch.int64)
        indices = torch.tensor([1, 2, 3], dtype=torch.int32)
        values = torch.ones(3)
        X = als_ops.als_solve(indptr.cuda(), indices.cuda(), values.cuda(),
                              Y.cuda(), lam=0.1).cpu()
        X_ref = als_ops.als_solve_ref(indptr, indices, values, Y, lam=0.1)
        assert torch.allclose(X, X_ref, atol=2e-3, rtol=2e-3)
        assert X[0].abs().max().item() == 0.0

    @pytest.mark.parametrize("f", [16, 32, 64, 128])
    @pytest.mark.parametrize("implicit", [False, True])
    def test_woodbury_seam(self, implicit, f):
        """Rows straddling WOODBURY_MAX_NNZ=32: small rows take the Woodbury
        path, large rows the dense-Gramian path — both must match the
        reference and the skip logic must leave no row unwritten."""
        from predictionio_amd.ops import als as als_ops
        g = torch.Generator().manual_seed(99)
        n_cols = 400
        # hits every solver variant boundary: NW=20 (<=20), NW=24
        # (21..24), NW=32 (25..32), dense (>32), empty
        sizes = [0, 1, 5, 20, 21, 24, 25, 28, 29, 31, 32, 33, 40, 64,
                 100, 2, 23, 32, 33, 0, 7]
        rows, cols, vals = [], [], []
        for r, n in enumerate(sizes):
            rows += [r] * n
            cols.append(torch.randint(0, n_cols, (n,), generator=g))
            vals.append(torch.rand(n, generator=g) * 3 + 0.5)
        indptr = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)),
                              dtype=torch.int64)
        cols = torch.cat(cols).to(torch.int32)
        vals = torch.cat(vals).float()
        Y = (torch.randn((n_cols, f), generator=g) / math.sqrt(f)).float()
        YtY = als_ops.gramian(Y) if implicit else None
        X_ref = als_ops.als_solve_ref(indptr, cols, vals, Y, YtY=YtY,
                                      lam=0.05, alpha=2.0, implicit=implicit)
        X = als_ops.als_solve(indptr.cuda(), cols.cuda(), vals.cuda(),
                              Y.cuda(), lam=0.05, alpha=2.0,
                              implicit=implicit).cpu()
        assert torch.allclose(X, X_ref, atol=3e-3, rtol=3e-3), \
            f"max abs diff {(X - X_ref).abs().max().item()}"

    def test_oob_column_id_raises(self):
        """Out-of-range CSR column ids must raise instead of letting the
        kernel gather OOB (which can wedge the device)."""
        from predictionio_amd.ops import als as als_ops
        Y = torch.randn((10, 64)).float().cuda()
        indptr = torch.tensor([0, 2], dtype=torch.int64).cuda()
        indices = torch.tensor([1, 10], dtype=torch.int32).cuda()  # 10 OOB
        values = torch.ones(2).cuda()
        with pytest.raises(ValueError, match="out of range"):
            als_ops.als_solve(indptr, indices, values, Y, lam=0.1)

    def test_large_row(self):
        """A row with nnz >> chunk size exercises the staging loop."""
        from predictionio_amd.ops import als as als_ops
        g = torch.Generator().manual_seed(7)
        f, n_cols, nnz = 64, 500, 2000
        cols = torch.randperm(n_cols, generator=g)[:450].repeat(5)[:nnz]
        cols = cols.to(torch.int32)
        vals = torch.rand(nnz, generator=g).float()
        indptr = torch.tensor([0, nnz], dtype=torch.int64)
        Y = (torch.randn((n_cols, f), generator=g) / math.sqrt(f)).float()
        X_ref = als_ops.als_solve_ref(indptr, cols, vals, Y, lam=0.1)
        X = als_ops.als_solve(indptr.cuda(), cols.cuda(), vals.cuda(),
                              Y.cuda(), lam=0.1).cpu()
        assert torch.allclose(X, X_ref, atol=5e-3, rtol=5e-3)


@requires_gpu
class TestTopKKernel:
    @pytest.mark.parametrize("mode", ["fp32", "mfma"])
    @pytest.mark.parametrize("f", [32, 64])
    @pytest.mark.parametrize("K", [1, 4, 20])
    def test_matches_reference(self, f, K, mode):
        from predictionio_amd.ops import topk as topk_ops
        g = torch.Generator().manual_seed(f * 100 + K)
        B, N = 37, 5000
        Xq = torch.randn((B, f), generator=g).float()
        Y = torch.randn((N, f), generator=g).float()
        rv, ri = topk_ops.topk_score_ref(Xq, Y, K)
        gv, gi = topk_ops.topk_score(Xq.cuda(), Y.cuda(), K, n_slices=7,
                                     mode=mode)
        gv, gi = gv.cpu(), gi.cpu()
        assert torch.allclose(gv, rv, atol=1e-4, rtol=1e-4), \
            f"max val diff {(gv - rv).abs().max()}"
        # indices may differ on exact ties; verify scores of chosen indices
        chosen = (Xq @ Y.t()).gather(1, gi.clamp_min(0))
        assert torch.allclose(chosen, rv, atol=1e-4, rtol=1e-4)

    @pytest.mark.parametrize("mode", ["fp32", "mfma"])
    def test_masks(self, mode):
        from predictionio_amd.ops import topk as topk_ops
        g = torch.Generator().manual_seed(5)
        B, N, f, K = 16, 3000, 64, 10
        Xq = torch.randn((B, f), generator=g).float()
        Y = torch.randn((N, f), generator=g).float()
        mask = (torch.rand(N, generator=g) < 0.3).to(torch.uint8)
        # per-user bans: random sorted lists
        bans = [torch.randint(0, N, (20,), generator=g).unique().sort()[0]
                for _ in range(B)]
        bi = torch.tensor([0] + [len(b) for b in bans]).cumsum(0)
        bx = torch.cat(bans).to(torch.int32)
        rv, ri = topk_ops.topk_score_ref(Xq, Y, K, item_mask=mask,
                                         ban_indptr=bi, ban_indices=bx)
        gv, gi = topk_ops.topk_score(Xq.cuda(), Y.cuda(), K,
                                     item_mask=mask.cuda(),
                                     ban_indptr=bi.cuda(),
                                     ban_indices=bx.cuda(), n_slices=5,
                                     mode=mode)
        gv, gi = gv.cpu(), gi.cpu()
        assert torch.allclose(gv, rv, atol=1e-4, rtol=1e-4)
        # no banned index may appear
        for b in range(B):
            banned = set(bans[b].tolist()) | set(
                torch.nonzero(mask).flatten().tolist())
            assert not (set(gi[b].tolist()) - {-1}) & banned

    @pytest.mark.parametrize("f", [32, 64, 128])
    def test_mfma_matches_fp32_reference(self, f):
        """MFMA path (bf16 score + fp32 rescore) vs the fp32 torch
        reference: top-K values must match exactly-ish (returned values
        ARE fp32 dots of the chosen items) and recall must be ~perfect
        on random data — the 2x candidate margin covers bf16 rounding."""
        from predictionio_amd.ops import topk as topk_ops
        g = torch.Generator().manual_seed(f)
        B, N, K = 130, 20000, 20
        Xq = torch.randn((B, f), generator=g).float()
        Y = torch.randn((N, f), generator=g).float()
        rv, ri = topk_ops.topk_score_ref(Xq, Y, K)
        gv, gi = topk_ops.topk_score(Xq.cuda(), Y.cuda(), K, mode="mfma")
        gv, gi = gv.cpu(), gi.cpu()
        # recall@K vs the fp32 reference
        hits = sum(len(set(gi[b].tolist()) & set(ri[b].tolist()))
                   for b in range(B))
        recall = hits / (B * K)
        assert recall >= 0.999, f"recall {recall}"
        # returned values are exact fp32 scores of the returned items
        chosen = (Xq @ Y.t()).gather(1, gi.clamp_min(0))
        assert torch.allclose(gv, chosen, atol=1e-5, rtol=1e-5)
        # and the K-th value can differ from the reference only by a
        # bf16-near-tie at the candidate cut
        assert torch.allclose(gv, rv, atol=5e-3, rtol=5e-3)

    def test_mfma_prof_variant_matches_live(self, monkeypatch):
        """The MFMA PROF=true instantiation must emit bit-identical raw
        candidates to the live one and fill prof[5]. Without the
        cross-slice exchange (PIO_TOPK_GTH=0) every list is owned by one
        wave and filled in program order, so the raw output is
        deterministic. B=70: two query blocks, the second partial;
        N=1000 is no multiple of 64 or of the 3 slices, so every slice
        ends in a tail chunk."""
        from predictionio_amd.ops import hip_ext
        monkeypatch.setenv("PIO_TOPK_GTH", "0")
        g = torch.Generator().manual_seed(29)
        B, N, f, K, ns, nb = 70, 1000, 32, 5, 3, 4
        Xq = torch.randn((B, f), generator=g).bfloat16().cuda()
        Y = torch.randn((N, f), generator=g).bfloat16().cuda()
        mask = (torch.rand(N, generator=g) < 0.2).to(torch.uint8).cuda()
        bi = (torch.arange(B + 1, dtype=torch.int64) * nb).cuda()
        bx = torch.sort(torch.randint(0, N, (B, nb), generator=g,
                                      dtype=torch.int32), dim=1)[0]
        bx = bx.reshape(-1).cuda()
        ext = hip_ext()
        v0, i0 = ext.topk_score_mfma(Xq, Y, K, ns, mask, bi, bx, 0)
        prof = torch.zeros(5, dtype=torch.uint64, device="cuda")
        v1, i1 = ext.topk_score_mfma(Xq, Y, K, ns, mask, bi, bx, 0, prof)
        torch.cuda.synchronize()
        assert torch.equal(v0, v1) and torch.equal(i0, i1)
        p = prof.cpu().tolist()
        assert p[4] == 2 * ns  # one sample per workgroup
        assert all(t > 0 for t in p[:4])  # every phase ticked

    @pytest.mark.parametrize("gth", ["0", "1"])
    def test_mfma_gth_modes_match_fp32(self, gth, monkeypatch):
        """Cross-slice global-threshold exchange (PIO_TOPK_GTH) on AND
        off must both reproduce the fp32 reference: the global cell only
        prunes items already beaten by K better ones somewhere, so the
        merged top-K is unchanged (many slices so pruning actually
        fires)."""
        from predictionio_amd.ops import topk as topk_ops
        monkeypatch.setenv("PIO_TOPK_GTH", gth)
        # the exchange lives in the list kernel; eager calls would
        # otherwise take the union path, which launches without it
        monkeypatch.setenv("PIO_TOPK_UNION", "0")
        g = torch.Generator().manual_seed(11)
        B, N, K, f = 96, 300_000, 20, 64
        Xq = torch.randn((B, f), generator=g).float()
        Y = torch.randn((N, f), generator=g).float()
        rv, ri = topk_ops.topk_score_ref(Xq, Y, K)
        gv, gi = topk_ops.topk_score(Xq.cuda(), Y.cuda(), K, mode="mfma",
                                     n_slices=96)
        gv, gi = gv.cpu(), gi.cpu()
        hits = sum(len(set(gi[b].tolist()) & set(ri[b].tolist()))
                   for b in range(B))
        assert hits / (B * K) >= 0.999
        chosen = (Xq @ Y.t()).gather(1, gi.clamp_min(0))
        assert torch.allclose(gv, chosen, atol=1e-5, rtol=1e-5)

    @pytest.mark.parametrize("bloom", ["0", "1"])
    def test_mfma_ban_bloom_modes(self, bloom, monkeypatch):
        """Ban handling with the bloom pre-test on AND off: no banned
        item may ever be served, and recall vs the fp32 reference stays
        perfect (the bloom only SKIPS searches for items provably not
        in the list)."""
        from predictionio_amd.ops import topk as topk_ops
        monkeypatch.setenv("PIO_TOPK_BLOOM", bloom)
        g = torch.Generator().manual_seed(23)
        B, N, K, f, nb = 128, 200_000, 20, 64, 30
        Xq = torch.randn((B, f), generator=g).float()
        Y = torch.randn((N, f), generator=g).float()
        bi = torch.arange(B + 1, dtype=torch.int64) * nb
        bxl = torch.randint(0, N, (B * nb,), generator=g,
                            dtype=torch.int32)
        bx = torch.sort(bxl.view(B, nb), dim=1)[0].reshape(-1)
        rv, ri = topk_ops.topk_score_ref(Xq, Y, K, ban_indptr=bi,
                                         ban_indices=bx)
        gv, gi = topk_ops.topk_score(Xq.cuda(), Y.cuda(), K, mode="mfma",
                                     ban_indptr=bi.cuda(),
                                     ban_indices=bx.cuda())
        gi = gi.cpu()
        for b in range(B):
            assert not (set(gi[b].tolist())
                        & set(bx.view(B, nb)[b].tolist())), \
                f"banned item served at row {b} (bloom={bloom})"
        hits = sum(len(set(gi[b].tolist()) & set(ri[b].tolist()))
                   for b in range(B))
        assert hits / (B * K) >= 0.999

    def test_mfma_more_k_than_items(self):
        from predictionio_amd.ops import topk as topk_ops
        Xq = torch.randn((3, 64)).float().cuda()
        Y = torch.randn((10, 64)).float().cuda()
        gv, gi = topk_ops.topk_score(Xq, Y, 20, n_slices=2, mode="mfma")
        assert gi.shape == (3, 20)
        assert (gi[:, 10:] == -1).all()
        assert (gv[:, 10:] == float("-inf")).all()

    def test_small_k_full_block(self):
        """K small enough that ys+lists < the 17.4 KB query-staging pass,
        with B=64 filling the user block: high lanes' staged queries used
        to land beyond the dynamic LDS allocation (OOB ds_writes are
        dropped, the transpose read zeros) — the launcher now floors the
        allocation at the staging footprint."""
        from predictionio_amd.ops import topk as topk_ops
        g = torch.Generator().manual_seed(23)
        B, N, f = 64, 3000, 64
        Xq = torch.randn((B, f), generator=g).float()
        Y = torch.randn((N, f), generator=g).float()
        for K in (1, 4, 8):
            rv, ri = topk_ops.topk_score_ref(Xq, Y, K)
            gv, gi = topk_ops.topk_score(Xq.cuda(), Y.cuda(), K,
                                         n_slices=5)
            gv, gi = gv.cpu(), gi.cpu()
            assert torch.allclose(gv, rv, atol=1e-4, rtol=1e-4),                 f"K={K}: max diff {(gv - rv).abs().max()} "                 f"(worst user {int((gv - rv).abs().max(1)[0].argmax())})"

    def test_prof_variant_matches_live(self):
        """The PROF=true instantiation (wall_clock64 phase probe,
        scripts/serve_phase_probe.py) must return the same candidates as
        the live PROF=false path and fill prof[5]."""
        from predictionio_amd.ops import hip_ext
        g = torch.Generator().manual_seed(17)
        B, N, f, K, ns = 16, 4000, 64, 8, 3
        Xq = torch.randn((B, f), generator=g).float().cuda()
        Y = torch.randn((N, f), generator=g).float().cuda()
        ext = hip_ext()
        v0, i0 = ext.topk_score(Xq, Y, K, ns, None, None, None, 0)
        prof = torch.zeros(5, dtype=torch.uint64, device="cuda")
        v1, i1 = ext.topk_score(Xq, Y, K, ns, None, None, None, 0, prof)
        torch.cuda.synchronize()
        assert torch.equal(v0, v1) and torch.equal(i0, i1)
        p = prof.cpu().tolist()
        assert p[4] > 0  # sampled workgroups
        assert p[1] > 0 and p[2] > 0  # stage + score phases ticked

    def test_more_k_than_items(self):
        from predictionio_amd.ops import topk as topk_ops
        Xq = torch.randn((3, 64)).float().cuda()
        Y = torch.randn((10, 64)).float().cuda()
        gv, gi = topk_ops.topk_score(Xq, Y, 20, n_slices=2)
        assert gi.shape == (3, 20)
        assert (gi[:, 10:] == -1).all()


@requires_gpu
class TestALSTrainerGPU:
    def test_end_to_end_matches_cpu(self):
        from predictionio_amd.models.als import ALSParams, ALSTrainer
        g = torch.Generator().manual_seed(11)
        n_users, n_items, f = 200, 100, 32
        nnz = 4000
        users = torch.randint(0, n_users, (nnz,), generator=g,
                              dtype=torch.int32)
        items = torch.randint(0, n_items, (nnz,), generator=g,
                              dtype=torch.int32)
        vals = (torch.rand(nnz, generator=g) * 4 + 1).float()
        from predictionio_amd.ops import als as als_ops
        users, items, vals = als_ops.aggregate_ratings(users, items, vals,
                                                       n_items, "sum")
        p = ALSParams(rank=f, iterations=3, lambda_=0.05, seed=9)
        tc = ALSTrainer(p, n_users, n_items, torch.device("cpu"))
        tc.set_ratings(users, items, vals)
        Xc, Yc = tc.fit()
        tg = ALSTrainer(p, n_users, n_items, torch.device("cuda"))
        tg.set_ratings(users, items, vals)
        Xg, Yg = tg.fit()
        assert torch.allclose(Xg.cpu(), Xc, atol=5e-2, rtol=5e-2), \
            f"max diff {(Xg.cpu() - Xc).abs().max()}"


@requires_gpu
class TestTemplatesOnGPU:
    def test_recommendation_template_gpu(self, mem_storage):
        """Template end-to-end on the MI355X: train on synthetic events
        (kernels + storage together), predict through the fused top-K."""
        import random
        from predictionio_amd.data.events import DataMap, Event, utcnow
        from predictionio_amd.data.storage.base import App
        app_id = mem_storage.get_meta_data_apps().insert(
            App(id=0, name="GpuApp"))
        mem_storage.get_l_events().init(app_id)
        rng = random.Random(5)
        le = mem_storage.get_l_events()
        for u in range(50):
            for i in rng.sample(range(30), 8):
                le.insert(Event(
                    event="rate", entity_type="user", entity_id=f"u{u}",
                    target_entity_type="item", target_entity_id=f"i{i}",
                    properties=DataMap({"rating": rng.uniform(1, 5)}),
                    event_time=utcnow()), app_id)
        from predictionio_amd.controller import EngineParams, Params
        from predictionio_amd.templates.recommendation import (
            ALSAlgorithm, Query, RecommendationEngine,
        )
        e = RecommendationEngine.apply()
        ep = EngineParams(
            data_source_params=Params({"appName": "GpuApp"}),
            algorithms_params=[("als", Params(
                {"rank": 16, "numIterations": 5, "seed": 3}))])
        models = e.train(ep)
        assert models[0].user_features.is_cuda  # trained on device
        algo = ALSAlgorithm(ep.algorithms_params[0][1])
        r = algo.predict(models[0], Query(user="u1", num=5))
        assert len(r.item_scores) == 5
        banned = [s.item for s in r.item_scores[:2]]
        r2 = algo.predict(models[0],
                          Query(user="u1", num=5, black_list=banned))
        assert not set(s.item for s in r2.item_scores) & set(banned)

        # batch_predict: one fused launch for several users must agree
        # with per-user predict (the micro-batching server path)
        queries = [(k, Query(user=f"u{k}", num=5)) for k in range(6)]
        batched = dict(algo.batch_predict(models[0], queries))
        for k, q in queries:
            single = algo.predict(models[0], q)
            assert [s.item for s in batched[k].item_scores] ==                 [s.item for s in single.item_scores]


@requires_gpu
class TestGraphedTopK:
    def test_create_close_create(self):
        """Graph lifecycle: close() must fully release the capture so a
        LATER graph can be built (ROCm kept the pool entry referenced
        after reset — allocator use_count assert on the next capture
        into the same pool; close() now retires the shared pool)."""
        from predictionio_amd.ops.graphs import GraphedTopK
        Y = torch.randn((50_000, 64)).float().cuda()
        for _ in range(2):
            gt = GraphedTopK(Y, 10, 4)
            v, i = gt(torch.randn((4, 64), device="cuda"))
            assert i.shape == (4, 10)
            del v, i
            gt.close()
        # concurrent generation, closed together, then a fresh one
        a, b = GraphedTopK(Y, 10, 1), GraphedTopK(Y, 10, 8)
        a(torch.randn((1, 64), device="cuda"))
        b(torch.randn((8, 64), device="cuda"))
        a.close()
        b.close()
        c = GraphedTopK(Y, 10, 2)
        c(torch.randn((2, 64), device="cuda"))
        c.close()

    def test_graph_matches_eager(self):
        """hipGraph-captured serving step equals the eager launch and is
        replayable with new query content."""
        from predictionio_amd.ops import topk as topk_ops
        from predictionio_amd.ops.graphs import GraphedTopK
        g = torch.Generator().manual_seed(21)
        N, f, K, B = 20000, 64, 10, 4
        Y = torch.randn((N, f), generator=g).float().cuda()
        gt = GraphedTopK(Y, K=K, batch=B)
        for trial in range(3):
            Xq = torch.randn((B, f), generator=g).float().cuda()
            gv, gi = gt(Xq)
            ev, ei = topk_ops.topk_score(Xq, Y, K)
            assert torch.allclose(gv, ev, atol=1e-4), \
                f"trial {trial}: {(gv - ev).abs().max()}"
            chosen = (Xq @ Y.t()).gather(1, gi.clamp_min(0))
            assert torch.allclose(chosen, ev, atol=1e-4)


@requires_gpu
class TestEvalOnGPU:
    def test_precision_at_k_eval(self, mem_storage):
        """k-fold Precision@K evaluation with device-batched predictions
        (the reference's eval hot loop, Engine.scala:771-786, with
        batchPredict = one fused top-K launch per fold)."""
        import random
        from predictionio_amd.data.events import DataMap, Event, utcnow
        from predictionio_amd.data.storage.base import App
        app_id = mem_storage.get_meta_data_apps().insert(
            App(id=0, name="EvalApp"))
        le = mem_storage.get_l_events()
        le.init(app_id)
        rng = random.Random(9)
        for u in range(40):
            for i in rng.sample([i for i in range(24)
                                 if i % 2 == u % 2], 6):
                le.insert(Event(
                    event="rate", entity_type="user", entity_id=f"u{u}",
                    target_entity_type="item", target_entity_id=f"i{i}",
                    properties=DataMap({"rating": rng.uniform(3.5, 5)}),
                    event_time=utcnow()), app_id)
        from predictionio_amd.controller import (
            EngineParams, MetricEvaluator, Params,
        )
        from predictionio_amd.templates.recommendation import (
            RecommendationEngine,
        )
        from predictionio_amd.templates.recommendation.evaluation import (
            PrecisionAtK,
        )
        e = RecommendationEngine.apply()
        ep = EngineParams(
            data_source_params=Params({"appName": "EvalApp",
                                       "evalParams": {"kFold": 2,
                                                      "queryNum": 5}}),
            algorithms_params=[("als", Params(
                {"rank": 16, "numIterations": 5, "seed": 2}))])
        res = MetricEvaluator(PrecisionAtK(k=5)).evaluate_base(
            e, e.batch_eval([ep]))
        assert 0.0 <= res.best_score <= 1.0


@requires_gpu
class TestWoodburyOptIns:
    def test_dual_bf16_combo_numerics(self):
        """The opt-in PIO_ALS_DUAL + PIO_ALS_STAGE_BF16 path must stay
        within the bf16-staging numerics bound (study: ~2e-3 relative).
        Runs in a subprocess so the env flags apply from the first
        launch."""
        import subprocess
        import sys
        code = """
import torch, math
from predictionio_amd.ops import als as als_ops
g = torch.Generator().manual_seed(3)
n_rows, n_cols, f = 3000, 1500, 64
nnz = n_rows * 15
indptr = torch.arange(0, nnz + 1, 15, dtype=torch.int64)[: n_rows + 1]
ix = torch.randint(0, n_cols, (nnz,), generator=g, dtype=torch.int32)
vv = torch.ones(nnz)
Y = (torch.randn((n_cols, f), generator=g) / math.sqrt(f)).float()
YtY = als_ops.gramian(Y)
ref = als_ops.als_solve_ref(indptr, ix, vv, Y, YtY, lam=0.01,
                            alpha=40.0, implicit=True)
X = als_ops.als_solve(indptr.cuda(), ix.cuda(), vv.cuda(), Y.cuda(),
                      YtY.cuda(), lam=0.01, alpha=40.0,
                      implicit=True).cpu()
rel = ((X - ref).norm() / ref.norm()).item()
assert rel < 5e-3, rel
print("REL", rel)
"""
        env = dict(os.environ, PIO_ALS_DUAL="1", PIO_ALS_STAGE_BF16="1")
        r = subprocess.run([sys.executable, "-c", code], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "REL" in r.stdout


@requires_gpu
class TestRCCLBackend:
    def test_collectives_and_trainer_on_rccl(self):
        """Every distributed call-site shape on the REAL nccl(=RCCL)
        backend (zero RCCL-executed coverage): runs
        scripts/rccl_smoke.py under torchrun with world_size = visible
        GPUs (1 on a single-GPU box; N>1 exercises real exchanges)."""
        import subprocess
        import sys
        n = torch.cuda.device_count()
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        r = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run",
             "--nnodes=1", f"--nproc-per-node={n}",
             "--master-addr", "127.0.0.1", "--master-port", "29557",
             os.path.join(repo, "scripts", "rccl_smoke.py")],
            env=env, capture_output=True, text=True, timeout=420,
            cwd=repo)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "RCCL smoke OK" in r.stdout


@requires_gpu
class TestLargeK:
    def test_k_above_kernel_cap_falls_back(self):
        """The reference allows arbitrary `num`; K > 64 takes the
        device torch fallback and must match the CPU reference."""
        from predictionio_amd.ops import topk as topk_ops
        g = torch.Generator().manual_seed(71)
        B, N, f, K = 9, 3000, 64, 100
        Xq = torch.randn((B, f), generator=g).float()
        Y = torch.randn((N, f), generator=g).float()
        mask = (torch.rand(N, generator=g) < 0.2).to(torch.uint8)
        rv, ri = topk_ops.topk_score_ref(Xq, Y, K, item_mask=mask)
        gv, gi = topk_ops.topk_score(Xq.cuda(), Y.cuda(), K,
                                     item_mask=mask.cuda())
        assert torch.allclose(gv.cpu(), rv, atol=1e-4, rtol=1e-4)
        chosen = (Xq @ Y.t()).gather(1, gi.cpu().clamp_min(0))
        ok = rv != float("-inf")
        assert torch.allclose(chosen[ok], rv[ok], atol=1e-4, rtol=1e-4)


@requires_gpu
class TestTemplatesOnDevice:
    def test_cooccurrence_sparse_mm_on_rocm(self):
        """CooccurrenceAlgorithm.train uses torch.sparse.mm(sparse,
        sparse) on the device when available — verify the ROCm build
        supports it and matches a dense reference."""
        g = torch.Generator().manual_seed(9)
        n_u, n_i = 200, 50
        u = torch.randint(0, n_u, (1500,), generator=g)
        i = torch.randint(0, n_i, (1500,), generator=g)
        key = torch.unique(u * n_i + i)
        u, i = key // n_i, key % n_i
        A = torch.sparse_coo_tensor(
            torch.stack([u, i]).cuda(),
            torch.ones(u.numel(), device="cuda"),
            (n_u, n_i)).coalesce()
        C = torch.sparse.mm(A.t(), A).coalesce()
        Ad = torch.zeros(n_u, n_i)
        Ad[u, i] = 1.0
        ref = Ad.t() @ Ad
        dense = torch.zeros(n_i, n_i, device="cuda")
        dense[C.indices()[0], C.indices()[1]] = C.values()
        assert torch.allclose(dense.cpu(), ref, atol=1e-4)

    def test_similarproduct_template_end_to_end_gpu(self):
        """Similarproduct trains + predicts on device (cosine path via
        the MFMA kernel, category masks resident)."""
        from predictionio_amd.controller import Params
        from predictionio_amd.templates.similarproduct import (
            ALSAlgorithm, Query,
        )
        from predictionio_amd.templates.similarproduct.engine import (
            Item, PreparedData,
        )
        g = torch.Generator().manual_seed(4)
        from predictionio_amd.templates.similarproduct.engine import (
            ViewEvent,
        )
        views = []
        for u in range(40):
            for j in range(6):
                views.append(ViewEvent(f"u{u}", f"i{(u + j) % 25}",
                                       float(u * 10 + j)))
        items = {f"i{k}": Item(categories=["odd" if k % 2 else "even"])
                 for k in range(25)}
        pd_ = PreparedData(users={}, items=items, view_events=views)
        algo = ALSAlgorithm(Params({"rank": 16, "numIterations": 5,
                                    "seed": 2}))
        model = algo.train(pd_)
        assert model.item_factors_norm.is_cuda
        r = algo.predict(model, Query(items=["i3"], num=5,
                                      categories=["odd"]))
        assert len(r.item_scores) == 5
        for s in r.item_scores:
            assert int(s.item[1:]) % 2 == 1  # category filter held


@requires_gpu
class TestMfmaGramian:
    def test_dense_rows_on_matrix_cores(self):
        """PIO_ALS_MFMA_GRAMIAN=1 routes nnz>32 rows through the MFMA
        Gramian (bf16 inputs / fp32 accumulate) — numerics within the
        bf16 bound vs the fp32 reference. Subprocess so the env applies
        from the first launch."""
        import subprocess
        import sys
        code = """
import torch, math
from predictionio_amd.ops import als as als_ops
g = torch.Generator().manual_seed(5)
n_rows, n_cols, f, nnz_r = 500, 800, 64, 48
nnz = n_rows * nnz_r
indptr = torch.arange(0, nnz + 1, nnz_r, dtype=torch.int64)[: n_rows + 1]
ix = torch.randint(0, n_cols, (nnz,), generator=g, dtype=torch.int32)
vv = (torch.rand(nnz, generator=g) * 3 + 0.5).float()
Y = (torch.randn((n_cols, f), generator=g) / math.sqrt(f)).float()
for implicit in (True, False):
    YtY = als_ops.gramian(Y) if implicit else None
    ref = als_ops.als_solve_ref(indptr, ix, vv, Y, YtY, lam=0.05,
                                alpha=2.0, implicit=implicit)
    X = als_ops.als_solve(indptr.cuda(), ix.cuda(), vv.cuda(), Y.cuda(),
                          YtY.cuda() if implicit else None, lam=0.05,
                          alpha=2.0, implicit=implicit).cpu()
    rel = ((X - ref).norm() / ref.norm()).item()
    assert rel < 5e-3, (implicit, rel)
print("GRAMIAN_OK")
"""
        env = dict(os.environ, PIO_ALS_MFMA_GRAMIAN="1")
        r = subprocess.run([sys.executable, "-c", code], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert "GRAMIAN_OK" in r.stdout
