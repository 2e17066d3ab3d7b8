"""GPU tests of the fused top-K union path for 64 < K <= 1024: the MFMA
kernel's interleaved slices (`interleave=True`), `topk_rescore`, and
`topk_score` end to end against the torch reference.

Shapes are the smallest at which the interleave can go wrong: one chunk
per slice, several, none, a partial last chunk, no tail, three query
blocks with a partial last one.

Run on an MI355X: python -m pytest tests/test_topk_union_gpu.py -m gpu -q
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

FMIN = torch.finfo(torch.float32).min


def _ext():
    from predictionio_amd.ops import hip_ext
    return hip_ext()


def _flagged():
    from predictionio_amd.ops import topk as topk_ops
    return topk_ops.union_stats()["flagged"]


# ---------------------------------------------------------------- coverage

_int_problems = {}


def _int_problem(B, N, f):
    """Small-integer operands in [-4, 4]: exact in bf16, and every partial
    sum of the dot (|.| <= 16 f) is exact in fp32, so kernel scores equal
    the integer dots bit for bit. Built once per shape, never modified."""
    key = (B, N, f)
    if key not in _int_problems:
        g = torch.Generator().manual_seed(100 + N + f)
        Xq = torch.randint(-4, 5, (B, f), generator=g).float()
        Y = torch.randint(-4, 5, (N, f), generator=g).float()
        _int_problems[key] = (Xq, Y, Xq @ Y.t())
    return _int_problems[key]


def _launch_ilv(Xq, Y, L, S):
    vals, idxs = _ext().topk_score_mfma(
        Xq.cuda().to(torch.bfloat16), Y.cuda().to(torch.bfloat16), L, S,
        interleave=True, gth=False)
    torch.cuda.synchronize()
    B = Xq.shape[0]
    assert vals.shape == (B, S * L) and idxs.shape == (B, S * L)
    return vals.cpu().view(B, S, L), idxs.cpu().view(B, S, L).long()


@requires_gpu
class TestInterleavedCoverage:
    B = 130   # three query blocks, the last one partial

    @pytest.mark.parametrize("f", [32, 64, 128])
    def test_one_chunk_per_slice_partial_tail(self, f):
        """N=1000, 16 slices: every item is in exactly one list."""
        Xq, Y, dots = _int_problem(self.B, 1000, f)
        vals, idxs = _launch_ilv(Xq, Y, 64, 16)
        for b in range(self.B):
            ok = idxs[b] >= 0
            assert sorted(idxs[b][ok].tolist()) == list(range(1000))
            assert torch.equal(vals[b][ok], dots[b][idxs[b][ok]])
            assert (vals[b][~ok] == FMIN).all()
        # slice s holds chunk s and nothing else
        ok = idxs >= 0
        s_of = torch.arange(16).view(1, 16, 1).expand_as(idxs)
        assert torch.equal((idxs // 64)[ok], s_of[ok])

    @pytest.mark.parametrize("f", [32, 64, 128])
    @pytest.mark.parametrize("N,S", [(1000, 5), (64 * 7, 7)])
    def test_slice_groups_match_membership(self, f, N, S):
        """Several chunks per slice with a partial tail (1000, 5); no
        tail at all (448, 7). Each group = top 64 of its membership."""
        Xq, Y, dots = _int_problem(self.B, N, f)
        vals, idxs = _launch_ilv(Xq, Y, 64, S)
        chunk = torch.arange(N) // 64
        for s in range(S):
            members = (chunk % S == s).nonzero().flatten()
            k = min(64, members.numel())
            want = torch.topk(dots[:, members], k, dim=1).values
            got = torch.sort(vals[:, s], dim=1, descending=True).values
            assert torch.equal(got[:, :k], want), f"slice {s}"
            assert (got[:, k:] == FMIN).all()
            gi = idxs[:, s]
            ok = gi >= 0
            assert torch.equal(ok.sum(dim=1), torch.full((self.B,), k))
            assert ((gi // 64) % S == s)[ok].all()
            assert torch.equal(vals[:, s][ok],
                               dots.gather(1, gi.clamp_min(0))[ok])
            for b in (0, 64, self.B - 1):
                assert len(set(gi[b][ok[b]].tolist())) == k

    @pytest.mark.parametrize("f", [32, 64, 128])
    def test_slices_without_a_chunk_write_empty_groups(self, f):
        """N=100, 4 slices: two chunks, so slices 2 and 3 own nothing."""
        Xq, Y, dots = _int_problem(self.B, 100, f)
        vals, idxs = _launch_ilv(Xq, Y, 64, 4)
        assert (idxs[:, 2:] == -1).all() and (vals[:, 2:] == FMIN).all()
        for b in range(self.B):
            for s, lo, hi in ((0, 0, 64), (1, 64, 100)):
                ok = idxs[b, s] >= 0
                assert sorted(idxs[b, s][ok].tolist()) == list(range(lo, hi))
                assert torch.equal(vals[b, s][ok], dots[b][idxs[b, s][ok]])

    def test_prof_with_interleave_raises(self):
        Xq, Y, _ = _int_problem(self.B, 100, 64)
        prof = torch.zeros(5, dtype=torch.uint64, device="cuda")
        with pytest.raises(RuntimeError):
            _ext().topk_score_mfma(
                Xq.cuda().to(torch.bfloat16), Y.cuda().to(torch.bfloat16),
                20, 2, prof=prof, interleave=True)


# -------------------------------------------------------------- end to end

_problems = {}


def _problem(B, N, f):
    """Seeded inputs, CPU scores and per-K references, built once per
    shape and shared unchanged."""
    key = (B, N, f)
    if key not in _problems:
        g = torch.Generator().manual_seed(7 * B + N + f)
        Xq = torch.randn((B, f), generator=g).float()
        Y = torch.randn((N, f), generator=g).float()
        _problems[key] = dict(Xq=Xq, Y=Y, scores=Xq @ Y.t(), refs={})
    return _problems[key]


def _check_e2e(p, K, gv, gi, rv=None):
    from predictionio_amd.ops import topk as topk_ops
    if rv is None:
        if K not in p["refs"]:
            p["refs"][K] = topk_ops.topk_score_ref(p["Xq"], p["Y"], K)
        rv = p["refs"][K][0]
    gv, gi = gv.cpu(), gi.cpu()
    assert gi.dtype == torch.int64 and gv.shape == rv.shape == gi.shape
    assert torch.allclose(gv, rv, atol=1e-4, rtol=1e-4), \
        f"max val diff {(gv - rv)[torch.isfinite(rv)].abs().max()}"
    valid = gi >= 0
    assert torch.equal(valid, torch.isfinite(rv))
    chosen = p["scores"].gather(1, gi.clamp_min(0))
    assert torch.allclose(gv[valid], chosen[valid], atol=1e-5, rtol=1e-5), \
        f"max |value - dot| {(gv[valid] - chosen[valid]).abs().max()}"
    for b in range(gi.shape[0]):
        got = gi[b][valid[b]].tolist()
        assert len(set(got)) == len(got)


E2E_CASES = [
    # B, N, f, K, list_k, n_slices
    (37, 5000, 64, 100, 40, 20),
    (130, 5000, 64, 65, 32, 20),
    (64, 20000, 64, 256, 64, 40),
    (37, 5000, 32, 100, 40, 20),
    (37, 5000, 128, 100, 40, 20),
    (37, 5000, 10, 100, None, None),    # unpadded rank, the default plan
]


@requires_gpu
class TestUnionEndToEnd:
    @pytest.mark.parametrize("B,N,f,K,list_k,n_slices", E2E_CASES)
    def test_matches_reference_unflagged(self, B, N, f, K, list_k, n_slices):
        """No query may be flagged here (the most top-2K items any slice
        holds on these shapes is far below list_k): a flagged query is
        answered by the fallback and would hide a kernel bug."""
        from predictionio_amd.ops import topk as topk_ops
        p = _problem(B, N, f)
        before = topk_ops.union_stats()
        gv, gi = topk_ops.topk_score(p["Xq"].cuda(), p["Y"].cuda(), K,
                                     n_slices=n_slices, list_k=list_k)
        after = topk_ops.union_stats()
        assert after["calls"] == before["calls"] + 1
        assert after["queries"] == before["queries"] + B
        assert after["flagged"] == before["flagged"]
        _check_e2e(p, K, gv, gi)

    def test_filters_compose(self):
        """item_mask (30%), 20 bans per query and a W=2 category filter
        at K=100, with zero-word queries and a 7-member rare category."""
        from predictionio_amd.ops import topk as topk_ops
        B, N, f, K, W = 37, 5000, 64, 100, 2
        p = _problem(B, N, f)
        g = torch.Generator().manual_seed(77)
        rng = np.random.default_rng(77)
        mask = (torch.rand(N, generator=g) < 0.3).to(torch.uint8)
        bans = [torch.randperm(N, generator=g)[:20].sort().values
                for _ in range(B)]
        indptr = torch.arange(0, 20 * B + 1, 20, dtype=torch.int64)
        indices = torch.cat(bans).to(torch.int32)
        # bit 0 = ANY; category c owns bit c + 1; category 0 is rare
        ncat = 32 * W - 1
        rare = [0, 1, 63, 64, 1279, N - 2, N - 1]
        words = np.zeros((N, W), dtype=np.uint32)
        words[:, 0] |= 1
        for c in (rng.integers(1, ncat, N), rng.integers(1, ncat, N)):
            bit = c + 1
            words[np.arange(N), bit >> 5] |= (
                np.uint32(1) << (bit & 31).astype(np.uint32))
        words[rare, 0] |= np.uint32(2)
        mask[rare] = 0
        qwords = np.zeros((B, W), dtype=np.uint32)
        for b in range(B):
            if b % 11 == 0:
                continue                       # zero words: nothing passes
            if b % 5 == 0:
                qwords[b, 0] = 1               # ANY only: no filter
            elif b == 1:
                qwords[b, 0] = 2               # the rare category
            else:
                bit = b % (ncat - 1) + 2
                qwords[b, bit >> 5] = np.uint32(1) << np.uint32(bit & 31)
        item_cats = torch.from_numpy(words.view(np.int32))
        query_cats = torch.from_numpy(qwords.view(np.int32))
        rv, _ = topk_ops.topk_score_ref(
            p["Xq"], p["Y"], K, mask, indptr, indices,
            item_cats=item_cats, query_cats=query_cats)
        calls = topk_ops.union_stats()["calls"]
        gv, gi = topk_ops.topk_score(
            p["Xq"].cuda(), p["Y"].cuda(), K, item_mask=mask.cuda(),
            ban_indptr=indptr.cuda(), ban_indices=indices.cuda(),
            item_cats=item_cats.cuda(), query_cats=query_cats.cuda())
        assert topk_ops.union_stats()["calls"] == calls + 1
        _check_e2e(p, K, gv, gi, rv)
        gi = gi.cpu()
        hit = torch.zeros((B, N), dtype=torch.bool)
        for w in range(W):
            hit |= (item_cats[:, w].unsqueeze(0)
                    & query_cats[:, w].unsqueeze(1)) != 0
        for b in range(B):
            got = gi[b][gi[b] >= 0]
            assert hit[b][got].all()
            assert not mask[got].any()
            assert not set(got.tolist()) & set(bans[b].tolist())
        assert (gi[0] == -1).all()                      # zero-word query
        want1 = sorted(set(rare) - set(bans[1].tolist()))
        assert sorted(gi[1][gi[1] >= 0].tolist()) == want1
        assert (gi[5] >= 0).all()                       # ANY only

    def test_flagged_queries_are_recomputed(self):
        """Query 0's best items all sit in chunks = 0 mod S, i.e. in one
        slice: it must be flagged, and still come back right."""
        from predictionio_amd.ops import topk as topk_ops
        B, N, f, K, L, S = 37, 5000, 64, 100, 32, 20
        p = _problem(B, N, f)
        g = torch.Generator().manual_seed(5)
        Y = p["Y"].clone()
        hot = ((torch.arange(N) // 64) % S == 0).nonzero().flatten()
        assert hot.numel() > 2 * K
        Y[hot] = p["Xq"][0] * (1.5 + 0.5 * torch.rand((hot.numel(), 1),
                                                      generator=g))
        q = dict(Xq=p["Xq"], Y=Y, scores=p["Xq"] @ Y.t(), refs={})
        before = _flagged()
        gv, gi = topk_ops.topk_score(q["Xq"].cuda(), Y.cuda(), K,
                                     n_slices=S, list_k=L)
        assert _flagged() >= before + 1
        _check_e2e(q, K, gv, gi)
        assert set(gi[0].tolist()) <= set(hot.tolist())

    def test_union_mode_below_the_cutover(self, monkeypatch):
        """mode="union" at K=20 returns the list kernel's items, the
        eager default is the union path too, and all values are the
        fp32 dots: each within the fp32 accumulation bound
        f 2^-23 (|x|.|y|) of the float64 dot."""
        from predictionio_amd.ops import topk as topk_ops
        B, N, f, K = 37, 5000, 64, 20
        p = _problem(B, N, f)
        Xq, Y = p["Xq"].cuda(), p["Y"].cuda()
        calls = topk_ops.union_stats()["calls"]
        uv, ui = topk_ops.topk_score(Xq, Y, K, mode="union")
        assert topk_ops.union_stats()["calls"] == calls + 1
        ev, ei = topk_ops.topk_score(Xq, Y, K)
        assert topk_ops.union_stats()["calls"] == calls + 2
        assert torch.equal(ev, uv) and torch.equal(ei, ui)
        monkeypatch.setenv("PIO_TOPK_UNION", "0")
        dv, di = topk_ops.topk_score(Xq, Y, K)
        assert topk_ops.union_stats()["calls"] == calls + 2
        assert torch.equal(ui.sort(dim=1).values, di.sort(dim=1).values)
        d64 = p["Xq"].double() @ p["Y"].double().t()
        bound = f * 2.0 ** -23 * (p["Xq"].abs().double()
                                  @ p["Y"].abs().double().t())
        for v, i in ((uv, ui), (dv, di)):
            v, i = v.cpu().double(), i.cpu()
            assert ((v - d64.gather(1, i)).abs() <= bound.gather(1, i)).all()

    def test_routing(self, monkeypatch):
        from predictionio_amd.ops import topk as topk_ops
        p = _problem(37, 5000, 64)
        Xq, Y = p["Xq"].cuda(), p["Y"].cuda()
        with pytest.raises(ValueError):
            topk_ops.topk_score(Xq, Y[:100], 100, mode="union")
        calls = topk_ops.union_stats()["calls"]
        # no plan (tiny N), fp32 mode, K > 1024 and the switch: fallback
        gv, gi = topk_ops.topk_score(Xq, Y[:100], 100)
        assert (gi[:, :100] >= 0).all()
        topk_ops.topk_score(Xq, Y, 100, mode="fp32")
        topk_ops.topk_score(Xq, Y, 1025)
        monkeypatch.setenv("PIO_TOPK_UNION", "0")
        gv, gi = topk_ops.topk_score(Xq, Y, 100)
        assert topk_ops.union_stats()["calls"] == calls
        _check_e2e(p, 100, gv, gi)
        monkeypatch.delenv("PIO_TOPK_UNION")
        gv, gi = topk_ops.topk_score(Xq, Y, 1024)
        assert topk_ops.union_stats()["calls"] == calls + 1
        _check_e2e(p, 1024, gv, gi)


# ----------------------------------------------------------------- rescore

@requires_gpu
class TestTopkRescore:
    def test_exact_on_integers_and_empty_slots(self):
        B, N, f, C = 37, 1000, 64, 200
        Xq, Y, dots = _int_problem(130, N, f)
        Xq, dots = Xq[:B], dots[:B]
        g = torch.Generator().manual_seed(3)
        idx = torch.randint(0, N, (B, C), generator=g, dtype=torch.int32)
        idx[:, ::7] = -1
        idx[3] = -1
        out = _ext().topk_rescore(Xq.cuda(), Y.cuda(), idx.cuda()).cpu()
        ok = idx >= 0
        assert torch.equal(out[ok], dots.gather(1, idx.long().clamp_min(0))[ok])
        assert (out[~ok] == float("-inf")).all()

    @pytest.mark.parametrize("f", [10, 16, 64, 128])
    @pytest.mark.parametrize("C", [1, 200])
    @pytest.mark.parametrize("aligned", [True, False])
    def test_error_bound(self, f, C, aligned):
        """|out - ref64| <= f 2^-23 (|x|.|y|): n fp32 roundings of at most
        2^-24 relative each, with a factor two to spare. The unaligned
        view (base pointer 4 B past a 16 B boundary) takes the
        one-float-per-load path; so does f = 10."""
        B, N = 37, 3000
        g = torch.Generator().manual_seed(11 * f + C)
        Xq = torch.randn((B, f), generator=g)
        Y = torch.randn((N, f), generator=g)
        idx = torch.randint(0, N, (B, C), generator=g, dtype=torch.int32)
        if aligned:
            Yd = Y.cuda()
        else:
            buf = torch.empty(N * f + 1, device="cuda")
            Yd = buf[1:].view(N, f)
            Yd.copy_(Y)
            assert Yd.is_contiguous() and Yd.data_ptr() % 16 == 4
        out = _ext().topk_rescore(Xq.cuda(), Yd, idx.cuda()).cpu().double()
        Yg = Y[idx.long()].double()                      # B x C x f
        ref = torch.einsum("bf,bcf->bc", Xq.double(), Yg)
        mag = torch.einsum("bf,bcf->bc", Xq.double().abs(), Yg.abs())
        ratio = ((out - ref).abs() / (f * 2.0 ** -23 * mag)).max().item()
        print(f"rescore f={f} C={C} aligned={aligned}: "
              f"worst error / bound = {ratio:.4f}")
        assert ratio <= 1.0

    def test_contract_violations_raise(self):
        ext = _ext()
        Xq = torch.randn((4, 64), device="cuda")
        Y = torch.randn((100, 64), device="cuda")
        idx = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
        bad = idx.clone()
        bad[2, 3] = 100
        for args in ((Xq, Y, bad),                       # index >= N
                     (Xq, Y, idx.long()),                # dtype
                     (Xq, Y, idx.cpu()),                 # device
                     (Xq, Y, idx.t()),                   # contiguity
                     (Xq, Y, idx[:3]),                   # rows
                     (Xq[:, :32].contiguous(), Y, idx),  # rank mismatch
                     (Xq.double(), Y, idx)):
            with pytest.raises(RuntimeError):
                ext.topk_rescore(*args)
