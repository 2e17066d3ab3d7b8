"""CPU tests of the union path's pure-torch parts (ops/topk.py):
`_union_merge` against a brute-force reference on per-slice lists built
here with the kernel's chunk-interleaved slice membership, and
`_union_plan`'s guarantees. No GPU needed.
"""

import math

import pytest
import torch

from predictionio_amd.ops import topk as topk_ops

FMIN = torch.finfo(torch.float32).min


def _slice_lists(scores, L, S):
    """What the interleaved kernel writes for `scores` [B, N] (-inf =
    filtered): slice s owns the 64-item chunks s, s+S, s+2S, ...; its
    group holds its top L valid scores, empty slots at -FLT_MAX / -1."""
    B, N = scores.shape
    chunk = torch.arange(N) // 64
    vals = torch.full((B, S, L), FMIN)
    idxs = torch.full((B, S, L), -1, dtype=torch.int32)
    for s in range(S):
        members = (chunk % S == s).nonzero().flatten()
        if members.numel() == 0:
            continue
        k = min(L, members.numel())
        v, p = torch.topk(scores[:, members], k, dim=1)
        ok = v > float("-inf")
        vals[:, s, :k] = torch.where(ok, v, torch.tensor(FMIN))
        idxs[:, s, :k] = torch.where(ok, members[p].int(),
                                     torch.tensor(-1, dtype=torch.int32))
    return vals.reshape(B, S * L), idxs.reshape(B, S * L)


def _brute_top(scores, M):
    """Per query: the sorted valid (score, item) top M over all items."""
    out = []
    for row in scores:
        valid = (row > float("-inf")).nonzero().flatten()
        order = valid[torch.argsort(row[valid], descending=True)][:M]
        out.append(order.tolist())
    return out


def _brute_flag(vals, L, S, M):
    """The flag definition, spelled out per query and slice."""
    out = []
    for row in vals:
        valid = row[row > FMIN]
        v_m = (torch.sort(valid, descending=True).values[M - 1].item()
               if valid.numel() >= M else float("-inf"))
        flag = False
        for s in range(S):
            g = row[s * L:(s + 1) * L]
            if (g > FMIN).all() and g.min().item() > v_m:
                flag = True
        out.append(flag)
    return out


def _random_scores(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, N), generator=g)


class TestUnionMerge:
    def test_random_unflagged_and_exact(self):
        B, N, K, L, S = 16, 5000, 100, 40, 20
        M = 2 * K
        scores = _random_scores(B, N, 1)
        vals, idxs = _slice_lists(scores, L, S)
        si, sv, fl = topk_ops._union_merge(vals, idxs, L, S, M)
        assert fl.tolist() == _brute_flag(vals, L, S, M)
        assert not fl.any()
        assert si.shape == (B, M) and si.dtype == torch.int64
        want = _brute_top(scores, M)
        for b in range(B):
            assert si[b].tolist() == want[b]
            assert torch.equal(sv[b], scores[b][si[b]])

    def test_adversarial_layout_flags_query_zero(self):
        B, N, K, L, S = 8, 5000, 100, 32, 20
        M = 2 * K
        scores = _random_scores(B, N, 2)
        # query 0's best items all sit in chunks = 0 mod S (slice 0)
        hot = ((torch.arange(N) // 64) % S == 0).nonzero().flatten()
        assert hot.numel() > M
        scores[0, hot] += 100.0
        vals, idxs = _slice_lists(scores, L, S)
        _, _, fl = topk_ops._union_merge(vals, idxs, L, S, M)
        assert fl.tolist() == _brute_flag(vals, L, S, M)
        assert fl[0]
        assert not fl[1:].any()

    def test_selective_filter_returns_all_passing(self):
        B, N, K, L, S = 6, 5000, 100, 32, 20
        M = 2 * K
        scores = _random_scores(B, N, 3)
        g = torch.Generator().manual_seed(33)
        keep = torch.rand((B, N), generator=g) < 0.03   # ~150 < M pass
        scores = scores.masked_fill(~keep, float("-inf"))
        vals, idxs = _slice_lists(scores, L, S)
        per_slice = (vals.view(B, S, L) > FMIN).sum(dim=2)
        assert (per_slice < L).all() and (keep.sum(dim=1) < M).all()
        si, sv, fl = topk_ops._union_merge(vals, idxs, L, S, M)
        assert not fl.any()
        assert fl.tolist() == _brute_flag(vals, L, S, M)
        for b in range(B):
            got = si[b][si[b] >= 0]
            assert sorted(got.tolist()) == keep[b].nonzero().flatten().tolist()
            n = got.numel()
            assert (si[b][n:] == -1).all()
            assert torch.isinf(sv[b][n:]).all()

    def test_short_with_a_full_list_is_flagged(self):
        B, N, K, L, S = 4, 5000, 100, 32, 20
        M = 2 * K
        scores = _random_scores(B, N, 4)
        chunk = torch.arange(N) // 64
        keep = torch.zeros((B, N), dtype=torch.bool)
        # query 0: 50 passing items, all in slice 3 (> L there, < M in all)
        keep[0, (chunk % S == 3).nonzero().flatten()[:50]] = True
        # query 1: 50 passing items spread one chunk apart: no full list
        keep[1, torch.arange(50) * 64] = True
        keep[2:, ::40] = True
        scores = scores.masked_fill(~keep, float("-inf"))
        vals, idxs = _slice_lists(scores, L, S)
        _, _, fl = topk_ops._union_merge(vals, idxs, L, S, M)
        assert fl.tolist() == _brute_flag(vals, L, S, M)
        assert fl.tolist() == [True, False, False, False]

    def test_ties_at_the_cut_do_not_flag(self):
        """A full list whose minimum EQUALS v_M dropped nothing better."""
        L, S, M = 2, 2, 2
        vals = torch.tensor([[5.0, 3.0, 3.0, FMIN]])
        idxs = torch.tensor([[0, 1, 64, -1]], dtype=torch.int32)
        si, _, fl = topk_ops._union_merge(vals, idxs, L, S, M)
        assert not fl[0]
        assert si[0, 0].item() == 0 and si[0, 1].item() in (1, 64)


class TestUnionPlan:
    @pytest.mark.parametrize("B", [1, 64, 1024, 4096])
    @pytest.mark.parametrize("N", [5000, 100_000, 10_000_000])
    @pytest.mark.parametrize("K", [1, 20, 65, 100, 256, 1024])
    @pytest.mark.parametrize("pf,W", [(32, 0), (64, 0), (128, 4)])
    def test_plan_invariants(self, B, N, K, pf, W):
        plan = topk_ops._union_plan(B, N, pf, K, W)
        if plan is None:
            # only when even L = 64 cannot meet the rule within N/64 slices
            nch = (N + 63) // 64
            assert not topk_ops._union_rule(64, nch, 2 * K)
            return
        L, S = plan
        assert 1 <= L <= 64
        assert 2 <= S <= (N + 63) // 64
        assert S * L >= 2 * K
        mu = 2 * K / S
        assert L >= mu + 6 * math.sqrt(mu)
        # the shortest list that fits: a shorter one would need more
        # slices than there are chunks
        shorter = [l for l in (16, 20, 24, 32, 40, 48, 64) if l < L]
        for l in shorter:
            assert topk_ops._union_min_slices(l, 2 * K) > (N + 63) // 64

    def test_serve_shape_plan(self):
        """K = 100 at the serve shape: the shortest list, with the fewest
        slices that keep P(a list fills) below 1e-6 — more than the 24
        that fill the chip. Small batches keep the chip-filling count."""
        assert topk_ops._union_plan(4096, 10_000_000, 64, 100, 0) == (16, 56)
        assert topk_ops._union_plan(64, 10_000_000, 64, 100, 0) == (16, 1536)
        assert topk_ops._union_plan(4096, 10_000_000, 64, 1024, 0) \
            == (16, 568)

    def test_tiny_n_has_no_plan(self):
        assert topk_ops._union_plan(8, 100, 64, 100, 0) is None
        assert topk_ops._union_plan(8, 60, 64, 5, 0) is None

    def test_pinned_plan(self):
        assert topk_ops._union_plan(37, 5000, 64, 100, 0, 40, 20) == (40, 20)
        # a pinned slice count is clipped to one chunk per slice
        assert topk_ops._union_plan(37, 1000, 64, 20, 0, 64, 40) == (64, 16)
        # too few candidates for the 2K shortlist
        assert topk_ops._union_plan(37, 5000, 64, 100, 0, 16, 4) is None
        with pytest.raises(ValueError):
            topk_ops._union_plan(37, 5000, 64, 100, 0, 65, 20)


class TestRoutingOnCpu:
    def test_cpu_results_unchanged_and_stats_idle(self):
        g = torch.Generator().manual_seed(9)
        Xq = torch.randn((5, 16), generator=g)
        Y = torch.randn((700, 16), generator=g)
        before = topk_ops.union_stats()
        assert set(before) == {"calls", "queries", "flagged"}
        v, i = topk_ops.topk_score(Xq, Y, 100)
        rv, ri = topk_ops.topk_score_ref(Xq, Y, 100)
        assert torch.equal(v, rv) and torch.equal(i, ri)
        assert topk_ops.union_stats() == before
