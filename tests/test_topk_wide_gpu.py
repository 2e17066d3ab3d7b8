"""GPU tests of the wide-rank MFMA top-K (topk_mfma_wide_kernel: factor
ranks 129..512, streamed through LDS in 128-wide panels), reached through
`topk_score` / `cosine_topk` on both routes.

Integer data throughout: factors in {-2..2} (times 1..4 in the panel-order
test), weights in {1, 2, -1}. Every bf16 value and product is exact and
every partial sum is an integer far below 2^24, so the bf16 ranking, the
fp32 re-score and the float64 reference agree exactly and no tolerance is
needed. Ties are frequent, so the assertions are the tie-proof ones: equal
sorted values, distinct valid ids, each id's reference score equal to its
returned value.

Run on an MI355X: python -m pytest tests/test_topk_wide_gpu.py -m gpu -q
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")


@functools.lru_cache(maxsize=None)
def _problem(B, N, f):
    """(Xq, Y) fp32 with entries in {-2..2}; built once per shape and
    never modified."""
    g = torch.Generator().manual_seed(7 * N + f)
    return (torch.randint(-2, 3, (B, f), generator=g).float(),
            torch.randint(-2, 3, (N, f), generator=g).float())


def _filters(B, N, seed):
    """item_mask, ban CSR, W = 2 category words and weights, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(N, generator=g) < 0.2).to(torch.uint8)
    bans = [torch.randperm(N, generator=g)[:(7 * b) % 40].sort().values
            for b in range(B)]
    indptr = torch.tensor([0] + [len(x) for x in bans]).cumsum(0)
    indices = torch.cat(bans).to(torch.int32)
    ic = torch.randint(0, 4, (N, 2), generator=g, dtype=torch.int32)
    qc = torch.randint(0, 4, (B, 2), generator=g, dtype=torch.int32)
    w = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (N,), generator=g)]
    return dict(item_mask=mask, ban_indptr=indptr, ban_indices=indices,
                item_cats=ic, query_cats=qc, item_weights=w)


def _reference(Xq, Y, flt):
    """[B, N] float64 scores, -inf where an item fails a filter."""
    s = Xq.double() @ Y.double().t()
    if not flt:
        return s
    s = s * flt["item_weights"].double()
    ok = ((flt["item_cats"].unsqueeze(0) & flt["query_cats"].unsqueeze(1))
          != 0).any(dim=2)
    ok &= ~flt["item_mask"].bool().unsqueeze(0)
    ip = flt["ban_indptr"].tolist()
    for b in range(Xq.shape[0]):
        ok[b, flt["ban_indices"][ip[b]:ip[b + 1]].long()] = False
    return s.masked_fill(~ok, float("-inf"))


def _check(Xq, Y, K, flt=None, **kw):
    from predictionio_amd.ops.topk import topk_score
    flt = flt or {}
    vals, idx = topk_score(Xq.cuda(), Y.cuda(), K,
                           **{k: v.cuda() for k, v in flt.items()}, **kw)
    torch.cuda.synchronize()
    vals, idx = vals.cpu().double(), idx.cpu()
    B, N = Xq.shape[0], Y.shape[0]
    assert vals.shape == (B, K) and idx.shape == (B, K)
    ref = _reference(Xq, Y, flt)
    want = torch.full((B, K), float("-inf"), dtype=torch.float64)
    want[:, :min(K, N)] = torch.topk(ref, min(K, N), dim=1).values
    assert torch.equal(vals, want)
    assert torch.equal(idx == -1, vals == float("-inf"))
    for b in range(B):
        ids = idx[b][idx[b] >= 0]
        assert ids.unique().numel() == ids.numel() and bool((ids < N).all())
        # equal to a finite returned value, so the id passed every filter
        assert torch.equal(ref[b, ids], vals[b, :ids.numel()])


def _route(monkeypatch, route):
    if route == "list":
        monkeypatch.setenv("PIO_TOPK_UNION", "0")
        return {}
    return {"mode": "union"}


@requires_gpu
@pytest.mark.parametrize("route", ["union", "list"])
@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("B,N", [(1, 200), (70, 200)])
@pytest.mark.parametrize("f", [129, 256, 300, 384, 512])
def test_main_grid(monkeypatch, f, B, N, K, route):
    """Padding into each panel count and the exact widths; a tail query
    block and two blocks; 4 chunks with an 8-item tail chunk."""
    _check(*_problem(B, N, f), K, **_route(monkeypatch, route))


@requires_gpu
@pytest.mark.parametrize("B,N,pin", [
    (1, 200, dict(list_k=64, n_slices=4)),
    (70, 200, dict(list_k=64, n_slices=4)),
    (70, 1000, {})])
@pytest.mark.parametrize("f", [129, 256, 300, 384, 512])
def test_k100_union(f, B, N, pin):
    """K = 100. At N = 200 the 2K shortlist is every item, which the plan
    rule does not reach with 4 chunks, so the plan is pinned (64 x 4: every
    item is kept, the case checks scores). N = 1000 has a plan of its own,
    (40, 13): lists shorter than their slices of one or two chunks, the
    last chunk partial, so the selection and the flag fallback run too."""
    _check(*_problem(B, N, f), 100, mode="union", **pin)


@requires_gpu
@pytest.mark.parametrize("route", ["union", "list"])
@pytest.mark.parametrize("NP,p", [(n, p) for n in (2, 3, 4) for p in range(n)])
def test_panel_order(monkeypatch, NP, p, route):
    """Xq is zero outside panel p, and inside it each 32-column k-step
    carries its own multiplier: pairing panel p of Y with another panel's
    X fragment, or permuting k-steps inside a panel, changes the scores."""
    Xq, Y = _problem(5, 200, 128 * NP)
    Xp = torch.zeros_like(Xq)
    for ks in range(4):
        c = slice(128 * p + 32 * ks, 128 * p + 32 * ks + 32)
        Xp[:, c] = Xq[:, c] * (ks + 1)
    _check(Xp, Y, 20, **_route(monkeypatch, route))


@requires_gpu
@pytest.mark.parametrize("route", ["union", "list"])
@pytest.mark.parametrize("N,kw", [(200, {}), (2000, dict(n_slices=3))])
@pytest.mark.parametrize("NP", [2, 3, 4])
def test_filters(monkeypatch, NP, N, kw, route):
    """item_mask, ban lists, W = 2 categories and weights together. At
    N = 2000 in 3 slices a slice runs 10 or 11 chunks, so each parity
    buffer of the staged category words and weights is reused."""
    B = 70
    _check(*_problem(B, N, 128 * NP - 3), 20, _filters(B, N, NP),
           **_route(monkeypatch, route), **kw)


@requires_gpu
def test_cross_slice_threshold(monkeypatch):
    """List route, 3 contiguous slices of 11 chunks each: the threshold
    cell is published by full lists and folded in at chunk 8."""
    monkeypatch.setenv("PIO_TOPK_UNION", "0")
    _check(*_problem(70, 2000, 256), 5, n_slices=3)


@requires_gpu
def test_rank_256_is_served():
    """topk_score and cosine_topk at rank 256, K = 20, on the device
    return (they raised ValueError: rank > 128 not supported)."""
    from predictionio_amd.ops.topk import cosine_topk, topk_score
    Xq, Y = _problem(1, 200, 256)
    want = torch.topk(Xq.double() @ Y.double().t(), 20, dim=1).values
    for vals, idx in (topk_score(Xq.cuda(), Y.cuda(), 20),
                      cosine_topk(Xq[0].cuda(), Y.cuda(), 20)):
        assert torch.equal(vals.cpu().double(), want)
        assert idx.shape == (1, 20) and int(idx.min()) >= 0
