"""Per-item score weights on the GPU: every route of `topk_score` against
the fp64 brute force and exact integer data of test_topk_weights_cpu."""

import functools

import pytest
import torch

from test_topk_weights_cpu import check, problem

pytestmark = pytest.mark.gpu

N, SLICES = 5000, 7
SEAMS = tuple(-(-N // SLICES) * k for k in range(1, SLICES))
cached_problem = functools.lru_cache(maxsize=None)(problem)


def run(monkeypatch, route, K, prob, **extra):
    """route: list<gth> = the MFMA list kernel, None = candidates, or mode"""
    from predictionio_amd.ops import topk as topk_ops
    (Xq, Y, kw), S64, valid = prob
    mode = route
    if route and route.startswith("list"):
        monkeypatch.setenv("PIO_TOPK_UNION", "0")
        monkeypatch.setenv("PIO_TOPK_GTH", route[-1])
        mode = "mfma"
    dev = {k: v.cuda() for k, v in kw.items()}
    dev.update(extra)
    calls = topk_ops.union_stats()["calls"]
    v, idx = topk_ops.topk_score(Xq.cuda(), Y.cuda(), K, mode=mode, **dev)
    assert (topk_ops.union_stats()["calls"] > calls) == (route == "union")
    return v, idx, S64, valid, K


@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("route,f", [
    ("list0", 32), ("list1", 32), ("list1", 64), ("list0", 128),
    ("list1", 128), ("fp32", 16), ("fp32", 64)])
def test_sliced_with_tail_chunks(monkeypatch, route, f, K):
    prob = cached_problem(37, N, f, f, seams=SEAMS)
    check(*run(monkeypatch, route, K, prob, n_slices=SLICES))


@pytest.mark.parametrize("route", ["list1", "fp32"])
def test_three_query_blocks(monkeypatch, route):
    check(*run(monkeypatch, route, 20, cached_problem(130, N, 64, 1)))


@pytest.mark.parametrize("route,K,n", [
    ("union", 20, N), ("union", 100, N), ("mfma", 1100, 1500)])
def test_union_and_materialized_fallback(monkeypatch, route, K, n):
    check(*run(monkeypatch, route, K, cached_problem(37, n, 64, 2)))


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("route", ["list1", "union", "fp32"])
def test_with_every_filter(monkeypatch, route, W):
    # a multiply after the -FLT_MAX select would serve filtered items
    prob = cached_problem(37, N, 64, 5 + W, W, True, SEAMS)
    check(*run(monkeypatch, route, 20, prob, n_slices=SLICES))


@pytest.mark.parametrize("K", [20, 100])       # selection / scores mode
@pytest.mark.parametrize("f", [10, 64])        # scalar / float4 row loads
@pytest.mark.parametrize("W,filters", [(0, False), (2, True)])
def test_candidate_lists(monkeypatch, f, K, W, filters):
    prob = cached_problem(4, N, f, 8 + f, W, filters,
                          cand_lens=(1, 256, 257, 3000))
    (Xq, Y, kw), S64, valid = prob
    raw = Xq.double() @ Y.double().t()
    zero = (kw["item_weights"] == 0)[None] & valid
    assert (zero & (raw < 0)).any() and (zero & (raw > 0)).any()
    check(*run(monkeypatch, None, K, prob), exact_ids=True)


@pytest.mark.parametrize("route,K", [
    ("list1", 20), ("fp32", 20), ("union", 100), ("mfma", 1100),
    ("cands", 20), ("cands", 100)])
def test_none_changes_nothing(monkeypatch, route, K):
    cands = (1, 256, 257, 1000) if route == "cands" else None
    (Xq, Y, kw), S64, valid = cached_problem(4, 1500, 64, 9,
                                             cand_lens=cands)
    plain = ((Xq, Y, {k: v for k, v in kw.items() if k != "item_weights"}),
             S64, valid)
    route = None if route == "cands" else route
    v0, i0 = run(monkeypatch, route, K, plain)[:2]
    v1, i1 = run(monkeypatch, route, K, plain, item_weights=None)[:2]
    assert torch.equal(v0, v1) and torch.equal(i0, i1)


@pytest.mark.parametrize("bad", ["dtype", "length", "strided", "cpu"])
@pytest.mark.parametrize("route", ["list1", "fp32", "union", "cands"])
def test_validation(monkeypatch, route, bad):
    cands = (5, 9) if route == "cands" else None
    prob = cached_problem(2, 300, 64, 0, cand_lens=cands)
    w = prob[0][2]["item_weights"].cuda()
    w = {"dtype": w.double(), "length": w[:-1],
         "strided": torch.stack([w, w], 1)[:, 0], "cpu": w.cpu()}[bad]
    with pytest.raises(ValueError):
        run(monkeypatch, None if route == "cands" else route, 5, prob,
            item_weights=w)
