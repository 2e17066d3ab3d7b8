"""Per-item score weights on the CPU: the torch references against an fp64
brute force; the e-commerce template ranks on weight * score. Integer
factors and WSET weights make every score exact in bf16/fp32/fp64."""

import pytest
import torch

from predictionio_amd.ops import topk as topk_ops

WSET = torch.tensor([-1.0, 0.0, 0.25, 0.5, 1.0, 2.0, 8.0])
INF = float("inf")


def problem(B, N, f, seed, W=0, filters=False, seams=(), cand_lens=None):
    """((Xq, Y, kwargs), S64 [B,N] fp64 scores, valid [B,N]). Weight 8 at
    both ends and seams, 0 / -1 on top raw items and filtered items."""
    g = torch.Generator().manual_seed(seed)
    Xq = torch.randint(-2, 3, (B, f), generator=g).float()
    Y = torch.randint(-2, 3, (N, f), generator=g).float()
    w = WSET[torch.randint(0, len(WSET), (N,), generator=g)].clone()
    w[[j for s in (0, N, *seams) for j in (s - 1, s) if 0 <= j < N]] = 8.0
    raw = Xq.double() @ Y.double().t()
    top = raw.topk(min(4, N), dim=1).indices[:3]
    w[top[:, :2].flatten()] = 0.0
    w[top[:, 2:].flatten()] = -1.0
    kw = dict(item_weights=w)
    valid = torch.ones(B, N, dtype=torch.bool)
    if W:
        ic = torch.zeros((N, W), dtype=torch.int32)
        ic[torch.arange(N), torch.randint(0, W, (N,), generator=g)] = (
            1 << torch.randint(0, 31, (N,), generator=g)).int()
        ic[::11] = 0
        w[::22] = -1.0
        qc = torch.randint(0, 2 ** 31 - 1, (B, W), generator=g).int()
        qc[1] = 0                                  # nothing passes
        kw.update(item_cats=ic, query_cats=qc)
        valid &= ((ic[None] & qc[:, None]) != 0).any(-1)
    if filters:
        mask = (torch.rand(N, generator=g) < 0.1).to(torch.uint8)
        bans = [torch.randperm(N, generator=g)[:(b % 4) * 5].sort().values
                for b in range(B)]
        kw.update(item_mask=mask, ban_indices=torch.cat(bans).int(),
                  ban_indptr=torch.tensor(
                      [0] + [len(x) for x in bans]).cumsum(0))
        valid &= ~mask.bool()[None]
        for b, x in enumerate(bans):
            valid[b, x] = False
    if cand_lens is not None:
        cands = [torch.randperm(N, generator=g)[:n].sort().values
                 for n in cand_lens]
        kw.update(cand_indices=torch.cat(cands).int(),
                  cand_indptr=torch.tensor(
                      [0] + list(cand_lens)).cumsum(0))
        listed = torch.zeros_like(valid)
        for b, x in enumerate(cands):
            listed[b, x] = True
        valid &= listed
    return (Xq, Y, kw), raw * w.double() + 0.0, valid


def check(v, idx, S64, valid, K, exact_ids=False):
    """Exact values; distinct, unfiltered ids; -inf / -1 tail padding."""
    v, idx = v.cpu().double(), idx.cpu()
    ref = S64.masked_fill(~valid, -INF)
    rv, ri = ref.sort(dim=1, descending=True, stable=True)
    pad = max(0, K - ref.shape[1])
    rv = torch.nn.functional.pad(rv[:, :K], (0, pad), value=-INF)
    ri = torch.nn.functional.pad(ri[:, :K], (0, pad), value=-1)
    assert torch.equal(v, rv)
    live = rv > -INF
    assert torch.equal(idx >= 0, live)
    assert torch.equal(idx[~live], torch.full_like(idx[~live], -1))
    assert torch.equal(ref.gather(1, idx.clamp_min(0))[live], v[live])
    s = idx.sort(dim=1).values
    assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)).any()
    if exact_ids:
        assert torch.equal(idx, ri.masked_fill(~live, -1))


@pytest.mark.parametrize("W", [0, 1, 4])
@pytest.mark.parametrize("K", [1, 10, 250])
def test_ref_against_brute_force(W, K):
    (Xq, Y, kw), S64, valid = problem(5, 200, 8, 3 + W, W, filters=True)
    check(*topk_ops.topk_score(Xq, Y, K, **kw), S64, valid, K)


@pytest.mark.parametrize("W", [0, 2])
@pytest.mark.parametrize("K", [3, 70])
def test_cands_ref_against_brute_force(W, K):
    (Xq, Y, kw), S64, valid = problem(5, 200, 8, 7 + W, W, filters=True,
                                      cand_lens=[1, 0, 60, 200, 17])
    check(*topk_ops.topk_score(Xq, Y, K, **kw), S64, valid, K,
          exact_ids=True)


N_ITEMS, NUM = 12, 3


def _ecomm(storage, weighted=None):
    """User u0 scores item i_j at 12 - j; i0..i3 have 5, 4, 3, 1 buys."""
    from predictionio_amd.controller import Params
    from predictionio_amd.data.bimap import BiMap
    from predictionio_amd.data.storage.base import App
    from predictionio_amd.templates.ecommercerecommendation import engine as E
    app_id = storage.get_meta_data_apps().insert(App(id=0, name="WApp"))
    storage.get_l_events().init(app_id)
    names = [f"i{j}" for j in range(N_ITEMS)]
    Y = torch.zeros((N_ITEMS, 4))
    Y[:, 0] = torch.arange(N_ITEMS, 0, -1).float()
    model = E.ECommModel(
        4, torch.tensor([[1.0, 0, 0, 0]]), Y,
        torch.nn.functional.normalize(Y, dim=1), BiMap.string_int(["u0"]),
        BiMap.string_int(names), {n: E.Item(["c0"]) for n in names},
        {0: 5, 1: 4, 2: 3, 3: 1})
    p = {"appName": "WApp"}
    if weighted:
        p["weightedItems"] = weighted
    return E.ECommAlgorithm(Params(p)), model, app_id


def _both(algo, model, user="u0"):
    from predictionio_amd.templates.ecommercerecommendation import Query
    q = Query(user=user, num=NUM)
    out = [(s.item, s.score) for s in algo.predict(model, q).item_scores]
    batch = algo.batch_predict(model, [(0, q)])[0][1].item_scores
    assert [(s.item, s.score) for s in batch] == out
    return out


I7 = [{"items": ["i7"], "weight": 8.0}]


@pytest.mark.parametrize("groups,user,want", [
    # boosted from unweighted rank 8 > NUM
    (I7, "u0", [("i7", 40.0), ("i0", 12.0), ("i1", 11.0)]),
    # demoted (0.5 * 0.5) and replaced by the former rank NUM + 1
    ([{"items": ["i0", "i9"], "weight": 0.5}, {"items": ["i0"], "weight": 0.5}],
     "u0", [("i1", 11.0), ("i2", 10.0), ("i3", 9.0)]),
    # the popularity default
    ([{"items": ["i3"], "weight": 8.0}], "ghost",
     [("i3", 8.0), ("i0", 5.0), ("i1", 4.0)])])
def test_template_ranks_on_the_product(mem_storage, groups, user, want):
    algo, model, _ = _ecomm(mem_storage, groups)
    assert _both(algo, model, user) == want


def test_template_weights_from_constraint(mem_storage):
    from predictionio_amd.data.events import DataMap, Event, utcnow
    algo, model, app_id = _ecomm(mem_storage,
                                 [{"items": ["i1"], "weight": 0.0}])
    mem_storage.get_l_events().insert(Event(
        event="$set", entity_type="constraint", entity_id="weightedItems",
        properties=DataMap({"weights": I7}),
        event_time=utcnow()), app_id)
    assert _both(algo, model) == [("i7", 40.0), ("i0", 12.0), ("i1", 11.0)]
