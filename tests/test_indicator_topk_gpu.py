"""csrc/indicator_topk.hip through indicator_topk, against the brute force
of test_indicator_topk_cpu.py: both instantiations and the torch route in
one call, a long run, high id bits, every filter, real LLR values."""

import copy

import pytest
import torch

from predictionio_amd.ops.cooccurrence import (
    cross_occurrence_topn, indicator_topk,
)
from test_indicator_topk_cpu import (
    FILTERS, NR, QUERIES, VALIDATION, brute, cooc_model, csr, filter_kw,
    table,
)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.int32, torch.float32]


def run(ids, sc, queries, K, **kw):
    out = indicator_topk(ids.to(DEV), sc.to(DEV), *csr(queries, DEV), K, **kw)
    torch.cuda.synchronize()
    return out[0].tolist(), out[1].tolist()


# rows per query; with n = 64 the entry counts are 0, 64, 512 (the wave
# tier full), 576, 8192 (the workgroup tier full) and 8256 (torch route);
# with n = 57 query 9 has 513, the first workgroup size; with n = 1 E = 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,K", [(1, 3), (57, 1024), (64, 20)])
def test_every_route_in_one_batch(dtype, n, K):
    nr = 160
    ids, sc = table(nr, n, nr, dtype, seed=n)
    g = torch.Generator().manual_seed(7)
    queries = [sorted(torch.randperm(nr, generator=g)[:m].tolist())
               for m in (9, 0, 129, 1, 128, 8)]
    want = brute(ids.tolist(), sc.tolist(), queries, K)
    assert run(ids, sc, queries, K) == want   # eighths: fp32 sums are exact


def test_popular_item_run_and_count_ties():
    ids, sc = table(130, 8, 129, torch.int32, seed=11)
    ids[torch.arange(130), torch.arange(130) % 8] = 129  # in every row
    sc = sc % 3                                          # many tied sums
    queries = [list(range(128)), [128, 129]]
    want = brute(ids.tolist(), sc.tolist(), queries, 40)
    assert want[0][0].count(129) == 1
    assert run(ids, sc, queries, 40) == want


def test_high_id_bits():
    n_cols = 2 ** 31 - 1
    g = torch.Generator().manual_seed(13)
    ids = torch.stack([n_cols - 1 - torch.randperm(8, generator=g)[:4]
                       for _ in range(16)]).to(torch.int32)
    sc = torch.randint(0, 9, (16, 4), generator=g, dtype=torch.int32)
    queries = [list(range(16)), [3], [1, 2, 5]]
    ban = [[n_cols - 3], [], [n_cols - 8, n_cols - 1]]
    bp, bi = csr(ban, DEV)
    want = brute(ids.tolist(), sc.tolist(), queries, 8, own=False, ban=ban)
    # eight ids, one banned: seven candidates, all within 8 of the top
    assert min(want[0][0][:7]) >= n_cols - 8 and want[0][0][7] == -1
    got = run(ids, sc, queries, 8, n_cols=n_cols, exclude_query=False,
              ban_indptr=bp, ban_indices=bi)
    assert got == want


# n = 32: query 4 (20 rows, 640 entries) runs in the workgroup kernel, the
# others in the wave kernel
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("K", [4, 64])  # 64: fewer survivors than K
def test_filters(dtype, filt, K):
    ids, sc = table(NR, 32, NR, dtype, seed=3)
    op, br = filter_kw(filt, DEV)
    want = brute(ids.tolist(), sc.tolist(), QUERIES, K, **br)
    assert run(ids, sc, QUERIES, K, **op) == want


def test_real_llr_values():
    g = torch.Generator().manual_seed(17)
    U, na, nb, n = 200, 60, 50, 16
    ua, ub = (torch.randint(0, U, (1500,), generator=g) for _ in range(2))
    ia = torch.randint(0, na, (1500,), generator=g)
    ib = torch.randint(0, nb, (1500,), generator=g)
    ids, sc = cross_occurrence_topn(ua.to(DEV), ia.to(DEV), na, ub.to(DEV),
                                    ib.to(DEV), nb, U, n, score="llr")
    queries = [sorted(torch.randperm(na, generator=g)[:m].tolist())
               for m in (1, 5, 20, 40, 33)]
    K = 10
    kw = dict(n_cols=nb, exclude_query=False)
    qp, qi = csr(queries, DEV)
    got_ids, got_sc = indicator_topk(ids, sc, qp, qi, K, **kw)
    # every candidate's fp64 sum, in order
    all_ids, all_sc = brute(ids.tolist(), sc.double().tolist(), queries, nb,
                            own=False)
    for b, q in enumerate(queries):
        s64 = dict(zip(all_ids[b], all_sc[b]))
        eps = (len(q) - 1) * 2.0 ** -24
        row_ids, row_sc = got_ids[b].tolist(), got_sc[b].tolist()
        real = min(K, len(all_ids[b]) - all_ids[b].count(-1))
        assert len(set(row_ids[:real]) - {-1}) == real
        assert row_ids[real:] == [-1] * (K - real)
        for r, (j, s) in enumerate(zip(row_ids[:real], row_sc)):
            assert abs(s - s64[j]) <= eps * s64[j]
            assert abs(s - all_sc[b][r]) <= eps * all_sc[b][r]
        assert row_sc == sorted(row_sc, reverse=True)
    again = indicator_topk(ids, sc, qp, qi, K, **kw)
    assert torch.equal(again[0], got_ids) and torch.equal(again[1], got_sc)
    perm = torch.argsort(torch.rand((na, n), generator=g), dim=1).to(DEV)
    permuted = indicator_topk(ids.gather(1, perm), sc.gather(1, perm), qp, qi,
                              K, **kw)
    assert torch.equal(permuted[0], got_ids)
    assert torch.equal(permuted[1], got_sc)


@pytest.mark.parametrize("case", list(VALIDATION))
def test_validation_errors_on_device(case):
    a = {k: v.to(DEV) if torch.is_tensor(v) else v
         for k, v in VALIDATION[case]().items()}
    pos = [a.pop(k) for k in ("top_ids", "top_scores", "q_indptr", "q_items",
                              "K")]
    with pytest.raises(ValueError):
        indicator_topk(*pos, **a)


def test_batch_predict_on_device_equals_cpu():
    algo, model, queries = cooc_model()
    assert model.device_table()[0].is_cuda
    indexed = list(enumerate(queries))
    got = algo.batch_predict(model, indexed)
    want = algo.batch_predict(copy.copy(model).to("cpu"), indexed)
    assert got == want and any(r.item_scores for _, r in got)
