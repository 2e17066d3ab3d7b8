"""Candidate-list top-K on CPU tensors: topk_score_cands_ref against the
float64 reference (exact inputs, bit-for-bit), and the argument checks."""

import pytest
import torch

from _topk_oracle import int_problem, reference_topk, valid_items
from predictionio_amd.ops import topk as topk_ops

N = 256


def _csr(lists):
    ip = torch.tensor([0] + [len(c) for c in lists]).cumsum(0)
    ci = torch.tensor([j for c in lists for j in c], dtype=torch.int32)
    return ip, ci


@pytest.mark.parametrize("f,K", [(10, 1), (64, 20), (128, 64), (64, 300)])
@pytest.mark.parametrize("filtered", [False, True])
def test_ref_matches_float64(f, K, filtered):
    lens = [0, 1, K - 1, K, 17, 65, 200]
    B = len(lens)
    Xq, Y = int_problem(B, N, f, seed=K)
    g = torch.Generator().manual_seed(f + K)
    lists = [sorted(torch.randperm(N, generator=g)[:min(c, N)].tolist())
             for c in lens]
    member = torch.zeros((B, N), dtype=torch.bool)
    for b, c in enumerate(lists):
        member[b, c] = True
    flt = {}
    if filtered:
        top = reference_topk(Xq, Y, 1, member)[1][:, 0].clamp_min(0)
        flt["item_mask"] = torch.zeros(N, dtype=torch.uint8)
        flt["item_mask"][top[::2]] = 1
        flt["ban_indptr"], flt["ban_indices"] = _csr(
            [sorted({int(top[b]), b}) for b in range(B)])
        j = torch.arange(N)
        flt["item_cats"] = (1 << (j % 5)).int().view(N, 1)
        flt["query_cats"] = torch.full((B, 1), 0b10111, dtype=torch.int32)
    ip, ci = _csr(lists)
    want = reference_topk(Xq, Y, K, valid_items(B, N, **flt) & member)
    for fn in (topk_ops.topk_score, topk_ops.topk_score_ref,
               topk_ops.topk_score_cands_ref):
        v, i = fn(Xq, Y, K, cand_indptr=ip, cand_indices=ci, **flt)
        assert v.dtype == torch.float32 and i.dtype == torch.int64
        assert torch.equal(i, want[1]) and torch.equal(v, want[0])


def test_ties_id_ascending():
    Y = torch.zeros((8, 4))
    Y[:, 0] = torch.tensor([3., 5, 5, 1, 5, 3, 9, 9])
    Xq = torch.tensor([[1., 0, 0, 0]])
    ip, ci = _csr([[0, 1, 2, 4, 5, 7]])
    v, i = topk_ops.topk_score(Xq, Y, 5, cand_indptr=ip, cand_indices=ci)
    assert i[0].tolist() == [7, 1, 2, 4, 0]
    assert v[0].tolist() == [9, 5, 5, 5, 3]


@pytest.mark.parametrize("ip,ci", [
    ([0, 3], [1, 2, N]),          # out of range
    ([0, 3], [-1, 2, 3]),         # negative
    ([0, 3], [1, 3, 2]),          # unsorted
    ([0, 3], [1, 2, 2]),          # duplicated
    ([0, 2], [1, 2, 3]),          # indptr does not end at nnz
    ([1, 3], [1, 2, 3]),          # indptr does not start at 0
    ([0, 3, 2], [1, 2]),          # indptr decreases
    ([0, 3], None),               # one of the two
])
def test_validation(ip, ci):
    Xq, Y = int_problem(len(ip) - 1, N, 10)
    kw = dict(cand_indptr=torch.tensor(ip))
    if ci is not None:
        kw["cand_indices"] = torch.tensor(ci, dtype=torch.int32)
    with pytest.raises(ValueError):
        topk_ops.topk_score(Xq, Y, 5, **kw)
