"""Held-out ranking evaluation: exact ranks of held-out items.

For every held-out pair (b, t) of a test CSR, with s_bj = x_b . y_j and
the candidates C_b = all items but the user's seen (training) items:

    gt = #{j in C_b : s_bj > s_bt}
    eq = #{j in C_b, j != t : s_bj == s_bt}

and n_cand[b] = N - |seen_b|. From these follow the expected percentile
rank of Hu, Koren and Volinsky (MPR), AUC, recall@K, MRR and NDCG@K
(ranking_metrics). On the GPU the counts come from the fused fp32-MFMA
kernels of csrc/rank_count.hip and no B x N score matrix exists; the
plain-torch heldout_ranks_ref is the CPU path and, in float64, the oracle.
"""

from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from predictionio_amd.ops.als import pad_rank


def _check_csr(indptr: torch.Tensor, indices: torch.Tensor, B: int,
               name: str) -> None:
    if (indptr.dtype != torch.int64 or indptr.dim() != 1
            or indptr.numel() != B + 1):
        raise ValueError(f"{name}_indptr must be a 1-D int64 tensor of B + 1")
    if indices.dtype != torch.int32 or indices.dim() != 1:
        raise ValueError(f"{name}_indices must be a 1-D int32 tensor")


def _not_finite(t: torch.Tensor) -> torch.Tensor:
    """Scalar bool tensor: t holds a NaN or an infinity. One min/max
    reduction (both propagate NaN) and no temporary: isfinite(t).all()
    allocated 1.75 times the size of a multi-GB factor matrix."""
    if t.numel() == 0:
        return torch.zeros((), dtype=torch.bool, device=t.device)
    mn, mx = torch.aminmax(t)
    return ~(torch.isfinite(mn) & torch.isfinite(mx))


def _validate(X, Y, test_indptr, test_indices, seen_indptr, seen_indices):
    """The contract of heldout_ranks, checked on the tensors' device with
    one transfer to the host. Every id the kernels gather by is checked
    here: they trust what they are given."""
    if (X.dim() != 2 or Y.dim() != 2 or X.shape[1] != Y.shape[1]
            or X.dtype != torch.float32 or Y.dtype != torch.float32):
        raise ValueError("X [B, f] and Y [N, f] must be fp32 with one rank")
    B, f = X.shape
    N = Y.shape[0]
    if not 1 <= f <= 128:
        raise ValueError("rank must be in [1, 128]")
    if N < 1 or N >= 2 ** 31:
        raise ValueError("the item count N must be in [1, 2^31)")
    if (seen_indptr is None) != (seen_indices is None):
        raise ValueError("seen_indptr and seen_indices must be given "
                         "together")
    _check_csr(test_indptr, test_indices, B, "test")
    lists = [("test", test_indptr, test_indices)]
    if seen_indptr is not None:
        _check_csr(seen_indptr, seen_indices, B, "seen")
        lists.append(("seen", seen_indptr, seen_indices))
    dev = X.device
    if any(t.device != dev for t in (Y, *[a for _, p, i in lists
                                          for a in (p, i)])):
        raise ValueError("all tensors must share a device")
    flags, names = [], []

    def flag(cond, msg):
        flags.append(cond.reshape(()))
        names.append(msg)

    flag(_not_finite(X) | _not_finite(Y), "X and Y must be finite")
    keys = []
    for name, ip, ci in lists:
        nnz = ci.numel()
        lens = ip[1:] - ip[:-1]
        is_start = torch.zeros(nnz + 1, dtype=torch.bool, device=dev)
        is_start[ip.clamp(0, nnz)] = True
        flag((ip[0] != 0) | (ip[-1] != nnz),
             f"{name}_indptr must run from 0 to len({name}_indices)")
        flag((lens < 0).any(), f"{name}_indptr must not decrease")
        flag(((ci < 0) | (ci >= N)).any(),
             f"{name}_indices holds an id outside [0, {N})")
        flag(((ci[1:] <= ci[:-1]) & ~is_start[1:nnz]).any(),
             f"{name}_indices must be strictly ascending inside every user")
        keys.append((ip, lens, ci))
    bad = torch.stack(flags).tolist()
    for b, msg in zip(bad, names):
        if b:
            raise ValueError(msg)
    if len(keys) == 2 and keys[0][2].numel() and keys[1][2].numel():
        # the CSRs are sound by now: (user, item) keys of both, one sort
        k = [torch.repeat_interleave(
                torch.arange(B, device=dev), lens) * N + ci.long()
             for _, lens, ci in keys]
        allk = torch.sort(torch.cat(k)).values
        if bool((allk[1:] == allk[:-1]).any()):
            raise ValueError("a held-out item is also in its user's seen "
                             "list")


def _pad_factors(X: torch.Tensor, Y: torch.Tensor):
    f = X.shape[1]
    pf = pad_rank(f)
    if pf != f:
        X = torch.nn.functional.pad(X, (0, pf - f))
        Y = torch.nn.functional.pad(Y, (0, pf - f))
    return X.contiguous(), Y.contiguous(), pf


def default_slices(n_groups: int, N: int, pf: int, lds_bytes: int) -> int:
    """Item slices of the stream kernel: enough workgroups to fill the
    chip once (256 CUs x what fits a CU: at most 4 four-wave workgroups
    by registers, fewer by LDS), as for the MFMA top-K; never slices
    shorter than eight 64-item chunks."""
    target = 256 * max(1, min(4 if pf <= 64 else 2,
                              (160 * 1024) // lds_bytes))
    n_chunks = (N + 63) // 64
    return int(max(1, min(-(-target // n_groups), (n_chunks + 7) // 8,
                          65535)))


def _build_slots(test_indptr: torch.Tensor, test_indices: torch.Tensor,
                 tmax: int, group: int):
    """Slots of at most tmax targets: (slot_user [S] int32, slot_tgt
    [S, tmax] int32 with -1 for none, n_real), S padded to a multiple of
    `group` with slots of user 0 and no targets. Slots are in user order
    and targets keep their order, so slot_tgt >= 0 selects the pairs in
    the order of test_indices."""
    dev = test_indptr.device
    B = test_indptr.numel() - 1
    lens = test_indptr[1:] - test_indptr[:-1]
    per_user = (lens + tmax - 1) // tmax
    n_real = int(per_user.sum())
    S = -(-max(n_real, 1) // group) * group
    slot_user = torch.zeros(S, dtype=torch.int32, device=dev)
    slot_tgt = torch.full((S, tmax), -1, dtype=torch.int32, device=dev)
    if n_real:
        users = torch.repeat_interleave(torch.arange(B, device=dev), per_user)
        first_slot = torch.cumsum(per_user, 0) - per_user
        within = torch.arange(n_real, device=dev) - first_slot[users]
        pos = (test_indptr[users] + within * tmax)[:, None] + \
            torch.arange(tmax, device=dev)[None, :]
        ok = pos < test_indptr[users + 1][:, None]
        ids = test_indices[pos.clamp_max(max(test_indices.numel() - 1, 0))]
        slot_user[:n_real] = users.to(torch.int32)
        slot_tgt[:n_real] = torch.where(ok, ids, torch.full_like(ids, -1))
    return slot_user, slot_tgt, n_real


def heldout_ranks(X: torch.Tensor, Y: torch.Tensor,
                  test_indptr: torch.Tensor, test_indices: torch.Tensor,
                  seen_indptr: Optional[torch.Tensor] = None,
                  seen_indices: Optional[torch.Tensor] = None, *,
                  count_ties: bool = True, n_slices: Optional[int] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(gt [nnz_test], eq [nnz_test], n_cand [B]) int32, exact; see the
    module docstring. X [B, f], Y [N, f] fp32; test / seen CSRs over the B
    users (indptr int64, indices int32, strictly ascending per user,
    disjoint). count_ties=False skips eq (zeros).

    CUDA tensors take the fused kernels: s_bj is then one fp32 fma chain
    in a fixed k order, the same bits for a target and for the streamed
    item. A rank f outside {16, 32, 64, 128} is zero-padded once to the
    next of them (a copy of X and Y). n_slices pins the item split of the
    stream kernel. CPU tensors take heldout_ranks_ref.

    Everything is validated before any launch; each violation raises
    ValueError."""
    _validate(X, Y, test_indptr, test_indices, seen_indptr, seen_indices)
    if n_slices is not None and n_slices < 1:
        raise ValueError("n_slices must be >= 1")
    if not X.is_cuda:
        return heldout_ranks_ref(X, Y, test_indptr, test_indices,
                                 seen_indptr, seen_indices,
                                 count_ties=count_ties, _checked=True)
    from predictionio_amd.ops import hip_ext
    ext = hip_ext()
    B, N = X.shape[0], Y.shape[0]
    n_cand = _n_cand(B, N, seen_indptr, X.device)
    nnz = test_indices.numel()
    if nnz == 0:
        z = torch.zeros(0, dtype=torch.int32, device=X.device)
        return z, z.clone(), n_cand
    Xp, Yp, pf = _pad_factors(X, Y)
    tmax, group = ext.rank_count_tmax(), ext.rank_count_group()
    slot_user, slot_tgt, _ = _build_slots(test_indptr, test_indices, tmax,
                                          group)
    if n_slices is None:
        n_slices = default_slices(slot_user.numel() // group, N, pf,
                                  ext.rank_stream_lds_bytes(pf))
    n_slices = min(int(n_slices), (N + 63) // 64, 65535)
    if seen_indptr is not None:
        tscore, corr = ext.rank_list(Xp, Yp, slot_user, slot_tgt,
                                     seen_indptr.contiguous(),
                                     seen_indices.contiguous())
    else:
        tscore, corr = ext.rank_list(Xp, Yp, slot_user, slot_tgt)
    partial = ext.rank_stream(Xp, Yp, slot_user, tscore, n_slices,
                              bool(count_ties))
    has = slot_tgt >= 0
    gt = (partial[:, :, 0].sum(0) - corr[:, 0])[has].to(torch.int32)
    if count_ties:
        ge = (partial[:, :, 1].sum(0) - corr[:, 1])[has].to(torch.int32)
        eq = ge - gt - 1  # the target itself, counted once by >=
    else:
        eq = torch.zeros_like(gt)
    return gt, eq, n_cand


def _n_cand(B: int, N: int, seen_indptr, device) -> torch.Tensor:
    if seen_indptr is None:
        return torch.full((B,), N, dtype=torch.int32, device=device)
    return (N - (seen_indptr[1:] - seen_indptr[:-1])).to(torch.int32)


def heldout_ranks_ref(X: torch.Tensor, Y: torch.Tensor,
                      test_indptr: torch.Tensor, test_indices: torch.Tensor,
                      seen_indptr: Optional[torch.Tensor] = None,
                      seen_indices: Optional[torch.Tensor] = None, *,
                      count_ties: bool = True,
                      dtype: torch.dtype = torch.float32,
                      block_elems: int = 1 << 24, _checked: bool = False
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """heldout_ranks in plain torch on the tensors' device: users in
    blocks of about block_elems scores, one GEMM per block in `dtype`
    (float64: the oracle). Seen items are made NaN, which no compare
    accepts."""
    if not _checked:
        _validate(X, Y, test_indptr, test_indices, seen_indptr, seen_indices)
    dev = X.device
    B, N = X.shape[0], Y.shape[0]
    nnz = test_indices.numel()
    gt = torch.zeros(nnz, dtype=torch.int32, device=dev)
    eq = torch.zeros(nnz, dtype=torch.int32, device=dev)
    n_cand = _n_cand(B, N, seen_indptr, dev)
    Yd = Y.to(dtype)
    ptr = test_indptr.tolist()
    step = max(1, block_elems // N)
    for lo in range(0, B, step):
        hi = min(B, lo + step)
        if ptr[hi] == ptr[lo]:
            continue
        S = X[lo:hi].to(dtype) @ Yd.t()
        if seen_indptr is not None:
            a, b = int(seen_indptr[lo]), int(seen_indptr[hi])
            rows = torch.repeat_interleave(
                torch.arange(hi - lo, device=dev),
                seen_indptr[lo + 1:hi + 1] - seen_indptr[lo:hi])
            S[rows, seen_indices[a:b].long()] = float("nan")
        lens = test_indptr[lo + 1:hi + 1] - test_indptr[lo:hi]
        for m in range(int(lens.max())):
            rows = torch.nonzero(lens > m)[:, 0]
            at = test_indptr[lo:hi][rows] + m
            t = S[rows, test_indices[at].long()][:, None]
            gt[at] = (S[rows] > t).sum(1).to(torch.int32)
            if count_ties:
                eq[at] = ((S[rows] == t).sum(1) - 1).to(torch.int32)
    return gt, eq, n_cand


def ranking_metrics(gt: torch.Tensor, eq: torch.Tensor, n_cand: torch.Tensor,
                    test_indptr: torch.Tensor, ks: Sequence[int] = (10,),
                    weights: Optional[torch.Tensor] = None
                    ) -> Dict[str, float]:
    """Ranking metrics from the counts of heldout_ranks, in float64.

    A pair's position is p = gt + eq / 2 (0 = first; ties share the middle
    of their run). mpr: mean of p / max(n_cand_b - 1, 1) over the pairs,
    weighted by `weights` [nnz] if given (Hu et al.'s rank-bar); auc =
    1 - mpr. Over the users with at least one target: recall@K = mean
    share of targets with p < K; mrr = mean of 1 / (1 + min p); ndcg@K =
    mean of sum_{p < K} 1 / log2(2 + p) over the ideal DCG of
    min(|T_b|, K) hits. n_users / n_pairs count what was averaged."""
    dev = gt.device
    ip = test_indptr.to(dev)
    B = ip.numel() - 1
    lens = ip[1:] - ip[:-1]
    nnz = gt.numel()
    out: Dict[str, float] = {"n_users": int((lens > 0).sum()),
                             "n_pairs": int(nnz)}
    nan = float("nan")
    if nnz == 0:
        out.update(mpr=nan, auc=nan, mrr=nan)
        for K in ks:
            out[f"recall@{K}"] = nan
            out[f"ndcg@{K}"] = nan
        return out
    user = torch.repeat_interleave(torch.arange(B, device=dev), lens)
    p = gt.double() + eq.double() / 2
    denom = (n_cand.to(dev).double() - 1).clamp_min(1)[user]
    w = (torch.ones_like(p) if weights is None
         else weights.to(dev).double())
    mpr = float((w * p / denom).sum() / w.sum())
    out["mpr"] = mpr
    out["auc"] = 1.0 - mpr
    active = lens > 0
    nu = float(active.sum())
    best = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    best.scatter_reduce_(0, user, p, reduce="amin")
    out["mrr"] = float((1.0 / (1.0 + best[active])).sum() / nu)
    lf = lens.double()
    for K in ks:
        hit = (p < K).double()
        hits = torch.zeros(B, dtype=torch.float64, device=dev)
        hits.scatter_add_(0, user, hit)
        out[f"recall@{K}"] = float((hits[active] / lf[active]).sum() / nu)
        dcg = torch.zeros(B, dtype=torch.float64, device=dev)
        dcg.scatter_add_(0, user, hit / torch.log2(2.0 + p))
        ideal = torch.cumsum(torch.tensor(
            [0.0] + [1.0 / math.log2(2.0 + i) for i in range(int(K))],
            dtype=torch.float64, device=dev), 0)
        idcg = ideal[lens.clamp_max(int(K))]
        out[f"ndcg@{K}"] = float((dcg[active] / idcg[active]).sum() / nu)
    return out
