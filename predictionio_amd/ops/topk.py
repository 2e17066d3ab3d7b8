"""Masked top-K scoring: fused HIP kernel on GPU, torch reference on CPU.

Replaces the reference's serve-time scoring:
recommendation recommendProductsWithFilter (ALSModel.scala:44-60),
similarproduct cosine top-N (ALSAlgorithm.scala:168-242), ecommerce
predictKnownUser/predictSimilar (ECommAlgorithm.scala:471-599).
"""

from __future__ import annotations

import logging
import math
import os
from typing import Dict, Optional, Tuple

import torch
from torch.utils.weak import WeakTensorKeyDictionary

from predictionio_amd.ops.als import check_row_count, pad_rank

log = logging.getLogger(__name__)

# cached bf16 copies of factor matrices for the MFMA scoring path,
# keyed weakly by the fp32 tensor (invalidated on in-place writes via
# _version). Serving keeps Y resident across batches, so the one-time
# fp32->bf16 cast amortizes to zero.
_bf16_cache: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()


def bf16_copy(t: torch.Tensor, pad_to: Optional[int] = None) -> torch.Tensor:
    """bf16 (optionally column-padded) copy of `t`, cached weakly on `t`
    and invalidated by in-place writes (_version)."""
    f = t.shape[-1]
    pad_to = pad_to or f
    ent = _bf16_cache.get(t)
    if ent is not None and ent[0] == t._version and ent[1] == pad_to:
        return ent[2]
    p = t if pad_to == f else torch.nn.functional.pad(t, (0, pad_to - f))
    b = p.to(torch.bfloat16).contiguous()
    _bf16_cache[t] = (t._version, pad_to, b)
    return b


def _mfma_rank(f: int) -> Optional[int]:
    """Padded rank for the MFMA kernels, or None when unsupported: 32, 64
    or 128 for topk_mfma_kernel, and 256, 384 or 512 (two to four 128-wide
    rank panels) for topk_mfma_wide_kernel."""
    for s in (32, 64, 128, 256, 384, 512):
        if f <= s:
            return s
    return None


def topk_score(Xq: torch.Tensor, Y: torch.Tensor, K: int,
               item_mask: Optional[torch.Tensor] = None,
               ban_indptr: Optional[torch.Tensor] = None,
               ban_indices: Optional[torch.Tensor] = None,
               n_slices: Optional[int] = None,
               mode: Optional[str] = None,
               item_cats: Optional[torch.Tensor] = None,
               query_cats: Optional[torch.Tensor] = None,
               list_k: Optional[int] = None,
               cand_indptr: Optional[torch.Tensor] = None,
               cand_indices: Optional[torch.Tensor] = None,
               item_weights: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-K of (Xq @ Y.T) per query row, with optional global item mask
    (uint8, 1=banned) and per-query banned lists (CSR int32, sorted).
    Returns (values [B,K] fp32, indices [B,K] int64), sorted descending.
    Banned/empty slots carry -inf / -1.

    item_cats [N,W] / query_cats [B,W] (int32 bit words, W in {1,2,4},
    given together or not at all) add a per-query category filter: item
    j is a candidate for query b iff any word of item_cats[j] &
    query_cats[b] is non-zero. It composes with item_mask and the ban
    lists — an item must pass all three.

    mode: "mfma" (default on GPU) scores on the matrix cores with bf16
    inputs / fp32 accumulate, shortlists each query's best D valid items
    by those scores, and re-scores the shortlist against the fp32
    factors, so returned values are fp32 dots and an item of the fp32
    top K is served whenever its bf16 rank among the valid items is at
    most D. "fp32" forces the all-fp32 VALU kernel (v3), which is exact.
    CPU ignores mode.

    Rank: "mfma" serves any rank up to 512. Ranks up to 128 are padded to
    32 / 64 / 128 and run topk_mfma_kernel; ranks 129..512 are padded to
    256 / 384 / 512 and run topk_mfma_wide_kernel, which streams the rank
    through LDS in 128-wide panels, with the same routes, filters, weights
    and shortlist contract. Above 512 there is no fused kernel: K <= 64
    raises ValueError and larger K takes the materialized fallback.
    mode="fp32" keeps its limit of 128 (ValueError above), and so do
    candidate lists.

    Eager "mfma" calls with K <= 1024 take the union path
    (_topk_score_union) when the shape has a plan for it: short
    per-slice lists over interleaved slices, merged to the exact bf16
    top 2K (D = 2K). Otherwise K <= 64 runs the list kernel
    (_topk_score_mfma) with D = min(2K, 64): shapes without a plan
    (N <= 64 among them), calls under stream capture (the union path
    syncs with the host) and PIO_TOPK_UNION=0. mode="union" forces the
    union path at any K >= 1 (ValueError when the shape admits no plan);
    list_k with n_slices pins its plan. K > 64 without the union path,
    and any K > 1024, use the materialized fallback, which is exact.

    cand_indptr [B+1] int64 / cand_indices int32 (a CSR, given together,
    ids strictly ascending within a query) restrict query b to its own
    candidate list: only the listed rows of Y are read, the three filters
    apply as above, and the result is exact fp32 in the order score
    descending, id ascending on equal scores (_topk_score_cands on GPU
    in every mode, topk_score_cands_ref on CPU).

    item_weights (contiguous fp32 [N] on the device of Y, shared by the
    batch) makes the served score of item j for query b
    (Xq[b] . Y[j]) * item_weights[j]: ranking, returned values, the
    cross-slice threshold, the shortlist depth and the tie rule are all
    defined on that product, in every route and under every filter above
    (an item must still pass them all). With weights the "mfma" contract
    reads: an item of the top K is served whenever its weighted bf16 rank
    among the valid items is at most D. Any finite weight is allowed: a
    negative one flips the score's sign, a zero one gives the score +0.0
    (never -0.0) and is no filter. Non-finite weights are the caller's
    responsibility and are not checked: an item whose score is NaN is
    never inserted by the fused kernels. A tensor of the wrong dtype,
    shape, layout or device raises ValueError; None changes nothing."""
    B, f = Xq.shape
    N = Y.shape[0]
    K = int(K)
    check_row_count(Xq=B, Y=N)
    _check_cats(item_cats, query_cats, B, N)
    _check_weights(item_weights, Y)
    wt = item_weights
    if (cand_indptr is None) != (cand_indices is None):
        raise ValueError(
            "cand_indptr and cand_indices must be given together")
    if cand_indptr is not None:
        fn = _topk_score_cands if Xq.is_cuda else topk_score_cands_ref
        return fn(Xq, Y, K, cand_indptr, cand_indices, item_mask,
                  ban_indptr, ban_indices, item_cats, query_cats,
                  item_weights=wt)
    if Xq.is_cuda:
        if mode is None:
            mode = os.environ.get("PIO_TOPK_MODE", "mfma")
        if mode == "union":
            if K < 1:
                raise ValueError("K must be >= 1")
            out = _topk_score_union(Xq, Y, K, item_mask, ban_indptr,
                                    ban_indices, n_slices, list_k,
                                    item_cats, query_cats, wt)
            if out is None:
                raise ValueError(
                    f"no union plan for B={B}, N={N}, rank={f}, K={K}")
            return out
        # the eager mfma route at every K <= 1024 is the union path when
        # the shape has a plan: many short per-slice lists stand in for
        # one long one, and its shortlist is the exact bf16 top 2K where
        # the list kernel's 64-entry LDS lists stop at 64. It syncs with
        # the host to read its flags, so not under stream capture
        if (mode == "mfma" and 1 <= K <= 1024
                and os.environ.get("PIO_TOPK_UNION", "1") != "0"
                and not torch.cuda.is_current_stream_capturing()):
            out = _topk_score_union(Xq, Y, K, item_mask, ban_indptr,
                                    ban_indices, n_slices, list_k,
                                    item_cats, query_cats, wt)
            if out is not None:
                return out
        if K > 64:
            # arbitrary `num` (the reference allows any): a materialized
            # masked matmul + torch.topk on device
            return _topk_torch_gpu(Xq, Y, K, item_mask, ban_indptr,
                                   ban_indices, item_cats, query_cats, wt)
        if mode == "mfma" and _mfma_rank(f) is not None:
            return _topk_score_mfma(Xq, Y, K, item_mask, ban_indptr,
                                    ban_indices, n_slices,
                                    item_cats, query_cats, wt)
        from predictionio_amd.ops import hip_ext
        pf = pad_rank(f)
        Xp = Xq if pf == f else torch.nn.functional.pad(Xq, (0, pf - f))
        Yp = Y if pf == f else torch.nn.functional.pad(Y, (0, pf - f))
        if n_slices is None:
            # enough (slice, ublock) workgroups to oversubscribe 256 CUs
            # (~2048 WGs); more slices only add insert + merge cost, so
            # scale them inversely with the user-block count
            ublocks = (B + 63) // 64
            n_slices = max(1, min(2048 // ublocks + 1,
                                  (N + 255) // 256))
        vals, idxs = hip_ext().topk_score(
            Xp.contiguous(), Yp.contiguous(), K, int(n_slices),
            item_mask.contiguous() if item_mask is not None else None,
            ban_indptr.contiguous() if ban_indptr is not None else None,
            ban_indices.contiguous() if ban_indices is not None else None, 0,
            item_cats=item_cats, query_cats=query_cats, item_weights=wt)
        # phase 2: merge per-slice candidates (small [B, n_slices*K] topk)
        mvals, pos = torch.topk(vals, K, dim=1)
        midx = torch.gather(idxs, 1, pos).long()
        # the kernel pads empty slots with -FLT_MAX (not -inf); normalize
        # to the CPU reference's -inf / -1 convention for exact parity
        empty = mvals <= torch.finfo(torch.float32).min
        midx[empty] = -1
        mvals = mvals.masked_fill(empty, float("-inf"))
        return mvals, midx
    return topk_score_ref(Xq, Y, K, item_mask, ban_indptr, ban_indices,
                          item_cats, query_cats, item_weights=wt)


def _check_weights(item_weights, Y: torch.Tensor) -> None:
    """The item_weights contract (the native binding re-validates it):
    contiguous fp32 [N] on the device of Y. A mismatch raises — there is
    no fallback. Values are not looked at (no per-call reduction)."""
    w = item_weights
    if w is None:
        return
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32:
        raise ValueError("item_weights must be an fp32 tensor")
    if w.dim() != 1 or w.shape[0] != Y.shape[0]:
        raise ValueError(f"item_weights must have shape [{Y.shape[0]}], "
                         f"got {list(w.shape)}")
    if not w.is_contiguous():
        raise ValueError("item_weights must be contiguous")
    if w.device != Y.device:
        raise ValueError("item_weights must be on the device of Y")


def _weighted(scores: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """scores * w as the kernels form it: plus 0.0, so a zero weight
    gives +0.0 whatever the sign of the raw score."""
    return scores * w + 0.0


def _check_cats(item_cats, query_cats, B: int, N: int) -> None:
    """The category-filter contract (the native binding re-validates
    it): both or neither, int32, contiguous, [N,W] / [B,W], W in
    {1,2,4}. A mismatch raises — there is no fallback."""
    if (item_cats is None) != (query_cats is None):
        raise ValueError("item_cats and query_cats must be given together")
    if item_cats is None:
        return
    for name, t, rows in (("item_cats", item_cats, N),
                          ("query_cats", query_cats, B)):
        if t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 2-D int32 tensor")
        if t.shape[0] != rows:
            raise ValueError(f"{name} must have {rows} rows, "
                             f"got {t.shape[0]}")
    W = item_cats.shape[1]
    if W not in (1, 2, 4) or query_cats.shape[1] != W:
        raise ValueError("category words W must be 1, 2 or 4 and equal "
                         "for item_cats and query_cats")


def _cats_miss(item_cats: torch.Tensor, query_cats: torch.Tensor
               ) -> torch.Tensor:
    """[B,N] bool, True where item j fails query b's category filter
    (word by word, so no B x N x W intermediate)."""
    hit = None
    for w in range(item_cats.shape[1]):
        h = (item_cats[:, w].unsqueeze(0)
             & query_cats[:, w].unsqueeze(1)) != 0
        hit = h if hit is None else (hit | h)
    return ~hit


def _topk_torch_gpu(Xq: torch.Tensor, Y: torch.Tensor, K: int,
                    item_mask, ban_indptr, ban_indices,
                    item_cats=None, query_cats=None, item_weights=None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device fallback for K above what the fused paths take (K > 1024,
    shapes without a union plan, flagged union queries): materialized
    masked score matrix + torch.topk. Memory: B x N fp32 — callers with
    huge B should batch."""
    scores = Xq @ Y.t()
    if item_weights is not None:  # before the filters write -inf
        scores = _weighted(scores, item_weights.unsqueeze(0))
    if item_cats is not None:
        scores = scores.masked_fill(_cats_miss(item_cats, query_cats),
                                    float("-inf"))
    if item_mask is not None:
        scores = scores.masked_fill(item_mask.bool().unsqueeze(0),
                                    float("-inf"))
    if ban_indptr is not None:
        ip = ban_indptr.tolist()
        for b in range(scores.shape[0]):
            banned = ban_indices[ip[b]:ip[b + 1]].long()
            if banned.numel():
                scores[b, banned] = float("-inf")
    Kc = min(K, scores.shape[1])
    vals, idxs = torch.topk(scores, Kc, dim=1)
    idxs = idxs.clone()
    idxs[vals == float("-inf")] = -1
    if Kc < K:
        B = scores.shape[0]
        vals = torch.cat(
            [vals, torch.full((B, K - Kc), float("-inf"),
                              device=vals.device)], 1)
        idxs = torch.cat(
            [idxs, torch.full((B, K - Kc), -1, dtype=idxs.dtype,
                              device=idxs.device)], 1)
    return vals, idxs


def _mfma_default_slices(B: int, N: int, pf: int, K: int, W: int,
                         wt: bool = False) -> int:
    """Item slices for the MFMA kernel: just enough to fill the chip
    ONCE. The resident-WG count depends on the kernel's LDS (64-item
    tile + the per-query top-K lists), so the target shrinks for large
    K — a 1536-WG grid at K=64 only fits 768 at a time and the second
    pass doubled the time (profiles/serve_k_sweep_r2.log). W = category
    words per item (0 = no filter); wt = item weights are staged."""
    ublocks = (B + 63) // 64
    if pf > 128:
        # tw_lds_bytes in csrc/topk_mfma_wide.hip: two 16 KB panel
        # buffers at every rank, category words and weights staged twice;
        # its registers allow 3 workgroups per CU (2 in some filtered or
        # weighted rank-512 instantiations, which is not modelled)
        lds = 2 * 64 * 256 + 8 * 64 * (K + 1) + 4 * 64
        if W:
            lds += 2 * W * (64 + (32 // W if W > 1 else 0)) * 4 + 64 * W * 4
        if wt:
            lds += 2 * 64 * 4
        target = 256 * max(1, min(3, (160 * 1024) // lds))
        return max(2, min(target // ublocks, (N + 255) // 256))
    # the kernel's dynamic LDS: tm_lds_bytes in csrc/topk_mfma.hip
    lds = 64 * 2 * pf + 8 * 64 * (K + 1) + 4 * 64
    if W:
        # staged item category words (rows padded by 32/W words for
        # W > 1) + the queries' accepted words
        lds += W * (64 + (32 // W if W > 1 else 0)) * 4 + 64 * W * 4
    if wt:
        lds += 64 * 4   # the staged weight row
    target = 256 * max(1, min(6, (160 * 1024) // lds))
    return max(2, min(target // ublocks, (N + 255) // 256))


_UNION_LISTS = (16, 20, 24, 32, 40, 48, 64)
_union_stats: Dict[str, int] = {"calls": 0, "queries": 0, "flagged": 0}


def union_stats() -> Dict[str, int]:
    """Cumulative counters of the union path since import: calls, queries
    served, and queries whose flag sent them to the fallback."""
    return dict(_union_stats)


def _union_rule(L: int, S: int, M: int) -> bool:
    """A slice expects mu = M / S of a query's top M (interleaved slices
    make membership near-uniform). A FULL list flags its query whether or
    not it dropped anything, so the tail that matters is P(X >= L):
    L - 1 >= mu + 6 sqrt(mu) puts it below 1e-6 per slice (Poisson)."""
    mu = M / S
    return S * L >= M and L - 1 >= mu + 6.0 * math.sqrt(mu)


def _union_min_slices(L: int, M: int) -> int:
    """Smallest S that passes _union_rule for list length L."""
    mu_max = (math.sqrt(8 + L) - 3.0) ** 2   # mu + 6 sqrt(mu) = L - 1
    S = max(1, math.ceil(M / mu_max))
    while not _union_rule(L, S, M):          # guard the float boundary
        S += 1
    return S


def _union_plan(B: int, N: int, pf: int, K: int, W: int,
                list_k: Optional[int] = None,
                n_slices: Optional[int] = None, wt: bool = False
                ) -> Optional[Tuple[int, int]]:
    """(L, S) for the union path: per-slice list length L <= 64 and slice
    count S, or None when the shape admits none (tiny N).

    The SHORTEST list in _UNION_LISTS wins, with as many slices as it
    takes: S = max(chip-filling count, smallest S passing _union_rule),
    as long as S <= ceil(N / 64) (a slice needs a chunk). The sweep in
    NOTES.md decided this: at equal S a shorter list is always faster
    (the insert scan is O(L) and list LDS costs occupancy), and trading
    list length for slices beyond one chip-filling wave still pays — at
    B = 4096, K = 1024, (16, 512) runs in 84 ms against 331 ms for
    (64, 67). 2 <= S <= ceil(N / 64) and S * L >= 2K always hold.
    list_k / n_slices pin either half; a pinned pair is only
    range-checked."""
    M = 2 * K
    nch = (N + 63) // 64
    if nch < 2:
        return None
    if list_k is not None and not 1 <= list_k <= 64:
        raise ValueError("list_k must be in [1, 64]")
    if n_slices is not None:
        if n_slices < 1:
            raise ValueError("n_slices must be >= 1")
        n_slices = max(2, min(int(n_slices), nch))
    if list_k is not None and n_slices is not None:
        return (int(list_k), n_slices) if n_slices * list_k >= M else None
    for L in (_UNION_LISTS if list_k is None else (int(list_k),)):
        if n_slices is not None:
            if _union_rule(L, n_slices, M):
                return L, n_slices
            continue
        S = max(2, _mfma_default_slices(B, N, pf, L, W, wt),
                _union_min_slices(L, M))
        if S <= nch:
            return L, S
    return None


def _union_merge(vals: torch.Tensor, idxs: torch.Tensor, L: int, S: int,
                 M: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Top M of a query's S per-slice lists of length L, and the exact
    test of whether that is the top M of all items.

    vals / idxs [B, S*L]: slice-major candidate groups as the kernel
    writes them, empty slots at -FLT_MAX / -1. Returns (short_idx [B,C]
    int64, short_val [B,C], flagged [B] bool) with C = min(M, S*L);
    invalid shortlist slots carry -1 / -inf.

    A slice can only have dropped an item that belongs in the top M if
    its list is full and even its smallest entry beats v_M, the M-th
    best valid candidate of the union (-inf when fewer than M are
    valid). Such a query is flagged; every other query's shortlist is
    exactly the top M of the scores the lists were built from."""
    B = vals.shape[0]
    fmin = torch.finfo(torch.float32).min
    C = min(M, S * L)
    cv, pos = torch.topk(vals, C, dim=1)
    ok = cv > fmin
    short_idx = torch.gather(idxs, 1, pos).long().masked_fill(~ok, -1)
    short_val = cv.masked_fill(~ok, float("-inf"))
    if C == M:
        v_m = short_val[:, M - 1]
    else:
        v_m = torch.full((B,), float("-inf"), device=vals.device)
    smin = vals.view(B, S, L).min(dim=2).values   # > fmin iff list full
    flagged = ((smin > fmin) & (smin > v_m.unsqueeze(1))).any(dim=1)
    return short_idx, short_val, flagged


def _select_csr(indptr: torch.Tensor, indices: torch.Tensor,
                rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The CSR (indptr, indices) restricted to `rows`, in that order."""
    starts = indptr[rows]
    lens = indptr[rows + 1] - starts
    out_ptr = torch.zeros(rows.numel() + 1, dtype=indptr.dtype,
                          device=indptr.device)
    out_ptr[1:] = torch.cumsum(lens, 0)
    total = int(out_ptr[-1])
    src = (torch.repeat_interleave(starts - out_ptr[:-1], lens)
           + torch.arange(total, device=indptr.device))
    return out_ptr, indices[src]


def _topk_score_union(Xq: torch.Tensor, Y: torch.Tensor, K: int,
                      item_mask, ban_indptr, ban_indices,
                      n_slices: Optional[int], list_k: Optional[int],
                      item_cats=None, query_cats=None, item_weights=None
                      ) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """Union path, the eager route at every K <= 1024: ONE MFMA launch
    (topk_mfma_kernel, or topk_mfma_wide_kernel for ranks above 128)
    with short lists (L <= 64, the kernel's tuned regime) over S slices
    interleaved at chunk granularity, cross-slice threshold off; the
    S*L candidates are merged to the bf16 top M = 2K, re-scored exactly
    in fp32 by topk_rescore, and the top K of those returned. The flag
    test is exact, so the shortlist depth is D = 2K at any K. Queries
    that _union_merge flags (some slice may have dropped a top-M item)
    are recomputed by _topk_torch_gpu. None = no plan for this shape."""
    from predictionio_amd.ops import hip_ext
    B, f = Xq.shape
    N = Y.shape[0]
    check_row_count(Xq=B, Y=N)
    pf = _mfma_rank(f)
    if pf is None or B == 0:
        return None
    W = item_cats.shape[1] if item_cats is not None else 0
    plan = _union_plan(B, N, pf, K, W, list_k, n_slices,
                       item_weights is not None)
    if plan is None:
        return None
    L, S = plan
    M = 2 * K
    ext = hip_ext()
    Xp = Xq if pf == f else torch.nn.functional.pad(Xq, (0, pf - f))
    # ranks above 128: the rank-panel kernel, same arguments and output
    launch = ext.topk_score_mfma_wide if pf > 128 else ext.topk_score_mfma
    vals, idxs = launch(
        Xp.to(torch.bfloat16).contiguous(), bf16_copy(Y, pf), L, S,
        item_mask.contiguous() if item_mask is not None else None,
        ban_indptr.contiguous() if ban_indptr is not None else None,
        ban_indices.contiguous() if ban_indices is not None else None, 0,
        item_cats=item_cats, query_cats=query_cats,
        interleave=True, gth=False, item_weights=item_weights)
    short_idx, _, flagged = _union_merge(vals, idxs, L, S, M)
    exact = topk_rescore(Xq, Y, short_idx.to(torch.int32), item_weights)
    mv, p2 = torch.topk(exact, min(K, exact.shape[1]), dim=1)
    midx = torch.gather(short_idx, 1, p2)
    midx[mv == float("-inf")] = -1
    if mv.shape[1] < K:  # pad like the reference
        pad = K - mv.shape[1]
        mv = torch.cat([mv, torch.full((B, pad), float("-inf"),
                                       device=mv.device)], 1)
        midx = torch.cat([midx, torch.full((B, pad), -1, dtype=midx.dtype,
                                           device=midx.device)], 1)
    rows = flagged.nonzero().flatten()
    nf = rows.numel()
    _union_stats["calls"] += 1
    _union_stats["queries"] += B
    _union_stats["flagged"] += nf
    if nf:
        if nf * 100 > B:
            log.warning(
                "top-K union path: %d of %d queries flagged (K=%d, L=%d, "
                "S=%d) and recomputed by the materialized fallback", nf, B,
                K, L, S)
        blk = max(1, 2 ** 28 // N)  # <= 1 GiB of fp32 scores per block
        for r0 in range(0, nf, blk):
            r = rows[r0:r0 + blk]
            bp = bi = None
            if ban_indptr is not None:
                bp, bi = _select_csr(ban_indptr, ban_indices, r)
            fv, fi = _topk_torch_gpu(
                Xq[r], Y, K, item_mask, bp, bi, item_cats,
                query_cats[r] if query_cats is not None else None,
                item_weights)
            mv[r] = fv
            midx[r] = fi
    return mv, midx


def topk_rescore(Xq: torch.Tensor, Y: torch.Tensor, idx: torch.Tensor,
                 item_weights: Optional[torch.Tensor] = None
                 ) -> torch.Tensor:
    """out[b, c] = Xq[b] . Y[idx[b, c]] in fp32 on the GPU
    (csrc/topk_rescore.hip), times item_weights[idx[b, c]] when weights
    are given; -inf where idx < 0. idx [B, C] int32; Xq and Y are read
    where they lie."""
    check_row_count(Xq=Xq.shape[0], Y=Y.shape[0])
    _check_weights(item_weights, Y)
    from predictionio_amd.ops import hip_ext
    return hip_ext().topk_rescore(Xq.contiguous(), Y.contiguous(), idx,
                                  item_weights=item_weights)


def _topk_score_mfma(Xq: torch.Tensor, Y: torch.Tensor, K: int,
                     item_mask, ban_indptr, ban_indices,
                     n_slices: Optional[int],
                     item_cats=None, query_cats=None, item_weights=None
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """List-kernel MFMA path (capture-safe, any N): bf16 matrix-core
    scoring keeps a list of D = min(2K, 64) per item slice per query
    (masks/bans/categories applied in-kernel, so filtered items take no
    depth); the union of the lists holds the query's bf16 top D whatever
    the slicing and whether or not the cross-slice threshold is on (it
    prunes to the top D overall). The best 2K of them are re-scored
    against the fp32 factors and the final top-K taken on those values.

    Contract: an item of the fp32 top K is served if it is also in the
    bf16 top D among the valid items. bf16 rounding perturbs scores by
    ~0.4% relative, which on clustered factors moves items across the K
    cut in most queries but hardly ever past 2K. For 32 < K <= 64 the
    64-entry list cap leaves D = 64 < 2K here; the union path
    (_topk_score_union) delivers D = 2K at every K."""
    from predictionio_amd.ops import hip_ext
    B, f = Xq.shape
    N = Y.shape[0]
    check_row_count(Xq=B, Y=N)
    pf = _mfma_rank(f)
    Xp = Xq if pf == f else torch.nn.functional.pad(Xq, (0, pf - f))
    # the per-slice list length IS the shortlist depth: with a list of K
    # a slice holding the bf16 top K + 1 drops the (K+1)-th, and the
    # cross-slice threshold prunes the other slices to the top K too
    depth = min(2 * K, 64)
    if n_slices is None:
        W = item_cats.shape[1] if item_cats is not None else 0
        n_slices = _mfma_default_slices(B, N, pf, depth, W,
                                        item_weights is not None)
    # Y's bf16 copy is cached (factors are static across serving batches);
    # Xq is cast per call — it changes every batch, and under hipGraph
    # capture (GraphedTopK) the cast must be part of the captured work
    ext = hip_ext()
    launch = ext.topk_score_mfma_wide if pf > 128 else ext.topk_score_mfma
    vals, idxs = launch(
        Xp.to(torch.bfloat16).contiguous(), bf16_copy(Y, pf), depth,
        int(n_slices),
        item_mask.contiguous() if item_mask is not None else None,
        ban_indptr.contiguous() if ban_indptr is not None else None,
        ban_indices.contiguous() if ban_indices is not None else None, 0,
        item_cats=item_cats, query_cats=query_cats,
        item_weights=item_weights)
    # merge candidate groups down to a 2K shortlist on the bf16 scores
    C = min(vals.shape[1], 2 * K)
    cv, pos = torch.topk(vals, C, dim=1)
    cidx = torch.gather(idxs, 1, pos).long()
    valid = cv > torch.finfo(torch.float32).min
    # exact fp32 re-score of the shortlist (tiny gather + batched dot)
    Yc = Y[cidx.clamp_min(0)]                      # B x C x f fp32
    exact = torch.einsum("bf,bcf->bc", Xq, Yc)
    if item_weights is not None:
        exact = _weighted(exact, item_weights[cidx.clamp_min(0)])
    exact = exact.masked_fill(~valid, float("-inf"))
    mv, p2 = torch.topk(exact, min(K, C), dim=1)
    midx = torch.gather(cidx, 1, p2)
    midx[mv == float("-inf")] = -1
    if mv.shape[1] < K:  # degenerate tiny-N case: pad like the reference
        pad = K - mv.shape[1]
        mv = torch.cat([mv, torch.full((B, pad), float("-inf"),
                                       device=mv.device)], 1)
        midx = torch.cat([midx, torch.full((B, pad), -1, dtype=midx.dtype,
                                           device=midx.device)], 1)
    return mv, midx


_cand_stats: Dict[str, int] = {"calls": 0, "queries": 0, "segments": 0}


def cand_stats() -> Dict[str, int]:
    """Cumulative counters of the candidate-list path since import:
    calls, queries served, and segments launched."""
    return dict(_cand_stats)


def _check_cands(cand_indptr: torch.Tensor, cand_indices: torch.Tensor,
                 B: int, N: int, seg_len: int, wave_max: int):
    """The candidate-CSR contract, checked on the tensors' device with one
    transfer to the host: cand_indptr [B+1] int64 runs from 0 to nnz
    without decreasing; cand_indices int32 holds ids in [0, N), strictly
    ascending inside every query. An out-of-range id would be an
    out-of-bounds gather and a repeated one breaks the selection's
    distinct-key premise, so each raises ValueError. Returns (lens [B],
    segments, segments longer than wave_max, most segments of a query)
    for lists cut every seg_len candidates."""
    ip, ci = cand_indptr, cand_indices
    if ip.dtype != torch.int64 or ip.dim() != 1 or ip.numel() != B + 1:
        raise ValueError("cand_indptr must be a 1-D int64 tensor of B + 1")
    if ci.dtype != torch.int32 or ci.dim() != 1:
        raise ValueError("cand_indices must be a 1-D int32 tensor")
    if ip.device != ci.device:
        raise ValueError("cand_indptr and cand_indices must share a device")
    nnz = ci.numel()
    lens = ip[1:] - ip[:-1]
    is_start = torch.zeros(nnz + 1, dtype=torch.bool, device=ci.device)
    is_start[ip.clamp(0, nnz)] = True
    full, rem = lens.clamp_min(0) // seg_len, lens.clamp_min(0) % seg_len
    nseg_q = full + (rem > 0)
    zero = torch.zeros((), dtype=torch.int64, device=ci.device)
    bad_ptr, bad_len, bad_id, bad_order, n_seg, n_long, max_seg = \
        torch.stack([
            (ip[0] != 0) | (ip[-1] != nnz),
            (lens < 0).any(),
            ((ci < 0) | (ci >= N)).any(),
            ((ci[1:] <= ci[:-1]) & ~is_start[1:nnz]).any(),
            nseg_q.sum(),
            (full * int(seg_len > wave_max) + (rem > wave_max)).sum(),
            nseg_q.max() if B else zero,
        ]).tolist()
    if bad_ptr:
        raise ValueError("cand_indptr must run from 0 to len(cand_indices)")
    if bad_len:
        raise ValueError("cand_indptr must not decrease")
    if bad_id:
        raise ValueError(f"cand_indices holds an id outside [0, {N})")
    if bad_order:
        raise ValueError("cand_indices must be strictly ascending inside "
                         "every query (sorted, no duplicates)")
    return lens, n_seg, n_long, max_seg


def _cand_order_key(score: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """int64 keys whose descending order is score descending, then id
    ascending: the kernel's (ord(score) << 32) | (0xFFFFFFFF - id) with
    ord shifted by 2^31 into the signed range. Empty slots (id -1) are
    keyed as id 0; their -inf score puts them last anyway."""
    u = score.contiguous().view(torch.int32).long()
    o = torch.where(u >= 0, u, -u - 1 - 2 ** 31)
    return (o << 32) | (0xFFFFFFFF - ids.long().clamp_min(0))


def _cand_select(qid: torch.Tensor, score: torch.Tensor, ids: torch.Tensor,
                 B: int, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The K best (score, id) pairs of every query from flat pairs tagged
    with their query: two sorts (key descending, then query, stable) and
    a scatter by rank. O(pairs) memory; -inf scores become -inf / -1."""
    dev = score.device
    n = score.numel()
    o1 = torch.argsort(_cand_order_key(score, ids), descending=True)
    perm = o1[torch.argsort(qid[o1], stable=True)]
    qs = qid[perm]
    counts = torch.bincount(qid, minlength=B)
    rank = torch.arange(n, device=dev) - (torch.cumsum(counts, 0)
                                          - counts)[qs]
    slot = torch.where(rank < K, qs * K + rank, B * K)  # B * K: dropped
    vals = torch.full((B * K + 1,), float("-inf"), device=dev)
    idx = torch.full((B * K + 1,), -1, dtype=torch.int64, device=dev)
    vals[slot] = score[perm]
    idx[slot] = ids[perm].long()
    vals, idx = vals[:-1].view(B, K), idx[:-1].view(B, K)
    idx[vals == float("-inf")] = -1
    return vals, idx


def _topk_score_cands(Xq: torch.Tensor, Y: torch.Tensor, K: int,
                      cand_indptr: torch.Tensor, cand_indices: torch.Tensor,
                      item_mask=None, ban_indptr=None, ban_indices=None,
                      item_cats=None, query_cats=None,
                      seg_len: int = 8192, wave_max: int = 256,
                      item_weights=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Candidate-list top-K on the GPU (csrc/topk_cand.hip): every query
    ranks its own CSR list, reading only the listed rows of Y. Exact
    fp32; order score descending, id ascending. Xq and Y are read where
    they lie (contiguous fp32, any rank 1..128) — no padding, no copy.

    Lists longer than seg_len are cut into segments of at most seg_len
    candidates so that one huge list (or B = 1) still fills the chip;
    segments of at most wave_max candidates run in the one-wave
    instantiation, longer ones in the 256-thread one. A query with
    several segments has its segments * K pairs merged by _cand_select,
    which equals the unsegmented result because a candidate's score does
    not depend on its segment. K > 64 runs the kernel's scores mode
    (every candidate's score into an [nnz] buffer) and the same
    device-side sort: O(nnz) memory. Syncs with the host once (the
    checks), so not under stream capture."""
    from predictionio_amd.ops import hip_ext
    B, f = Xq.shape
    N = Y.shape[0]
    check_row_count(Xq=B, Y=N)
    if K < 1:
        raise ValueError("K must be >= 1")
    if seg_len < 1 or wave_max < 0:
        raise ValueError("seg_len must be >= 1 and wave_max >= 0")
    for name, t in (("Xq", Xq), ("Y", Y)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous fp32: the candidate"
                             " kernel reads it where it lies")
    if not 1 <= f <= 128 or Y.shape[1] != f:
        raise ValueError("rank must be in [1, 128] and equal for Xq and Y")
    lens, n_seg, n_long, max_seg = _check_cands(
        cand_indptr, cand_indices, B, N, seg_len, wave_max)
    _cand_stats["calls"] += 1
    _cand_stats["queries"] += B
    _cand_stats["segments"] += n_seg
    dev = Xq.device
    if n_seg == 0:
        return (torch.full((B, K), float("-inf"), device=dev),
                torch.full((B, K), -1, dtype=torch.int64, device=dev))
    # the work list: (query, lo, hi), heaviest first
    full, rem = lens // seg_len, lens % seg_len
    nseg_q = full + (rem > 0)
    seg_q = torch.repeat_interleave(torch.arange(B, device=dev), nseg_q,
                                    output_size=n_seg)
    k = (torch.arange(n_seg, device=dev)
         - (torch.cumsum(nseg_q, 0) - nseg_q)[seg_q])
    lo = cand_indptr[seg_q] + k * seg_len
    hi = torch.minimum(lo + seg_len, cand_indptr[seg_q + 1])
    order = torch.argsort(hi - lo, descending=True, stable=True)
    segs = torch.stack([seg_q, lo, hi], 1)[order].contiguous()
    kw = dict(
        item_mask=item_mask.contiguous() if item_mask is not None else None,
        ban_indptr=ban_indptr.contiguous() if ban_indptr is not None
        else None,
        ban_indices=ban_indices.contiguous() if ban_indices is not None
        else None,
        item_cats=item_cats, query_cats=query_cats,
        item_weights=item_weights)
    ext = hip_ext()
    ci = cand_indices.contiguous()
    if K > 64:
        scores = torch.empty(ci.numel(), dtype=torch.float32, device=dev)
        ext.topk_cand(Xq, Y, ci, segs, 0, 256, scores=scores, **kw)
        qid = torch.repeat_interleave(torch.arange(B, device=dev), lens,
                                      output_size=ci.numel())
        return _cand_select(qid, scores, ci, B, K)
    parts = []
    if n_long:
        parts.append(ext.topk_cand(Xq, Y, ci, segs[:n_long], K, 256, **kw))
    if n_seg > n_long:
        parts.append(ext.topk_cand(Xq, Y, ci, segs[n_long:], K, 64, **kw))
    sv = torch.cat([p[0] for p in parts])
    si = torch.cat([p[1] for p in parts])
    sq = segs[:, 0]
    if max_seg > 1:
        return _cand_select(sq.repeat_interleave(K), sv.flatten(),
                            si.flatten(), B, K)
    vals = torch.full((B, K), float("-inf"), device=dev)
    idx = torch.full((B, K), -1, dtype=torch.int64, device=dev)
    vals[sq] = sv
    idx[sq] = si.long()
    return vals, idx


def topk_score_cands_ref(Xq, Y, K, cand_indptr, cand_indices,
                         item_mask=None, ban_indptr=None, ban_indices=None,
                         item_cats=None, query_cats=None, item_weights=None
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pure-torch candidate-list top-K (CPU path + GPU numerics
    baseline): gather the candidate rows, score, filter, and order by
    score descending then id ascending. O(nnz * f) memory."""
    B, N = Xq.shape[0], Y.shape[0]
    K = int(K)
    check_row_count(Xq=B, Y=N)
    if K < 1:
        raise ValueError("K must be >= 1")
    _check_cats(item_cats, query_cats, B, N)
    _check_weights(item_weights, Y)
    lens, _, _, _ = _check_cands(cand_indptr, cand_indices, B, N,
                                 1 << 62, 1 << 62)
    dev = Xq.device
    qid = torch.repeat_interleave(torch.arange(B, device=dev), lens)
    j = cand_indices.long()
    score = (Xq.float()[qid] * Y.float()[j]).sum(dim=1)
    if item_weights is not None:
        score = _weighted(score, item_weights[j])
    ok = torch.ones_like(j, dtype=torch.bool)
    if item_mask is not None:
        ok &= ~item_mask.bool()[j]
    if item_cats is not None:
        ok &= ((item_cats[j] & query_cats[qid]) != 0).any(dim=1)
    if ban_indptr is not None:
        bq = torch.repeat_interleave(torch.arange(B, device=dev),
                                     ban_indptr[1:] - ban_indptr[:-1])
        ok &= ~torch.isin(qid * N + j, bq * N + ban_indices.long())
    score = score.masked_fill(~ok, float("-inf"))
    return _cand_select(qid, score, cand_indices, B, K)


def topk_score_ref(Xq, Y, K, item_mask=None, ban_indptr=None,
                   ban_indices=None, item_cats=None, query_cats=None,
                   cand_indptr=None, cand_indices=None, item_weights=None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pure-torch reference (CPU path + GPU numerics baseline)."""
    check_row_count(Xq=Xq.shape[0], Y=Y.shape[0])
    if (cand_indptr is None) != (cand_indices is None):
        raise ValueError(
            "cand_indptr and cand_indices must be given together")
    if cand_indptr is not None:
        return topk_score_cands_ref(Xq, Y, K, cand_indptr, cand_indices,
                                    item_mask, ban_indptr, ban_indices,
                                    item_cats, query_cats, item_weights)
    _check_cats(item_cats, query_cats, Xq.shape[0], Y.shape[0])
    _check_weights(item_weights, Y)
    scores = Xq.float() @ Y.float().t()  # B x N
    if item_weights is not None:  # before the filters write -inf
        scores = _weighted(scores, item_weights.unsqueeze(0))
    if item_cats is not None:
        scores = scores.masked_fill(_cats_miss(item_cats, query_cats),
                                    float("-inf"))
    if item_mask is not None:
        scores = scores.masked_fill(item_mask.bool().unsqueeze(0),
                                    float("-inf"))
    if ban_indptr is not None:
        ip = ban_indptr.tolist()
        for b in range(scores.shape[0]):
            banned = ban_indices[ip[b]:ip[b + 1]].long()
            if banned.numel():
                scores[b, banned] = float("-inf")
    Kc = min(K, scores.shape[1])
    vals, idxs = torch.topk(scores, Kc, dim=1)
    idxs = idxs.clone()
    idxs[vals == float("-inf")] = -1
    if Kc < K:  # pad to K like the GPU kernel (empty slots = -inf / -1)
        B = scores.shape[0]
        vals = torch.cat([vals, torch.full((B, K - Kc), float("-inf"))], 1)
        idxs = torch.cat([idxs, torch.full((B, K - Kc), -1,
                                           dtype=idxs.dtype)], 1)
    return vals, idxs


def cosine_topk(query_vec: torch.Tensor, Y_normed: torch.Tensor, K: int,
                **kw) -> Tuple[torch.Tensor, torch.Tensor]:
    """Item-item cosine kNN (K4): score(j) = sum_q cos(y_q, y_j) collapses
    to a single dot with the summed normalized query vector, so it reuses
    the top-K scoring kernel (reference computes a scalar cosine loop per
    item, similarproduct ALSAlgorithm.scala:228-242)."""
    q = query_vec.reshape(1, -1) if query_vec.dim() == 1 else query_vec
    return topk_score(q, Y_normed, K, **kw)


def normalize_rows(Y: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    return Y / Y.norm(dim=1, keepdim=True).clamp_min(eps)
