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

from predictionio_amd.ops.als import pad_rank

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
    """Padded rank for the MFMA kernel (K-dim multiples of 32), or None
    when unsupported."""
    for s in (32, 64, 128):
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
               list_k: Optional[int] = None
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

    Eager "mfma" calls with K <= 1024 take the union path
    (_topk_score_union) when the shape has a plan for it: short
    per-slice lists over interleaved slices, merged to the exact bf16
    top 2K (D = 2K). Otherwise K <= 64 runs the list kernel
    (_topk_score_mfma) with D = min(2K, 64): shapes without a plan
    (N <= 64 among them), calls under stream capture (the union path
    syncs with the host) and PIO_TOPK_UNION=0. mode="union" forces the
    union path at any K >= 1 (ValueError when the shape admits no plan);
    list_k with n_slices pins its plan. K > 64 without the union path,
    and any K > 1024, use the materialized fallback, which is exact."""
    B, f = Xq.shape
    N = Y.shape[0]
    K = int(K)
    _check_cats(item_cats, query_cats, B, N)
    if Xq.is_cuda:
        if mode is None:
            mode = os.environ.get("PIO_TOPK_MODE", "mfma")
        if mode == "union":
            if K < 1:
                raise ValueError("K must be >= 1")
            out = _topk_score_union(Xq, Y, K, item_mask, ban_indptr,
                                    ban_indices, n_slices, list_k,
                                    item_cats, query_cats)
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
                                    item_cats, query_cats)
            if out is not None:
                return out
        if K > 64:
            # arbitrary `num` (the reference allows any): a materialized
            # masked matmul + torch.topk on device
            return _topk_torch_gpu(Xq, Y, K, item_mask, ban_indptr,
                                   ban_indices, item_cats, query_cats)
        if mode == "mfma" and _mfma_rank(f) is not None:
            return _topk_score_mfma(Xq, Y, K, item_mask, ban_indptr,
                                    ban_indices, n_slices,
                                    item_cats, query_cats)
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
            item_cats=item_cats, query_cats=query_cats)
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
                          item_cats, query_cats)


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
                    item_cats=None, query_cats=None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device fallback for K above what the fused paths take (K > 1024,
    shapes without a union plan, flagged union queries): materialized
    masked score matrix + torch.topk. Memory: B x N fp32 — callers with
    huge B should batch."""
    scores = Xq @ Y.t()
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


def _mfma_default_slices(B: int, N: int, pf: int, K: int, W: int) -> int:
    """Item slices for the MFMA kernel: just enough to fill the chip
    ONCE. The resident-WG count depends on the kernel's LDS (64-item
    tile + the per-query top-K lists), so the target shrinks for large
    K — a 1536-WG grid at K=64 only fits 768 at a time and the second
    pass doubled the time (profiles/serve_k_sweep_r2.log). W = category
    words per item (0 = no filter)."""
    ublocks = (B + 63) // 64
    # the kernel's dynamic LDS: tm_lds_bytes in csrc/topk_mfma.hip
    lds = 64 * 2 * pf + 8 * 64 * (K + 1) + 4 * 64
    if W:
        # staged item category words (rows padded by 32/W words for
        # W > 1) + the queries' accepted words
        lds += W * (64 + (32 // W if W > 1 else 0)) * 4 + 64 * W * 4
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
                n_slices: Optional[int] = None
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
        S = max(2, _mfma_default_slices(B, N, pf, L, W),
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
                      item_cats=None, query_cats=None
                      ) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """Union path, the eager route at every K <= 1024: ONE MFMA launch
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
    pf = _mfma_rank(f)
    if pf is None or B == 0:
        return None
    W = item_cats.shape[1] if item_cats is not None else 0
    plan = _union_plan(B, N, pf, K, W, list_k, n_slices)
    if plan is None:
        return None
    L, S = plan
    M = 2 * K
    ext = hip_ext()
    Xp = Xq if pf == f else torch.nn.functional.pad(Xq, (0, pf - f))
    vals, idxs = ext.topk_score_mfma(
        Xp.to(torch.bfloat16).contiguous(), bf16_copy(Y, pf), L, S,
        item_mask.contiguous() if item_mask is not None else None,
        ban_indptr.contiguous() if ban_indptr is not None else None,
        ban_indices.contiguous() if ban_indices is not None else None, 0,
        item_cats=item_cats, query_cats=query_cats,
        interleave=True, gth=False)
    short_idx, _, flagged = _union_merge(vals, idxs, L, S, M)
    exact = ext.topk_rescore(Xq.contiguous(), Y.contiguous(),
                             short_idx.to(torch.int32))
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
                query_cats[r] if query_cats is not None else None)
            mv[r] = fv
            midx[r] = fi
    return mv, midx


def _topk_score_mfma(Xq: torch.Tensor, Y: torch.Tensor, K: int,
                     item_mask, ban_indptr, ban_indices,
                     n_slices: Optional[int],
                     item_cats=None, query_cats=None
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
    pf = _mfma_rank(f)
    Xp = Xq if pf == f else torch.nn.functional.pad(Xq, (0, pf - f))
    # the per-slice list length IS the shortlist depth: with a list of K
    # a slice holding the bf16 top K + 1 drops the (K+1)-th, and the
    # cross-slice threshold prunes the other slices to the top K too
    depth = min(2 * K, 64)
    if n_slices is None:
        W = item_cats.shape[1] if item_cats is not None else 0
        n_slices = _mfma_default_slices(B, N, pf, depth, W)
    # Y's bf16 copy is cached (factors are static across serving batches);
    # Xq is cast per call — it changes every batch, and under hipGraph
    # capture (GraphedTopK) the cast must be part of the captured work
    vals, idxs = hip_ext().topk_score_mfma(
        Xp.to(torch.bfloat16).contiguous(), bf16_copy(Y, pf), depth,
        int(n_slices),
        item_mask.contiguous() if item_mask is not None else None,
        ban_indptr.contiguous() if ban_indptr is not None else None,
        ban_indices.contiguous() if ban_indices is not None else None, 0,
        item_cats=item_cats, query_cats=query_cats)
    # merge candidate groups down to a 2K shortlist on the bf16 scores
    C = min(vals.shape[1], 2 * K)
    cv, pos = torch.topk(vals, C, dim=1)
    cidx = torch.gather(idxs, 1, pos).long()
    valid = cv > torch.finfo(torch.float32).min
    # exact fp32 re-score of the shortlist (tiny gather + batched dot)
    Yc = Y[cidx.clamp_min(0)]                      # B x C x f fp32
    exact = torch.einsum("bf,bcf->bc", Xq, Yc)
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


def topk_score_ref(Xq, Y, K, item_mask=None, ban_indptr=None,
                   ban_indices=None, item_cats=None, query_cats=None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pure-torch reference (CPU path + GPU numerics baseline)."""
    _check_cats(item_cats, query_cats, Xq.shape[0], Y.shape[0])
    scores = Xq.float() @ Y.float().t()  # B x N
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
