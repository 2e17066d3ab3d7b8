"""Co-occurrence top-N: for every item the n items most often viewed by
the same users.

    c[i][j] = |users(i) ∩ users(j)|,  i != j

Row i of the result holds the n items j with the largest c[i][j] > 0,
ordered by count descending, then item id ascending — the descending
order of the u64 key (count << 32) | (0xFFFFFFFF - j). Unused slots are
id -1, count 0. Everything is integer: results are exact.

On a GPU the rows are counted on chip by csrc/cooc_topn.hip, routed per
row by a bound on its distinct neighbours (cooccurrence_plan); device
memory is O(nnz + N n + a fixed counter pool) and no pair data goes
through the host. On CPU tensors cooccurrence_topn_ref (torch.sparse.mm
plus a vectorised top-n) is the implementation; it materialises the
item x item product and is what the GPU tests compare against.

Cross-occurrence and LLR. cross_occurrence_topn takes two deduplicated
pair sets over the same U = n_users users, A over Na row items and B
over Nb column items ("viewed this, bought ..."). For a row item i and
a column item j

    k11 = |usersA(i) ∩ usersB(j)|    Ai = |usersA(i)|   Bj = |usersB(j)|
    k12 = Ai - k11    k21 = Bj - k11    k22 = U - Ai - Bj + k11
    xlx(x) = x ln x,  xlx(0) = 0

    llr = max(0, 2 (xlx(U) - xlx(Ai) - xlx(U - Ai) - xlx(Bj) - xlx(U - Bj)
                    + xlx(k11) + xlx(k12) + xlx(k21) + xlx(k22)))

which is Mahout's LogLikelihood.logLikelihoodRatio (row entropy + column
entropy - matrix entropy, clamped at 0) with the terms separated into a
per-row part R_i = xlx(U) - xlx(Ai) - xlx(U - Ai), a per-column part
H_j = xlx(Bj) + xlx(U - Bj) and four per-pair terms. A pair that is
merely popular scores near 0. Candidates of row i are the j with
k11 > 0 and, with exclude_self (needs Na == Nb), j != i. score="count"
ranks them by k11 as above; score="llr" by llr: row i holds the n
candidates with the largest score, score descending and id ascending on
equal fp32 scores, the descending order of
(bits(float(llr)) << 32) | (0xFFFFFFFF - j) (llr >= 0, so the raw fp32
bits are order-preserving; the key is never 0 and distinct per j).
Unused slots are id -1, score 0. The sum is formed in fp64 and rounded
to fp32 once: the terms reach U ln U (1.4e7 at a million users) and
cancel down to order 1, fp32 would keep no digits.

Serving. indicator_topk (at the end of this module) answers a batch of
queries from the [N, n] table these ops return: it sums the rows of each
query's items, filters and ranks, on a GPU in csrc/indicator_topk.hip.
"""

from __future__ import annotations

import os
import warnings

import torch

# largest distinct-neighbour bound each LDS hash table accepts: 3/4 of
# its 1024 / 8192 slots, so an insert always finds an empty one
HASH_CAPS = (768, 6144)
# u64 keys in the kernels' selection buffer
SELECT_BUF = 1024
# dense counters live in LDS (not the global pool) up to this many items
DENSE_LDS_MAX = 28672
N_MAX = 64

_DEFAULT_POOL_MB = 1024


def _default_pool_bytes() -> int:
    return int(os.environ.get("PIO_COOC_POOL_MB", _DEFAULT_POOL_MB)) << 20


def _check_n(n: int) -> int:
    n = int(n)
    if not 1 <= n <= N_MAX:
        raise ValueError(f"n must be in [1, {N_MAX}], got {n}")
    return n


def build_csrs(users, items, n_users: int, n_items: int):
    """Dedup the (user, item) pairs on u * N + i and return the
    user-major and item-major CSRs (u_indptr, u_items, i_indptr,
    i_users): i64 indptr, i32 indices, columns sorted."""
    n_users, n_items = int(n_users), int(n_items)
    if n_users >= 2 ** 31 or n_items >= 2 ** 31:
        raise ValueError("user and item counts must be below 2^31")
    u = users.to(torch.int64).reshape(-1)
    i = items.to(torch.int64).reshape(-1)
    if u.numel() != i.numel():
        raise ValueError("users and items must have the same length")
    if u.numel():
        if int(u.min()) < 0 or int(u.max()) >= n_users:
            raise ValueError(f"user id out of range [0, {n_users})")
        if int(i.min()) < 0 or int(i.max()) >= n_items:
            raise ValueError(f"item id out of range [0, {n_items})")
    key = torch.unique(u * n_items + i)  # sorted: user-major
    u, i = key // n_items, key % n_items
    dev = key.device

    def indptr(ids, size):
        out = torch.zeros(size + 1, dtype=torch.int64, device=dev)
        out[1:] = torch.bincount(ids, minlength=size).cumsum(0)
        return out

    u_indptr = indptr(u, n_users)
    u_items = i.to(torch.int32)
    i_users = torch.sort(i * n_users + u).values % n_users
    i_indptr = indptr(i, n_items)
    return u_indptr, u_items, i_indptr, i_users.to(torch.int32)


def cooccurrence_plan(u_indptr, i_indptr, i_users, n_items: int,
                      hash_caps=HASH_CAPS, *, exclude_self: bool = True,
                      cross: bool = False):
    """Route the item rows to tiers. With d the user degrees, per item

        deg_i  = its user count
        work_i = sum of d_u over its users (pair visits incl. itself)
        ub_i   = min(N - 1, work_i - deg_i) >= its distinct neighbours

    Cross form (cross=True): (i_indptr, i_users) is the item-major CSR
    of the row side A, u_indptr the user-major row pointers of the
    column side B (d = dB), n_items = Nb, and with s = 1 if exclude_self
    else 0

        ub_i   = min(Nb - s, work_i)

    (work_i - s * deg_i would assume that every user of i in A also has
    i in B, which only the self form guarantees.)

    Returns three int32 row lists — ub <= hash_caps[0], ub <=
    hash_caps[1], the rest — each sorted by work descending, so the
    heaviest rows start first and no launch ends on one late heavy row.
    Rows with deg_i = 0 or ub_i = 0 have no neighbour and are in no
    list. Pure torch; runs on CPU too."""
    c0, c1 = int(hash_caps[0]), int(hash_caps[1])
    d = u_indptr[1:] - u_indptr[:-1]
    deg = i_indptr[1:] - i_indptr[:-1]
    cs = torch.zeros(i_users.numel() + 1, dtype=torch.int64,
                     device=i_users.device)
    cs[1:] = d[i_users.long()].cumsum(0)
    work = cs[i_indptr[1:]] - cs[i_indptr[:-1]]
    s = 1 if exclude_self else 0
    ub = torch.clamp(work if cross else work - s * deg,
                     max=int(n_items) - s)
    live = (deg > 0) & (ub > 0)
    order = torch.argsort(work, descending=True, stable=True)
    ub_o, live_o = ub[order], live[order]
    tiers = (live_o & (ub_o <= c0),
             live_o & (ub_o > c0) & (ub_o <= c1),
             live_o & (ub_o > max(c0, c1)))
    return tuple(order[m].to(torch.int32) for m in tiers)


def _xlx(x):
    x = x.to(torch.float64)
    return torch.xlogy(x, x)


def _check_score(score: str) -> bool:
    if score not in ("count", "llr"):
        raise ValueError(f'score must be "count" or "llr", got {score!r}')
    return score == "llr"


def cross_occurrence_topn_ref(users_a, items_a, n_items_a: int, users_b,
                              items_b, n_items_b: int, n_users: int, n: int,
                              *, score: str = "llr",
                              exclude_self: bool = False):
    """Plain torch reference: sparse A^T B in fp64, LLR in fp64 by the
    formula of the module docstring rounded to fp32 (or the counts),
    packed keys sorted, scattered into [Na, n]. Any n >= 1. Memory grows
    with the number of distinct co-occurring pairs."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    llr = _check_score(score)
    n_users, na, nb = int(n_users), int(n_items_a), int(n_items_b)
    if exclude_self and na != nb:
        raise ValueError("exclude_self needs n_items_a == n_items_b")
    mats, degs = [], []
    for users, items, size in ((users_a, items_a, na), (users_b, items_b, nb)):
        if mats and users is users_a and items is items_a and size == na:
            mats.append(mats[0])   # self mode: one pair set, built once
            degs.append(degs[0])
            break
        u_indptr, u_items, i_indptr, _ = build_csrs(users, items, n_users,
                                                    size)
        dev = u_items.device
        u = torch.repeat_interleave(torch.arange(n_users, device=dev),
                                    u_indptr[1:] - u_indptr[:-1])
        mats.append(torch.sparse_coo_tensor(
            torch.stack([u, u_items.long()]),
            torch.ones(u.numel(), dtype=torch.float64, device=dev),
            (n_users, size)).coalesce())
        degs.append(i_indptr[1:] - i_indptr[:-1])
    top_ids = torch.full((na, n), -1, dtype=torch.int32, device=dev)
    top_val = torch.zeros((na, n), device=dev,
                          dtype=torch.float32 if llr else torch.int32)
    if mats[0]._nnz() == 0 or mats[1]._nnz() == 0:
        return top_ids, top_val
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        C = torch.sparse.mm(mats[0].t(), mats[1]).coalesce()
    ii, jj = C.indices()[0], C.indices()[1]
    vv = C.values().round().to(torch.int64)
    keep = vv > 0
    if exclude_self:
        keep &= ii != jj
    ii, jj, vv = ii[keep], jj[keep], vv[keep]
    if llr:
        ai, bj = degs[0][ii], degs[1][jj]
        s = (_xlx(torch.tensor(n_users)) - _xlx(ai) - _xlx(n_users - ai)
             - _xlx(bj) - _xlx(n_users - bj) + _xlx(vv) + _xlx(ai - vv)
             + _xlx(bj - vv) + _xlx(n_users - ai - bj + vv))
        val = torch.clamp(2.0 * s, min=0.0).to(torch.float32)
        hi = val.view(torch.int32).to(torch.int64)
    else:
        val = vv.to(torch.int32)
        hi = vv
    key = (hi << 32) | (0xFFFFFFFF - jj)
    o1 = torch.argsort(key, descending=True, stable=True)
    o2 = torch.argsort(ii[o1], stable=True)
    order = o1[o2]
    ii, jj, val = ii[order], jj[order], val[order]
    start = torch.zeros(na + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.bincount(ii, minlength=na).cumsum(0)
    rank = torch.arange(ii.numel(), device=dev) - start[ii]
    keep = rank < n
    top_ids[ii[keep], rank[keep]] = jj[keep].to(torch.int32)
    top_val[ii[keep], rank[keep]] = val[keep]
    return top_ids, top_val


def cooccurrence_topn_ref(users, items, n_users: int, n_items: int, n: int,
                          *, score: str = "count"):
    """The reference in self mode: A^T A with the diagonal dropped."""
    return cross_occurrence_topn_ref(users, items, n_items, users, items,
                                     n_items, n_users, n, score=score,
                                     exclude_self=True)


def _check_csr(indptr, indices, n_cols: int, name: str):
    if indptr.dim() != 1 or indptr.numel() < 1 or indices.dim() != 1:
        raise ValueError(f"{name}: indptr and indices must be 1-D")
    nnz = indices.numel()
    if int(indptr[0]) != 0 or int(indptr[-1]) != nnz:
        raise ValueError(f"{name}: indptr must run from 0 to nnz = {nnz}")
    if indptr.numel() > 1 and int((indptr[1:] - indptr[:-1]).min()) < 0:
        raise ValueError(f"{name}: indptr must not decrease")
    if nnz:
        mn, mx = int(indices.min()), int(indices.max())
        if mn < 0 or mx >= n_cols:
            raise ValueError(f"{name}: id out of range: [{mn}, {mx}]"
                             f" vs {n_cols}")


def _topn_tiers(u_indptr, u_items, i_indptr, i_users, n_cols: int, n: int,
                llr: bool, exclude_self: bool, same_pairs: bool, col_deg,
                hash_caps, pool, pool_slots, dense_lds):
    """Validate, plan and launch every tier: rows from the item-major
    CSR (i_indptr, i_users) of A, columns from the user-major CSR
    (u_indptr, u_items) of B over n_cols items. col_deg: int64 [n_cols]
    user counts of B's items (LLR only)."""
    n_users = u_indptr.numel() - 1
    n_rows = i_indptr.numel() - 1
    if max(n_users, n_rows, n_cols) >= 2 ** 31:
        raise ValueError("user and item counts must be below 2^31")
    if exclude_self and n_rows != n_cols:
        raise ValueError("exclude_self needs the same item count on both "
                         "sides")
    caps = HASH_CAPS if hash_caps is None else tuple(int(c) for c in hash_caps)
    if len(caps) != 2 or caps[0] > HASH_CAPS[0] or caps[1] > HASH_CAPS[1]:
        raise ValueError(f"hash_caps must be a pair within {HASH_CAPS}")
    # a bad id is an out-of-bounds atomic: check before any launch
    _check_csr(u_indptr, u_items, n_cols, "user-major CSR")
    _check_csr(i_indptr, i_users, n_users, "item-major CSR")
    if dense_lds is None:
        dense_lds = (DENSE_LDS_MAX > 0 and n_cols <= DENSE_LDS_MAX
                     and pool is None and pool_slots is None)
    elif dense_lds and n_cols > DENSE_LDS_MAX:
        raise ValueError(f"dense_lds needs N <= {DENSE_LDS_MAX}")
    if pool is not None and (
            pool.dtype != torch.int32 or pool.dim() != 2 or not pool.is_cuda
            or not pool.is_contiguous() or pool.shape[0] < 1
            or pool.shape[1] != n_cols):
        raise ValueError("pool must be a contiguous int32 [G >= 1, N] "
                         "GPU tensor")

    from predictionio_amd.ops import hip_ext
    ext = hip_ext()
    dev = u_indptr.device
    u_indptr, u_items = u_indptr.contiguous(), u_items.contiguous()
    i_indptr, i_users = i_indptr.contiguous(), i_users.contiguous()
    top_ids = torch.full((n_rows, n), -1, dtype=torch.int32, device=dev)
    top_val = torch.zeros((n_rows, n), device=dev,
                          dtype=torch.float32 if llr else torch.int32)
    col_h = None
    if llr:
        col_h = _xlx(col_deg) + _xlx(n_users - col_deg)
        col_deg = col_deg.to(torch.int32)
    tiers = cooccurrence_plan(u_indptr, i_indptr, i_users, n_cols, caps,
                              exclude_self=exclude_self,
                              cross=not same_pairs)
    for tier, rows in enumerate(tiers):
        if rows.numel() == 0:
            continue
        tier_pool = None
        if tier == 2 and dense_lds:
            tier = 3
        elif tier == 2:
            slots = (int(pool_slots) if pool_slots is not None
                     else _default_pool_bytes() // (4 * n_cols))
            if pool is not None:
                slots = min(slots, pool.shape[0])
            slots = max(1, min(slots, rows.numel()))
            tier_pool = (pool[:slots] if pool is not None else
                         torch.zeros((slots, n_cols), dtype=torch.int32,
                                     device=dev))
        ext.cooc_topn(u_indptr, u_items, i_indptr, i_users, rows.contiguous(),
                      n, tier, tier_pool, top_ids, top_val, llr=llr,
                      exclude_self=exclude_self,
                      n_cols=-1 if same_pairs else n_cols,
                      col_deg=col_deg if llr else None, col_h=col_h)
    return top_ids, top_val


def cooccurrence_topn_csr(u_indptr, u_items, i_indptr, i_users, n: int, *,
                          score: str = "count", hash_caps=None, pool=None,
                          pool_slots=None, dense_lds=None):
    """GPU entry on prebuilt CSRs (see build_csrs); returns (top_ids,
    top_cnt), int32 [N, n], or with score="llr" (top_ids, top_score
    float32).

    The keyword arguments let tests reach every tier at tiny shapes:
    hash_caps lowers the routing caps (never above HASH_CAPS); pool is a
    caller's zero int32 [G, N] counter pool (all zero again afterwards)
    and pool_slots caps its rows; dense_lds picks where rows above the
    caps keep their dense counters — True: LDS (N <= DENSE_LDS_MAX),
    False: the global pool, None: LDS when it fits and no pool was
    asked for."""
    n = _check_n(n)
    llr = _check_score(score)
    if not u_indptr.is_cuda:
        raise ValueError("cooccurrence_topn_csr needs GPU tensors")
    if u_items.numel() != i_users.numel():
        raise ValueError("the two CSRs must hold the same pairs")
    return _topn_tiers(u_indptr, u_items, i_indptr, i_users,
                       i_indptr.numel() - 1, n, llr, True, True,
                       i_indptr[1:] - i_indptr[:-1], hash_caps, pool,
                       pool_slots, dense_lds)


def cross_occurrence_topn_csr(csrs_a, csrs_b, n: int, *, score: str = "llr",
                              exclude_self: bool = False, hash_caps=None,
                              pool=None, pool_slots=None, dense_lds=None):
    """GPU entry on the two pair sets' prebuilt CSRs (each the 4-tuple
    of build_csrs, over the same users); returns (top_ids, top_score
    float32) or, with score="count", (top_ids, top_cnt int32), [Na, n].
    Rows walk A's item-major and B's user-major CSR; the pool, the LDS
    counters and dense_lds are sized by Nb. The other keyword arguments
    are those of cooccurrence_topn_csr."""
    n = _check_n(n)
    llr = _check_score(score)
    _, _, a_indptr, a_users = csrs_a
    b_indptr, b_items, bi_indptr, bi_users = csrs_b
    if not (a_indptr.is_cuda and b_indptr.is_cuda):
        raise ValueError("cross_occurrence_topn_csr needs GPU tensors")
    if csrs_a[0].numel() != b_indptr.numel():
        raise ValueError("the two pair sets must be over the same users")
    # col_deg comes from B's item-major side: it must be B's pairs too
    _check_csr(bi_indptr, bi_users, b_indptr.numel() - 1, "B item-major CSR")
    if bi_users.numel() != b_items.numel():
        raise ValueError("B's two CSRs must hold the same pairs")
    return _topn_tiers(b_indptr, b_items, a_indptr, a_users,
                       bi_indptr.numel() - 1, n, llr, bool(exclude_self),
                       False, bi_indptr[1:] - bi_indptr[:-1], hash_caps,
                       pool, pool_slots, dense_lds)


def _pool_knobs(pool_bytes, n_cols: int):
    if pool_bytes is None:
        return {}
    return {"pool_slots": max(1, int(pool_bytes) // (4 * max(1, int(n_cols)))),
            "dense_lds": int(n_cols) <= DENSE_LDS_MAX}


def cooccurrence_topn(users, items, n_users: int, n_items: int, n: int, *,
                      score: str = "count", pool_bytes=None):
    """(top_ids, top_cnt), int32 [n_items, n] on the inputs' device, from
    raw (user, item) id tensors; duplicate pairs count once. With
    score="llr" the rows are ranked by the log-likelihood ratio and the
    result is (top_ids, top_score float32). CPU tensors go to the
    reference, GPU tensors to the kernels (n <= 64 there). pool_bytes
    bounds the dense tier's global counter pool (default 1 GiB, or
    PIO_COOC_POOL_MB)."""
    _check_score(score)
    if not users.is_cuda:
        return cooccurrence_topn_ref(users, items, n_users, n_items, n,
                                     score=score)
    n = _check_n(n)
    csrs = build_csrs(users, items, n_users, n_items)
    return cooccurrence_topn_csr(*csrs, n, score=score,
                                 **_pool_knobs(pool_bytes, n_items))


def cross_occurrence_topn(users_a, items_a, n_items_a: int, users_b, items_b,
                          n_items_b: int, n_users: int, n: int, *,
                          score: str = "llr", exclude_self: bool = False,
                          pool_bytes=None):
    """Cross-occurrence top-N of the pair sets A (rows) and B (columns)
    over the same n_users users: (top_ids int32, top_score float32)
    [n_items_a, n], or int32 counts with score="count"; see the module
    docstring. CPU tensors go to cross_occurrence_topn_ref, GPU tensors
    to the kernels (n <= 64 there)."""
    _check_score(score)
    if exclude_self and int(n_items_a) != int(n_items_b):
        raise ValueError("exclude_self needs n_items_a == n_items_b")
    if users_a.is_cuda != users_b.is_cuda:
        raise ValueError("both pair sets must be on the same device")
    if not users_a.is_cuda:
        return cross_occurrence_topn_ref(
            users_a, items_a, n_items_a, users_b, items_b, n_items_b,
            n_users, n, score=score, exclude_self=exclude_self)
    n = _check_n(n)
    return cross_occurrence_topn_csr(
        build_csrs(users_a, items_a, n_users, n_items_a),
        build_csrs(users_b, items_b, n_users, n_items_b), n, score=score,
        exclude_self=exclude_self, **_pool_knobs(pool_bytes, n_items_b))


# --------------------------------------------------------------------------
# Indicator top-K: serve the [Nr, n] table the ops above return.
#
#   s[b][j] = sum of top_scores[i][c] over the rows i of query b and the
#             columns c with top_ids[i][c] == j
#
# Candidates of b are the j that occur at least once (a sum of 0 still
# counts) and pass every filter given; the result is the K candidates with
# the largest s, score descending then id ascending, padded with -1 / 0.
# Count tables sum in int32, exactly. Float tables add the addends of one
# (b, j) in ascending value order in fp32, one rounding per add: the
# canonical sum, a function of the multiset of addends alone, so the
# kernel (csrc/indicator_topk.hip) and indicator_topk_ref agree bit for
# bit with each other and with themselves whatever the order of a table
# row or of the threads.
# --------------------------------------------------------------------------

# entry counts (query rows x n) the two kernel instantiations take; larger
# queries go through indicator_topk_ref
IND_WAVE_MAX = 512
IND_WG_MAX = 8192
IND_K_MAX = 1024
# table entries the torch route holds at a time
IND_REF_CHUNK = 1 << 22


def _check_lists(indptr, indices, B: int, n_cols: int, name: str):
    """A per-query CSR of sorted id lists: int64 indptr of B + 1 from 0
    to nnz, not decreasing; int32 ids in [0, n_cols), strictly ascending
    inside every query."""
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32:
        raise ValueError(f"{name}: indptr must be int64 and indices int32")
    _check_csr(indptr, indices, n_cols, name)
    if indptr.numel() != B + 1:
        raise ValueError(f"{name}: indptr must have B + 1 = {B + 1} entries")
    nnz = indices.numel()
    if nnz > 1:
        is_start = torch.zeros(nnz + 1, dtype=torch.bool,
                               device=indices.device)
        is_start[indptr] = True
        if bool(((indices[1:] <= indices[:-1]) & ~is_start[1:nnz]).any()):
            raise ValueError(f"{name}: ids must be strictly ascending inside"
                             " every query (sorted, no duplicates)")


def check_indicator_table(top_ids, top_scores, n_cols=None) -> None:
    """The table contract of indicator_topk: top_ids int32 [Nr, n] in
    [-1, n_cols), top_scores int32 or float32 of the same shape, every
    score >= 0 and finite. A model checks its table once with this and
    then calls indicator_topk(..., check_table=False)."""
    if top_ids.dim() != 2 or top_ids.dtype != torch.int32:
        raise ValueError("top_ids must be a 2-D int32 tensor")
    if top_scores.shape != top_ids.shape or top_scores.dtype not in (
            torch.int32, torch.float32):
        raise ValueError("top_scores must be int32 or float32 of top_ids' "
                         "shape")
    if top_scores.device != top_ids.device:
        raise ValueError("top_ids and top_scores must share a device")
    n_cols = top_ids.shape[0] if n_cols is None else int(n_cols)
    if not 1 <= n_cols < 2 ** 31 or top_ids.shape[0] >= 2 ** 31:
        raise ValueError("row and column counts must be below 2^31 and "
                         "n_cols >= 1")
    if top_ids.numel():
        mn, mx = int(top_ids.min()), int(top_ids.max())
        if mn < -1 or mx >= n_cols:
            raise ValueError(f"top_ids out of range: [{mn}, {mx}] vs "
                             f"[-1, {n_cols})")
        ok = top_scores >= 0
        if top_scores.dtype == torch.float32:
            ok &= torch.isfinite(top_scores)
        if not bool(ok.all()):
            raise ValueError("top_scores must be >= 0 and finite")


def _ind_check(top_ids, top_scores, q_indptr, q_items, K, n_cols,
               ban_indptr, ban_indices, allow_indptr, allow_indices,
               item_cats, query_cats, exclude_query, check_table):
    """Everything indicator_topk validates, before any launch. Returns
    (K, n_cols, lens int64 [B])."""
    from predictionio_amd.ops.topk import _check_cats
    K = int(K)
    if not 1 <= K <= IND_K_MAX:
        raise ValueError(f"K must be in [1, {IND_K_MAX}], got {K}")
    if (top_ids.dim() != 2 or top_ids.dtype != torch.int32
            or top_scores.shape != top_ids.shape
            or top_scores.dtype not in (torch.int32, torch.float32)
            or top_scores.device != top_ids.device):
        raise ValueError("top_ids must be int32 [Nr, n] and top_scores int32"
                         " or float32 of the same shape and device")
    nr = top_ids.shape[0]
    n_cols = nr if n_cols is None else int(n_cols)
    if not 1 <= n_cols < 2 ** 31 or nr >= 2 ** 31:
        raise ValueError("row and column counts must be below 2^31 and "
                         "n_cols >= 1")
    if exclude_query and n_cols != nr:
        raise ValueError("exclude_query needs n_cols == the table's row "
                         "count")
    if q_indptr.dim() != 1 or q_indptr.numel() < 1:
        raise ValueError("query CSR: indptr must be 1-D and not empty")
    B = q_indptr.numel() - 1
    _check_lists(q_indptr, q_items, B, nr, "query CSR")
    lists = [q_indptr, q_items]
    for ip, ix, name in ((ban_indptr, ban_indices, "ban list"),
                         (allow_indptr, allow_indices, "allow list")):
        if (ip is None) != (ix is None):
            raise ValueError(f"{name}: indptr and indices must be given "
                             "together")
        if ip is not None:
            _check_lists(ip, ix, B, n_cols, name)
            lists += [ip, ix]
    _check_cats(item_cats, query_cats, B, n_cols)
    if item_cats is not None:
        lists += [item_cats, query_cats]
    if any(t.device != top_ids.device for t in lists):
        raise ValueError("all tensors must be on the table's device")
    if check_table:
        check_indicator_table(top_ids, top_scores, n_cols)
    lens = q_indptr[1:] - q_indptr[:-1]
    if top_scores.dtype == torch.int32 and B and top_scores.numel():
        if int(lens.max()) * int(top_scores.max()) >= 2 ** 31:
            raise ValueError("count sums may reach 2^31: max query length x"
                             " max count must stay below it")
    return K, n_cols, lens


def _ind_torch(top_ids, top_scores, q_indptr, q_items, queries, lens, K,
               n_cols, ban, allow, item_cats, query_cats, exclude_query,
               out_ids, out_sc, chunk: int = IND_REF_CHUNK):
    """The definition in plain torch for the listed queries (int64 ids),
    written into their rows of out_ids / out_sc. Entries are sorted by
    (query, j, score bits); the canonical sum is then formed segment by
    segment, position r of every segment added in step r. Chunked over
    queries so that at most `chunk` table entries (or one query) are in
    flight."""
    import numpy as np
    dev = top_ids.device
    n = top_ids.shape[1]
    is_float = top_scores.dtype == torch.float32
    B = lens.numel()
    if queries.numel() == 0 or n == 0:
        return

    def list_keys(indptr, indices):
        qid = torch.repeat_interleave(torch.arange(B, device=dev),
                                      indptr[1:] - indptr[:-1])
        return qid * n_cols + indices.long()

    own_keys = list_keys(q_indptr, q_items) if exclude_query else None
    ban_keys = list_keys(*ban) if ban is not None else None
    allow_keys = list_keys(*allow) if allow is not None else None

    cum = np.cumsum((lens[queries] * n).cpu().numpy())
    i = 0
    while i < len(cum):
        base = int(cum[i - 1]) if i else 0
        e = max(int(np.searchsorted(cum, base + chunk, side="right")), i + 1)
        qs = queries[i:e]
        i = e
        m = lens[qs]
        total = int(m.sum())
        if total == 0:
            continue
        rep = torch.repeat_interleave(torch.arange(qs.numel(), device=dev), m,
                                      output_size=total)
        off = torch.arange(total, device=dev) - (m.cumsum(0) - m)[rep]
        rows = q_items[q_indptr[qs][rep] + off].long()
        j = top_ids[rows].long().reshape(-1)
        v = top_scores[rows].reshape(-1)
        b = qs[rep].repeat_interleave(n)
        keep = j >= 0
        j, v, b = j[keep], v[keep], b[keep]
        if j.numel() == 0:
            continue
        if is_float:
            v = v + 0.0                           # -0.0 -> +0.0
        bits = v.view(torch.int32).long()         # >= 0: value order
        o = torch.argsort((j << 32) | bits)
        o = o[torch.argsort(b[o], stable=True)]
        j, v, b = j[o], v[o], b[o]
        head = torch.ones(j.numel(), dtype=torch.bool, device=dev)
        head[1:] = (b[1:] != b[:-1]) | (j[1:] != j[:-1])
        start = head.nonzero().reshape(-1)
        length = torch.diff(start, append=torch.tensor([j.numel()],
                                                       device=dev))
        acc = v[start].clone()
        for r in range(1, int(length.max())):
            sel = length > r
            acc[sel] = acc[sel] + v[start[sel] + r]
        sb, sj = b[start], j[start]
        ok = torch.ones_like(sj, dtype=torch.bool)
        key = sb * n_cols + sj
        if own_keys is not None:
            ok &= ~torch.isin(key, own_keys)
        if ban_keys is not None:
            ok &= ~torch.isin(key, ban_keys)
        if allow_keys is not None:
            ok &= torch.isin(key, allow_keys)
        if item_cats is not None:
            ok &= ((item_cats[sj] & query_cats[sb]) != 0).any(dim=1)
        sb, sj, acc = sb[ok], sj[ok], acc[ok]
        if sb.numel() == 0:
            continue
        o = torch.argsort((acc.view(torch.int32).long() << 32)
                          | (0xFFFFFFFF - sj), descending=True)
        o = o[torch.argsort(sb[o], stable=True)]
        sb, sj, acc = sb[o], sj[o], acc[o]
        first = torch.ones(sb.numel(), dtype=torch.bool, device=dev)
        first[1:] = sb[1:] != sb[:-1]
        pos = torch.arange(sb.numel(), device=dev)
        rank = pos - torch.cummax(torch.where(first, pos, 0), 0).values
        keep = rank < K
        out_ids[sb[keep], rank[keep]] = sj[keep].to(torch.int32)
        out_sc[sb[keep], rank[keep]] = acc[keep]


def _ind_out(B: int, K: int, top_scores):
    dev = top_scores.device
    return (torch.full((B, K), -1, dtype=torch.int32, device=dev),
            torch.zeros((B, K), dtype=top_scores.dtype, device=dev))


def _opt_pair(indptr, indices):
    return None if indptr is None else (indptr.contiguous(),
                                        indices.contiguous())


def indicator_topk_ref(top_ids, top_scores, q_indptr, q_items, K, *,
                       n_cols=None, ban_indptr=None, ban_indices=None,
                       allow_indptr=None, allow_indices=None, item_cats=None,
                       query_cats=None, exclude_query=True, check_table=True,
                       chunk: int = IND_REF_CHUNK):
    """indicator_topk in plain torch on the inputs' device: the CPU path,
    the route of queries above the kernel's cap, and what the GPU tests
    compare against. Memory is O(chunk) table entries."""
    K, n_cols, lens = _ind_check(
        top_ids, top_scores, q_indptr, q_items, K, n_cols, ban_indptr,
        ban_indices, allow_indptr, allow_indices, item_cats, query_cats,
        exclude_query, check_table)
    out_ids, out_sc = _ind_out(lens.numel(), K, top_scores)
    _ind_torch(top_ids, top_scores, q_indptr, q_items,
               torch.arange(lens.numel(), device=top_ids.device), lens, K,
               n_cols, _opt_pair(ban_indptr, ban_indices),
               _opt_pair(allow_indptr, allow_indices), item_cats, query_cats,
               exclude_query, out_ids, out_sc, chunk)
    return out_ids, out_sc


def indicator_topk(top_ids, top_scores, q_indptr, q_items, K, *,
                   n_cols=None, ban_indptr=None, ban_indices=None,
                   allow_indptr=None, allow_indices=None, item_cats=None,
                   query_cats=None, exclude_query=True, check_table=True):
    """Sum the indicator rows of every query's items, filter and rank:
    (ids int32 [B, K], scores [B, K] of top_scores.dtype), score
    descending then id ascending, padded with -1 / 0.

    top_ids int32 [Nr, n] (-1 padded) and top_scores int32 or float32
    [Nr, n] (>= 0, finite) are what cooccurrence_topn /
    cross_occurrence_topn return; n_cols (default Nr) is the id space of
    top_ids' entries. (q_indptr int64 [B + 1], q_items int32) lists the
    table rows of each query, strictly ascending. A candidate must pass
    every filter given: not a row of the query itself (exclude_query;
    needs n_cols == Nr), not in the query's ban list, in its allow list
    (both CSRs like the query's, ids in [0, n_cols)), and the category
    word test of topk_score (item_cats [n_cols, W], query_cats [B, W]).
    Every argument is validated before any launch; check_table=False
    skips the scan of the table for a caller that ran
    check_indicator_table once.

    GPU tensors go to csrc/indicator_topk.hip: queries of at most
    IND_WAVE_MAX table entries (rows x n) to its one-wave instantiation,
    of at most IND_WG_MAX to the 256-thread one, each a persistent launch
    over its queries sorted by entry count; larger queries, and CPU
    tensors, go through indicator_topk_ref. The route depends on the
    query's own entry count alone and both routes form the same canonical
    sum, so results do not depend on the batch."""
    K, n_cols, lens = _ind_check(
        top_ids, top_scores, q_indptr, q_items, K, n_cols, ban_indptr,
        ban_indices, allow_indptr, allow_indices, item_cats, query_cats,
        exclude_query, check_table)
    B = lens.numel()
    n = top_ids.shape[1]
    dev = top_ids.device
    out_ids, out_sc = _ind_out(B, K, top_scores)
    ban = _opt_pair(ban_indptr, ban_indices)
    allow = _opt_pair(allow_indptr, allow_indices)
    top_ids, top_scores = top_ids.contiguous(), top_scores.contiguous()
    q_indptr, q_items = q_indptr.contiguous(), q_items.contiguous()
    if not top_ids.is_cuda:
        _ind_torch(top_ids, top_scores, q_indptr, q_items,
                   torch.arange(B, device=dev), lens, K, n_cols, ban, allow,
                   item_cats, query_cats, exclude_query, out_ids, out_sc)
        return out_ids, out_sc
    if B == 0 or n == 0:
        return out_ids, out_sc
    from predictionio_amd.ops import hip_ext
    ext = hip_ext()
    E = lens * n
    order = torch.argsort(E, descending=True, stable=True)
    n_big, n_wg, n_live, m_wg, m_wave = torch.stack([
        (E > IND_WG_MAX).sum(), (E > IND_WAVE_MAX).sum(), (E > 0).sum(),
        torch.where(E <= IND_WG_MAX, lens, 0).max(),
        torch.where(E <= IND_WAVE_MAX, lens, 0).max()]).tolist()
    for work, threads, max_items in (
            (order[n_big:n_wg], 256, m_wg), (order[n_wg:n_live], 64, m_wave)):
        if work.numel():
            ext.indicator_topk(
                top_ids, top_scores, q_indptr, q_items,
                work.to(torch.int32).contiguous(), max_items, threads, K,
                n_cols, ban[0] if ban else None, ban[1] if ban else None,
                allow[0] if allow else None, allow[1] if allow else None,
                item_cats, query_cats, bool(exclude_query), out_ids, out_sc)
    if n_big:
        _ind_torch(top_ids, top_scores, q_indptr, q_items, order[:n_big],
                   lens, K, n_cols, ban, allow, item_cats, query_cats,
                   exclude_query, out_ids, out_sc)
    return out_ids, out_sc
