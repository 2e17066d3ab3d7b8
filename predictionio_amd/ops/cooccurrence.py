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
                      hash_caps=HASH_CAPS):
    """Route the item rows to tiers. With d the user degrees, per item

        deg_i  = its user count
        work_i = sum of d_u over its users (pair visits incl. itself)
        ub_i   = min(N - 1, work_i - deg_i) >= its distinct neighbours

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
    ub = torch.clamp(work - deg, max=int(n_items) - 1)
    live = (deg > 0) & (ub > 0)
    order = torch.argsort(work, descending=True, stable=True)
    ub_o, live_o = ub[order], live[order]
    tiers = (live_o & (ub_o <= c0),
             live_o & (ub_o > c0) & (ub_o <= c1),
             live_o & (ub_o > max(c0, c1)))
    return tuple(order[m].to(torch.int32) for m in tiers)


def cooccurrence_topn_ref(users, items, n_users: int, n_items: int, n: int):
    """Plain torch reference: sparse A^T A, diagonal dropped, packed keys
    sorted, scattered into [N, n]. Any n >= 1. Memory grows with the
    number of distinct co-occurring pairs."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    u_indptr, u_items, _, _ = build_csrs(users, items, n_users, n_items)
    dev = u_items.device
    n_users, n_items = int(n_users), int(n_items)
    top_ids = torch.full((n_items, n), -1, dtype=torch.int32, device=dev)
    top_cnt = torch.zeros((n_items, n), dtype=torch.int32, device=dev)
    if u_items.numel() == 0:
        return top_ids, top_cnt
    u = torch.repeat_interleave(torch.arange(n_users, device=dev),
                                u_indptr[1:] - u_indptr[:-1])
    A = torch.sparse_coo_tensor(
        torch.stack([u, u_items.long()]),
        torch.ones(u.numel(), dtype=torch.float64, device=dev),
        (n_users, n_items)).coalesce()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        C = torch.sparse.mm(A.t(), A).coalesce()
    ii, jj = C.indices()[0], C.indices()[1]
    vv = C.values().round().to(torch.int64)
    off = (ii != jj) & (vv > 0)
    ii, jj, vv = ii[off], jj[off], vv[off]
    key = (vv << 32) | (0xFFFFFFFF - jj)
    o1 = torch.argsort(key, descending=True, stable=True)
    o2 = torch.argsort(ii[o1], stable=True)
    order = o1[o2]
    ii, jj, vv = ii[order], jj[order], vv[order]
    start = torch.zeros(n_items + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.bincount(ii, minlength=n_items).cumsum(0)
    rank = torch.arange(ii.numel(), device=dev) - start[ii]
    keep = rank < n
    top_ids[ii[keep], rank[keep]] = jj[keep].to(torch.int32)
    top_cnt[ii[keep], rank[keep]] = vv[keep].to(torch.int32)
    return top_ids, top_cnt


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


def cooccurrence_topn_csr(u_indptr, u_items, i_indptr, i_users, n: int, *,
                          hash_caps=None, pool=None, pool_slots=None,
                          dense_lds=None):
    """GPU entry on prebuilt CSRs (see build_csrs); returns (top_ids,
    top_cnt), int32 [N, n].

    The keyword arguments let tests reach every tier at tiny shapes:
    hash_caps lowers the routing caps (never above HASH_CAPS); pool is a
    caller's zero int32 [G, N] counter pool (all zero again afterwards)
    and pool_slots caps its rows; dense_lds picks where rows above the
    caps keep their dense counters — True: LDS (N <= DENSE_LDS_MAX),
    False: the global pool, None: LDS when it fits and no pool was
    asked for."""
    n = _check_n(n)
    if not u_indptr.is_cuda:
        raise ValueError("cooccurrence_topn_csr needs GPU tensors")
    n_users = u_indptr.numel() - 1
    n_items = i_indptr.numel() - 1
    if n_users >= 2 ** 31 or n_items >= 2 ** 31:
        raise ValueError("user and item counts must be below 2^31")
    caps = HASH_CAPS if hash_caps is None else tuple(int(c) for c in hash_caps)
    if len(caps) != 2 or caps[0] > HASH_CAPS[0] or caps[1] > HASH_CAPS[1]:
        raise ValueError(f"hash_caps must be a pair within {HASH_CAPS}")
    if u_items.numel() != i_users.numel():
        raise ValueError("the two CSRs must hold the same pairs")
    # a bad id is an out-of-bounds atomic: check before any launch
    _check_csr(u_indptr, u_items, n_items, "user-major CSR")
    _check_csr(i_indptr, i_users, n_users, "item-major CSR")
    if dense_lds is None:
        dense_lds = (DENSE_LDS_MAX > 0 and n_items <= DENSE_LDS_MAX
                     and pool is None and pool_slots is None)
    elif dense_lds and n_items > DENSE_LDS_MAX:
        raise ValueError(f"dense_lds needs N <= {DENSE_LDS_MAX}")
    if pool is not None and (
            pool.dtype != torch.int32 or pool.dim() != 2 or not pool.is_cuda
            or not pool.is_contiguous() or pool.shape[0] < 1
            or pool.shape[1] != n_items):
        raise ValueError("pool must be a contiguous int32 [G >= 1, N] "
                         "GPU tensor")

    from predictionio_amd.ops import hip_ext
    ext = hip_ext()
    dev = u_indptr.device
    u_indptr, u_items = u_indptr.contiguous(), u_items.contiguous()
    i_indptr, i_users = i_indptr.contiguous(), i_users.contiguous()
    top_ids = torch.full((n_items, n), -1, dtype=torch.int32, device=dev)
    top_cnt = torch.zeros((n_items, n), dtype=torch.int32, device=dev)
    tiers = cooccurrence_plan(u_indptr, i_indptr, i_users, n_items, caps)
    for tier, rows in enumerate(tiers):
        if rows.numel() == 0:
            continue
        tier_pool = None
        if tier == 2 and dense_lds:
            tier = 3
        elif tier == 2:
            slots = (int(pool_slots) if pool_slots is not None
                     else _default_pool_bytes() // (4 * n_items))
            if pool is not None:
                slots = min(slots, pool.shape[0])
            slots = max(1, min(slots, rows.numel()))
            tier_pool = (pool[:slots] if pool is not None else
                         torch.zeros((slots, n_items), dtype=torch.int32,
                                     device=dev))
        ext.cooc_topn(u_indptr, u_items, i_indptr, i_users, rows.contiguous(),
                      n, tier, tier_pool, top_ids, top_cnt)
    return top_ids, top_cnt


def cooccurrence_topn(users, items, n_users: int, n_items: int, n: int, *,
                      pool_bytes=None):
    """(top_ids, top_cnt), int32 [n_items, n] on the inputs' device, from
    raw (user, item) id tensors; duplicate pairs count once. CPU tensors
    go to the reference, GPU tensors to the kernels (n <= 64 there).
    pool_bytes bounds the dense tier's global counter pool (default 1 GiB,
    or PIO_COOC_POOL_MB)."""
    if not users.is_cuda:
        return cooccurrence_topn_ref(users, items, n_users, n_items, n)
    n = _check_n(n)
    csrs = build_csrs(users, items, n_users, n_items)
    slots = None
    if pool_bytes is not None:
        slots = max(1, int(pool_bytes) // (4 * max(1, int(n_items))))
    return cooccurrence_topn_csr(*csrs, n, pool_slots=slots,
                                 dense_lds=None if slots is None else
                                 int(n_items) <= DENSE_LDS_MAX)
