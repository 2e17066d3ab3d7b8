#!/usr/bin/env python
"""Co-occurrence top-N: the fused pair-count kernels against the path
they replace (torch.sparse.mm(A^T, A) + a host lexsort), per shape.

Every measurement runs in a child process of its own under a time limit
(--timeout), synchronised, median of 7 runs after one warm-up; the
driver starts nothing more once a child fails or runs out of time. The
old path materialises one entry per (user, item, item) triple, so it is
run only where that count is at most --old-max-triples.

    python scripts/cooccurrence_bench.py                 # every shape
    python scripts/cooccurrence_bench.py --shapes small  # one of them

Prints one JSON line per measurement: wall time, peak device memory
above the inputs, and for the kernels the rows, summed pair visits and
time of each tier.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (users, items, views per user, item distribution)
SHAPES = {
    "small": (50_000, 40_000, 20, "uniform"),
    "uniform": (1_250_000, 1_000_000, 20, "uniform"),
    "zipf": (1_250_000, 1_000_000, 20, "zipf"),
    "zipf20k": (200_000, 20_000, 50, "zipf"),
}
RUNS = 7
N_KEEP = 10


def make_pairs(name, device):
    import torch
    n_users, n_items, views, dist = SHAPES[name]
    g = torch.Generator(device=device).manual_seed(0)
    if dist == "uniform":
        i = torch.randint(0, n_items, (n_users, views), generator=g,
                          device=device)
    else:  # Zipf(1) by inverse CDF
        w = 1.0 / torch.arange(1, n_items + 1, device=device,
                               dtype=torch.float64)
        cdf = (w / w.sum()).cumsum(0)
        r = torch.rand((n_users, views), generator=g, device=device,
                       dtype=torch.float64)
        i = torch.searchsorted(cdf, r).clamp_(max=n_items - 1)
    u = torch.arange(n_users, device=device).unsqueeze(1).expand_as(i)
    return u.reshape(-1).contiguous(), i.reshape(-1).contiguous()


def timed(fn):
    import torch
    fn()  # warm-up
    out = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return statistics.median(out)


def old_path(u, i, n_users, n_items, n_keep):
    """What CooccurrenceAlgorithm.train did before the kernels, up to
    the sorted pair arrays (the dict loop after them is unchanged)."""
    import numpy as np
    import torch
    key = torch.unique(u * n_items + i)
    u, i = key // n_items, key % n_items
    A = torch.sparse_coo_tensor(torch.stack([u, i]),
                                torch.ones(u.numel(), device=u.device),
                                (n_users, n_items)).coalesce()
    C = torch.sparse.mm(A.t(), A).coalesce()
    ii = C.indices()[0].cpu().numpy()
    jj = C.indices()[1].cpu().numpy()
    vv = C.values().cpu().numpy()
    off = ii != jj
    ii, jj, vv = ii[off], jj[off], vv[off].astype(np.int64)
    order = np.lexsort((-vv, ii))
    return ii[order], jj[order], vv[order]


def child(name, path, dense_lds):
    import torch
    from predictionio_amd.ops import cooccurrence as co
    from predictionio_amd.ops import hip_ext
    dev = torch.device("cuda")
    n_users, n_items, _, _ = SHAPES[name]
    u, i = make_pairs(name, dev)
    res = {"shape": name, "path": path, "users": n_users, "items": n_items,
           "pairs": int(u.numel())}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    if path == "old":
        res["wall_s"] = timed(lambda: old_path(u, i, n_users, n_items, N_KEEP))
    else:
        lds = {"auto": None, "lds": True, "pool": False}[dense_lds]
        csrs = co.build_csrs(u, i, n_users, n_items)
        res["wall_s"] = timed(
            lambda: co.cooccurrence_topn_csr(*co.build_csrs(
                u, i, n_users, n_items), N_KEEP, dense_lds=lds))
    torch.cuda.synchronize()
    res["peak_mib"] = round(
        (torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
    if path == "new":
        # per tier: rows, pair visits, and the launch alone
        ext = hip_ext()
        u_indptr, u_items, i_indptr, i_users = csrs
        tiers = co.cooccurrence_plan(u_indptr, i_indptr, i_users, n_items)
        d = u_indptr[1:] - u_indptr[:-1]
        cs = torch.zeros(i_users.numel() + 1, dtype=torch.int64, device=dev)
        cs[1:] = d[i_users.long()].cumsum(0)
        work = cs[i_indptr[1:]] - cs[i_indptr[:-1]]
        ids = torch.full((n_items, N_KEEP), -1, dtype=torch.int32, device=dev)
        cnt = torch.zeros_like(ids)
        use_lds = n_items <= co.DENSE_LDS_MAX if lds is None else lds
        res["dense_in_lds"] = bool(use_lds)
        res["tiers"] = []
        for t, rows in enumerate(tiers):
            entry = {"rows": int(rows.numel()),
                     "visits": int(work[rows.long()].sum())}
            if rows.numel():
                pool, tier = None, t
                if t == 2 and use_lds:
                    tier = 3
                elif t == 2:
                    slots = max(1, min(rows.numel(),
                                       (1 << 30) // (4 * n_items)))
                    pool = torch.zeros((slots, n_items), dtype=torch.int32,
                                       device=dev)
                entry["s"] = timed(lambda: ext.cooc_topn(
                    u_indptr, u_items, i_indptr, i_users, rows, N_KEEP,
                    tier, pool, ids, cnt))
            res["tiers"].append(entry)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--timeout", type=float, default=300.0,
                    help="seconds per child process")
    ap.add_argument("--old-max-triples", type=float, default=1e8)
    ap.add_argument("--dense", default="auto", choices=["auto", "lds", "pool"],
                    help="where rows above the hash caps keep counters")
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "PATH"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.dense)
        return 0
    for name in a.shapes.split(","):
        n_users, _, views, _ = SHAPES[name]
        paths = ["new"]
        if n_users * views * views <= a.old_max_triples:
            paths.append("old")
        else:
            print(json.dumps({"shape": name, "path": "old",
                              "skipped": "more triples than "
                                         "--old-max-triples"}), flush=True)
        for path in paths:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name,
                   path, "--dense", a.dense]
            try:
                rc = subprocess.run(cmd, timeout=a.timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"{name}/{path}: exit {rc}; stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
