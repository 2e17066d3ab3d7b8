#!/usr/bin/env python
"""ALS half-step at ranks 192 and 256: the packed-triangle MFMA solver
(csrc/als_wide.hip) against a plain torch route on the same device.

Ratings are bench-shaped: --users users x 20 ratings whose item ids follow
a seeded Zipf law of exponent 1 over --items items. The user side is a
half-step over rows of degree 20, the item side one over the Zipf degrees.

The torch route: rows sorted by degree and cut into batches that fit
--batch-mb; per batch the gathered factor rows are zero-padded to the
batch's longest row, the normal matrices are one bmm, then
torch.linalg.cholesky and cholesky_solve. Both routes solve the implicit
system of als_solve; their results are compared.

Prints one JSON line per measurement. Times are host clocks around work
that ends in a device synchronise, after one warm-up of each route.
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

from predictionio_amd.ops import als as als_ops  # noqa: E402

DEV = torch.device("cuda", 0)
LAM, ALPHA = 0.05, 40.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_route(indptr, cols, vals, Y, yty, batch_bytes):
    n_rows, f = indptr.numel() - 1, Y.shape[1]
    deg = indptr[1:] - indptr[:-1]
    order = torch.argsort(deg)
    deg_s = deg[order].tolist()
    X = torch.empty((n_rows, f), device=DEV)
    base = yty + LAM * torch.eye(f, device=DEV)
    lo = 0
    while lo < n_rows:
        # the largest batch whose padded gather and matrices both fit
        hi = lo + 1
        while hi < n_rows and (hi + 1 - lo) * 4 * f * max(
                deg_s[hi], f) <= batch_bytes:
            hi += 1
        rows = order[lo:hi]
        d = max(deg_s[hi - 1], 1)
        k = torch.arange(d, device=DEV)
        live = k[None, :] < deg[rows][:, None]
        pos = (indptr[rows][:, None] + k[None, :]).clamp_(
            max=cols.numel() - 1)
        Yr = Y[cols[pos].long()] * live[:, :, None]
        r = vals[pos] * live
        A = base + torch.bmm((Yr * (ALPHA * r)[:, :, None]).mT, Yr)
        b = torch.bmm(Yr.mT, ((1.0 + ALPHA * r) * live)[:, :, None])
        X[rows] = torch.cholesky_solve(b, torch.linalg.cholesky(A))[:, :, 0]
        lo = hi
    return X


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=50_000)
    ap.add_argument("--ranks", type=int, nargs="+", default=[192, 256])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-mb", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("als_wide_rank_probe needs a GPU: timings elsewhere say "
                 "nothing")
    g = torch.Generator(device=DEV).manual_seed(args.seed)
    cdf = torch.cumsum(1.0 / torch.arange(
        1, args.items + 1, device=DEV, dtype=torch.float64), 0)
    cdf /= cdf[-1].clone()
    u = torch.rand(args.users * 20, generator=g, device=DEV,
                   dtype=torch.float64)
    items = torch.searchsorted(cdf, u).clamp_(max=args.items - 1)
    users = torch.arange(args.users, device=DEV).repeat_interleave(20)
    vals = torch.ones(items.numel(), device=DEV)
    sides = {
        "user": (als_ops.build_csr(users, items, vals, args.users),
                 args.items),
        "item": (als_ops.build_csr(items, users, vals, args.items),
                 args.users),
    }
    for f in args.ranks:
        for side, ((indptr, cols, v), n_fixed) in sides.items():
            Y = torch.randn((n_fixed, f), generator=g, device=DEV) / f ** 0.5
            yty = als_ops.gramian(Y)
            routes = {
                "kernel": lambda: als_ops.als_solve(
                    indptr, cols, v, Y, YtY=yty, lam=LAM, alpha=ALPHA,
                    implicit=True),
                "torch": lambda: torch_route(indptr, cols, v, Y, yty,
                                             args.batch_mb << 20),
            }
            res = {name: fn() for name, fn in routes.items()}  # warm-up
            ms = {name: [] for name in routes}
            for _ in range(args.reps):
                for name, fn in routes.items():
                    ms[name].append(round(1e3 * timed(fn)[0], 3))
            deg = indptr[1:] - indptr[:-1]
            print(json.dumps({
                "probe": "als_wide_rank", "f": f, "side": side,
                "rows": int(deg.numel()), "nnz": int(cols.numel()),
                "max_degree": int(deg.max()), "ms": ms,
                "rel_diff_kernel_vs_torch": (
                    (res["kernel"] - res["torch"]).norm()
                    / res["torch"].norm()).item(),
                "device": torch.cuda.get_device_name()}), flush=True)


if __name__ == "__main__":
    main()
