#!/usr/bin/env python
"""Heavy-row ALS probe: where the split-row route (csrc/als_heavy.hip)
starts to pay, and which chunk length it wants.

  sweep   one implicit half-step over a CSR of --rows rows of degree 20
          plus 64 rows of degree n, n in --degrees, F in --ranks; the
          route off (PIO_ALS_HEAVY_MIN=0) and on (threshold just below n),
          alternating in one process after warm-up. At the largest n the
          chunk lengths in --chunks are timed too.
  zipf    one training iteration (both half-steps) on --rows users x 20
          ratings whose item ids follow a seeded Zipf law of exponent 1;
          route off against on at the defaults.

Prints one JSON line per measurement. Times are host clocks around work
that ends in a device synchronise.
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def alternate(fn, envs, reps):
    """Warm every variant once, then time them in turn, reps times;
    returns {name: [seconds]}."""
    for env in envs.values():
        timed(fn, env)
    out = {name: [] for name in envs}
    for _ in range(reps):
        for name, env in envs.items():
            out[name].append(timed(fn, env))
    return out


def sweep_csr(n_light, n, n_cols, seed):
    """n_light rows of degree 20 with 64 rows of degree n spread among
    them, columns uniform."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    deg = torch.full((n_light + 64,), 20, dtype=torch.int64, device=DEV)
    deg[torch.arange(64, device=DEV) * (n_light // 64) + 7] = n
    indptr = torch.zeros(deg.numel() + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(deg, 0, out=indptr[1:])
    nnz = int(indptr[-1])
    cols = torch.randint(0, n_cols, (nnz,), generator=g, device=DEV,
                         dtype=torch.int32)
    vals = torch.ones(nnz, device=DEV)
    return indptr, cols, vals


def run_sweep(args):
    for f in args.ranks:
        g = torch.Generator(device=DEV).manual_seed(args.seed + f)
        Y = torch.randn((args.cols, f), generator=g, device=DEV) / f ** 0.5
        yty = als_ops.gramian(Y)
        lv = als_ops.prepare_lv(Y, yty, 0.05)
        for n in args.degrees:
            indptr, cols, vals = sweep_csr(args.rows, n, args.cols,
                                           args.seed + n)
            out = torch.empty((indptr.numel() - 1, f), device=DEV)

            def half_step():
                als_ops.als_solve(indptr, cols, vals, Y, YtY=yty, lam=0.05,
                                  alpha=40.0, implicit=True, lv=lv, out=out)

            on = {"PIO_ALS_HEAVY_MIN": str(n - 1)}
            envs = {"off": {"PIO_ALS_HEAVY_MIN": "0"}, "on": dict(on)}
            if n == max(args.degrees):
                for c in args.chunks:
                    envs[f"on_chunk{c}"] = dict(
                        on, PIO_ALS_HEAVY_CHUNK=str(c))
            reps = args.reps if n < 500_000 else max(2, args.reps // 2)
            t = alternate(half_step, envs, reps)
            x_on = out.clone()
            timed(half_step, envs["off"])
            heavy = (indptr[1:] - indptr[:-1]) > 20
            err = ((x_on[heavy] - out[heavy]).norm()
                   / out[heavy].norm()).item()
            emit(probe="sweep", f=f, n=n, rows=args.rows, reps=reps,
                 ms={k: [round(1e3 * s, 3) for s in v] for k, v in t.items()},
                 median_ms={k: round(1e3 * sorted(v)[len(v) // 2], 3)
                            for k, v in t.items()},
                 heavy_rows_rel_diff_on_vs_off=err)
            del indptr, cols, vals, out, x_on


def run_zipf(args):
    from predictionio_amd.models.als import ALSParams, ALSTrainer
    n_users, n_items = args.rows, args.cols
    g = torch.Generator(device=DEV).manual_seed(args.seed)
    cdf = torch.cumsum(
        1.0 / torch.arange(1, n_items + 1, device=DEV, dtype=torch.float64),
        0)
    cdf /= cdf[-1].clone()
    u = torch.rand(n_users * 20, generator=g, device=DEV,
                   dtype=torch.float64)
    items = torch.searchsorted(cdf, u).clamp_(max=n_items - 1).int()
    users = torch.arange(n_users, device=DEV,
                         dtype=torch.int32).repeat_interleave(20)
    vals = torch.ones(items.numel(), device=DEV)
    p = ALSParams(rank=args.ranks[0], iterations=1, lambda_=0.05,
                  alpha=40.0, implicit=True, seed=args.seed)
    tr = ALSTrainer(p, n_users, n_items, DEV)
    tr.set_ratings_sharded((users, items, vals), (items, users, vals))
    tr.init_factors()
    x0, y0 = tr.X.clone(), tr.Y.clone()
    deg = tr.item_csr[0][1:] - tr.item_csr[0][:-1]

    def iteration():
        tr.X, tr.Y, tr._pending_y = x0.clone(), y0.clone(), None
        tr.step()

    t = alternate(iteration, {"off": {"PIO_ALS_HEAVY_MIN": "0"}, "on": {}},
                  args.reps)
    emit(probe="zipf", f=args.ranks[0], users=n_users, items=n_items,
         nnz=int(items.numel()), max_item_degree=int(deg.max()),
         items_above_heavy_min=int((deg > als_ops.heavy_min()).sum()),
         heavy_min=als_ops.heavy_min(), heavy_chunk=als_ops.heavy_chunk(),
         ms={k: [round(1e3 * s, 3) for s in v] for k, v in t.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["sweep", "zipf"])
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--cols", type=int, default=1_000_000)
    ap.add_argument("--degrees", type=int, nargs="+",
                    default=[256, 1024, 4096, 16384, 65536, 1_000_000])
    ap.add_argument("--ranks", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--chunks", type=int, nargs="+",
                    default=[1024, 2048, 4096, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("als_heavy_probe needs a GPU: timings elsewhere say nothing")
    emit(probe="knobs", heavy_min=als_ops.heavy_min(),
         heavy_chunk=als_ops.heavy_chunk(), device=torch.cuda.get_device_name())
    (run_sweep if args.what == "sweep" else run_zipf)(args)


if __name__ == "__main__":
    main()
