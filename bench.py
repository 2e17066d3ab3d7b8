#!/usr/bin/env python3
"""Flagship benchmark: ALS rank=64 implicit training (BASELINE.json config 4)
and batched top-K serving (config 5) on MI355X.

North-star metric (BASELINE.json): "ALS sec/iter + recs/sec (whole node),
rank=64 implicit 100M users x 10M items at 1/2/4/8 GPU". Weak scaling:
12.5M users x 20 ratings per GPU, 10M items fixed, synthetic uniform events,
random-init factors (there is no network for datasets).

Launch (driver contract):
  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  # N>1 via: python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
  #   --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One step = one full ALS iteration (user half-step + item half-step), each
half-step = RCCL all-gather of the fixed factor side + one fused HIP
Gramian+Cholesky solve over the local row block. Nothing is skipped inside
the timed region (both collectives + both solves + YtY GEMMs). fp32 compute.

A plain run only sets up, warms up, times the K steps and prints the JSON
result line. --dump-outputs DIR additionally writes what the last timed step
computed as DIR/<name>.npy; --full additionally co-measures the config-5
serve metric after a train-mode run (reported under `extra_metrics`).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

# --dump-outputs budget: 64 MB over all files. A factor matrix larger than
# its share is written as a fixed, seeded sample of whole rows.
DUMP_BUDGET_BYTES = 64 * 1000 * 1000


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench] {msg}", file=sys.stderr, flush=True)


def synth_shard(trainer, nnz_per_user: int, seed: int, device):
    """Generate this rank's synthetic user-block ratings (uniform items,
    implicit weight 1.0) and exchange to build the item-block shard."""
    from predictionio_amd.parallel import dist as pdist

    n_local_users = trainer.u_hi - trainer.u_lo
    nnz = n_local_users * nnz_per_user
    g = torch.Generator(device="cpu").manual_seed(seed + pdist.get_rank())
    # generate on device in chunks to bound host memory
    users = torch.arange(n_local_users, dtype=torch.int32, device=device) \
        .repeat_interleave(nnz_per_user)
    items = torch.randint(0, trainer.n_items, (nnz,), generator=g,
                          dtype=torch.int32).to(device)
    vals = torch.ones(nnz, dtype=torch.float32, device=device)
    # item-major shard: every triple whose item falls in this rank's item
    # block, from all ranks (the Spark-shuffle replacement; global user ids).
    # exchange_triples partitions by its `cols` argument → pass items there.
    g_users = (users.to(torch.int64) + trainer.u_lo).to(torch.int32)
    it_u, it_i, it_v = pdist.exchange_triples(g_users, items, vals,
                                              trainer.n_items)
    return (users, items, vals), (it_i, it_u, it_v)


def sample_rows(n_rows: int, max_rows: int, seed: int):
    """Sorted row ids to dump: all rows when they fit, else a seeded
    sample without replacement (the same ids for the same arguments)."""
    if n_rows <= max_rows:
        return np.arange(n_rows, dtype=np.int64)
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n_rows, size=max_rows, replace=False))


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """Write each array as <out_dir>/<name>.npy (float32 or float64)."""
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        total += a.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)
    assert total <= DUMP_BUDGET_BYTES, total
    log(f"dumped {len(arrays)} arrays ({total / 1e6:.1f} MB) to {out_dir}")


def run_train(args, device):
    from predictionio_amd.models.als import ALSParams, ALSTrainer
    from predictionio_amd.parallel import dist as pdist

    world = pdist.get_world_size()
    n_users = args.users_per_gpu * world
    n_items = args.items
    p = ALSParams(rank=args.rank, iterations=args.steps,
                  lambda_=args.lambda_, alpha=args.alpha,
                  implicit=args.implicit, seed=args.seed)
    trainer = ALSTrainer(p, n_users, n_items, device)
    log(f"generating synthetic shard: {args.users_per_gpu} users/GPU x "
        f"{args.nnz_per_user} ratings, {n_items} items, rank {args.rank}")
    t0 = time.time()
    (u, i, v), (ii, iu, iv) = synth_shard(trainer, args.nnz_per_user,
                                          args.seed, device)
    # install shards: user-major rows are local users; item-major rows are
    # local items (convert global item ids to local)
    trainer.set_ratings_sharded(
        (u, i, v), (ii - trainer.i_lo, iu, iv))
    del u, i, v, ii, iu, iv
    trainer.init_factors()
    if device.type == "cuda":
        torch.cuda.synchronize()
    log(f"setup done in {time.time() - t0:.1f}s; local nnz="
        f"{trainer.local_nnz()}")

    def sync():
        pdist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()

    for w in range(args.warmup):
        trainer.step()
    sync()
    trainer.phase_times = {"gather_s": 0.0, "solve_s": 0.0}
    t0 = time.time()
    for k in range(args.steps):
        trainer.step()
    sync()
    elapsed = time.time() - t0
    elapsed = pdist.max_scalar(elapsed)  # slowest rank
    sec_per_iter = elapsed / args.steps
    if os.environ.get("PIO_PHASE_TIMES") == "1":
        pt = trainer.phase_times
        log(f"phase times over timed steps: gather {pt['gather_s']:.3f}s "
            f"solve {pt['solve_s']:.3f}s")
    if args.dump_outputs and pdist.get_rank() == 0:
        # the factors a caller of step() reads back after the last timed
        # iteration (this rank's row blocks). Row ids ride along as
        # float64 so a sampled dump says which rows it holds.
        arrays = {}
        per_row = args.rank * 4 + 8
        for name, fac, sd in (("user_factors", trainer.X, args.seed),
                              ("item_factors", trainer.Y, args.seed + 1)):
            rows = sample_rows(fac.shape[0],
                               DUMP_BUDGET_BYTES // 2 // per_row, sd)
            idx = torch.from_numpy(rows).to(device)
            arrays[name] = fac.index_select(0, idx).float().cpu().numpy()
            arrays[name + "_rows"] = rows.astype(np.float64)
        dump_outputs(args.dump_outputs, arrays)
    total_nnz = args.users_per_gpu * args.nnz_per_user * world
    value = total_nnz / sec_per_iter  # ratings solved per second per iter
    return value, sec_per_iter, {
        "model": f"als_rank{args.rank}_"
                 f"{'implicit' if args.implicit else 'explicit'}",
        "global_batch": total_nnz,
        "users": n_users, "items": n_items,
        "nnz_per_user": args.nnz_per_user,
        "sec_per_iter": sec_per_iter,
        "parallelism": f"dp{world}",
    }


def run_serve(args, device):
    """Config 5: batched top-K serving with blacklist masks over item-block
    sharded factors; value = recommendations (user-queries) served /s."""
    from predictionio_amd.ops import topk as topk_ops
    from predictionio_amd.parallel import dist as pdist

    world = pdist.get_world_size()
    n_items = args.items
    i_lo, i_hi = pdist.block_bounds(n_items, world, pdist.get_rank())
    g = torch.Generator().manual_seed(args.seed)
    Y_local = (torch.randn((i_hi - i_lo, args.rank), generator=g)
               .float().to(device))
    B, K = args.serve_batch, args.topk
    Xq = torch.randn((B, args.rank), generator=g).float().to(device)
    # per-user blacklists (seen items), ~30 each, sorted
    bans = torch.randint(0, i_hi - i_lo, (B, 30), generator=g).sort(1)[0]
    ban_indptr = torch.arange(0, 30 * (B + 1), 30, dtype=torch.int64)[:B + 1] \
        .to(device)
    ban_indices = bans.to(torch.int32).flatten().to(device)

    from predictionio_amd.parallel.serve import sharded_topk_score

    def one_batch():
        return sharded_topk_score(Xq, Y_local, K, item_base=i_lo,
                                  ban_indptr=ban_indptr,
                                  ban_indices=ban_indices)

    def sync():
        pdist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_batch()
    sync()
    res = None
    t0 = time.time()
    for _ in range(args.steps):
        res = one_batch()
    sync()
    elapsed = pdist.max_scalar(time.time() - t0)
    sec_per_batch = elapsed / args.steps
    if args.dump_outputs and pdist.get_rank() == 0 and res is not None:
        # the (values, global item ids) of the last timed batch; ids as
        # float64 (exact), -1 marks an unfilled slot
        rows = torch.from_numpy(sample_rows(
            B, DUMP_BUDGET_BYTES // (K * 12), args.seed)).to(device)
        dump_outputs(args.dump_outputs, {
            "topk_values": res[0].index_select(0, rows).float().cpu().numpy(),
            "topk_indices": res[1].index_select(0, rows).double().cpu()
            .numpy(),
        })
    value = B / sec_per_batch  # user-queries served per second (whole job)
    return value, sec_per_batch, {
        "model": f"als_rank{args.rank}_topk_serving",
        "global_batch": B, "items": n_items, "topk": K,
        "parallelism": f"itemshard{world}",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", choices=["train", "serve"], default="train")
    ap.add_argument("--users-per-gpu", type=int, default=12_500_000)
    ap.add_argument("--items", type=int, default=10_000_000)
    ap.add_argument("--nnz-per-user", type=int, default=20)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--lambda", dest="lambda_", type=float, default=0.01)
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--explicit", dest="implicit", action="store_false")
    ap.add_argument("--serve-batch", type=int, default=4096)
    ap.add_argument("--topk", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--cpu-small", action="store_true",
                    help="tiny CPU config for smoke testing")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as "
                         "DIR/<name>.npy (float32/float64, <= 64 MB in all)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline "
                         "figure (train mode: the co-measured serve metric)")
    ap.add_argument("--no-serve-extra", action="store_true",
                    help="with --full: skip the co-measured serve metric "
                         "in train mode")
    args = ap.parse_args()

    if args.cpu_small:
        args.users_per_gpu = 2000
        args.items = 1000
        args.nnz_per_user = 10

    from predictionio_amd.parallel import dist as pdist
    rank, world = pdist.init_from_env()
    if world != args.gpus and "WORLD_SIZE" in os.environ:
        args.gpus = world
    use_cuda = torch.cuda.is_available() and not args.cpu_small
    if use_cuda and world > 1:
        # more ranks than GPUs: init_from_env fell back to gloo and the
        # compute must follow the collectives to the CPU
        use_cuda = pdist.compute_device().type == "cuda"
    if use_cuda:
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        # the HIP extension must be present on a GPU box — fail loudly
        from predictionio_amd.ops import hip_ext
        hip_ext()
    else:
        device = torch.device("cpu")

    extra = None
    if args.mode == "train":
        value, spi, config = run_train(args, device)
        metric = "als_ratings_per_sec"
        unit = "ratings/s"
        # --full: co-measure the config-5 serve metric OUTSIDE the timed
        # train region so such records certify serving too (VERDICT r1
        # item 6); skipped on CPU smoke runs to stay fast
        if args.full and use_cuda and not args.no_serve_extra:
            sargs = argparse.Namespace(**vars(args))
            sargs.steps, sargs.warmup = 5, 2
            sargs.dump_outputs = None
            sval, sspb, sconf = run_serve(sargs, device)
            extra = {
                "serving_queries_per_sec": sval,
                "serve_ms_per_batch": sspb * 1000.0,
                "serve_config": sconf,
            }
    else:
        value, spi, config = run_serve(args, device)
        metric = "serving_queries_per_sec"
        unit = "queries/s"

    if rank == 0:
        out = {
            "metric": metric,
            "value": value,
            "unit": unit,
            "n_gpus": args.gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": spi * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32",
            "data": "synthetic",
            "config": config,
        }
        if extra is not None:
            out["extra_metrics"] = extra
        print(json.dumps(out), flush=True)

    if pdist.is_distributed():
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
