#!/usr/bin/env python3
"""Indicator serving: the fused kernel vs the torch route vs predict()
(docs/KERNELS.md "Indicator top-K").

Workload: a random indicator table of N items x n float scores, K = 20,
every query sums the rows of its own `--query-items` random items, the
query's items excluded. For each B:

  (a) kernel   ONE indicator_topk call (csrc/indicator_topk.hip)
  (b) torch    ONE indicator_topk_ref call on the same device
  (c) predict  CooccurrenceAlgorithm.predict in a loop over the first
               --predict-queries queries, once, for scale (host dicts)

(a) and (b) are the median of --repeats device-synchronized runs after
--warmup runs of the same shape, alternating in one process; both skip
the table scan (check_table=False), as the template does, and must agree
bit for bit before they are timed. --rehearse runs tiny shapes on the CPU
to check the harness only.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--query-items", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+",
                    default=[64, 1024, 16384])
    ap.add_argument("--predict-queries", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()

    import torch
    from predictionio_amd.data.bimap import BiMap
    from predictionio_amd.controller import Params
    from predictionio_amd.ops.cooccurrence import (
        indicator_topk, indicator_topk_ref,
    )
    from predictionio_amd.templates.similarproduct.engine import (
        CooccurrenceAlgorithm, CooccurrenceModel, Query,
    )

    if args.rehearse:
        dev = torch.device("cpu")
        args.items, args.batches, args.predict_queries = 5000, [4, 16], 8
        args.warmup, args.repeats = 1, 2
    else:
        if not torch.cuda.is_available():
            sys.exit("indicator_serve_bench needs a GPU (or --rehearse)")
        dev = torch.device("cuda", 0)
        from predictionio_amd.ops import hip_ext
        hip_ext()  # the native extension must be there

    N, n, K, m = args.items, args.n, args.k, args.query_items
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, N, (N, n), generator=g, dtype=torch.int32).to(dev)
    sc = (torch.rand((N, n), generator=g) * 20).to(dev)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def once(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    def queries(B):
        # sorted draws plus 0..m-1: strictly ascending rows below N
        rows = torch.randint(0, N - m, (B, m), generator=g).sort(1).values
        rows = (rows + torch.arange(m)).to(torch.int32)
        return (torch.arange(B + 1, dtype=torch.int64, device=dev) * m,
                rows.reshape(-1).to(dev), rows)

    results = []
    for B in args.batches:
        qp, qi, _ = queries(B)

        def kernel():
            return indicator_topk(ids, sc, qp, qi, K, check_table=False)

        def torch_route():
            return indicator_topk_ref(ids, sc, qp, qi, K, check_table=False)

        a, b = kernel(), torch_route()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), \
            "the two routes differ"
        for _ in range(args.warmup):
            kernel()
            torch_route()
        ta, tb = [], []
        for _ in range(args.repeats):      # alternate the two routes
            ta.append(once(kernel))
            tb.append(once(torch_route))
        row = {"N": N, "n": n, "K": K, "query_items": m, "B": B,
               "kernel_ms": round(statistics.median(ta) * 1e3, 3),
               "kernel_min_max_ms": [round(min(ta) * 1e3, 3),
                                     round(max(ta) * 1e3, 3)],
               "torch_ms": round(statistics.median(tb) * 1e3, 3),
               "torch_min_max_ms": [round(min(tb) * 1e3, 3),
                                    round(max(tb) * 1e3, 3)]}
        row["speedup"] = round(row["torch_ms"] / row["kernel_ms"], 2)
        print(json.dumps(row), flush=True)
        results.append(row)

    # predict(): host dicts, only the rows its queries touch
    P = args.predict_queries
    _, _, rows = queries(P)
    item_map = BiMap.string_int(f"i{k}" for k in range(N))
    touched = torch.unique(rows).long()
    t_ids, t_sc = ids[touched.to(dev)].cpu(), sc[touched.to(dev)].cpu()
    top_n = {int(r): list(zip(t_ids[k].tolist(), t_sc[k].tolist()))
             for k, r in enumerate(touched.tolist())}
    model = CooccurrenceModel(top_n, item_map, {})
    algo = CooccurrenceAlgorithm(Params({"n": n}))
    qs = [Query(items=[f"i{r}" for r in row], num=K) for row in rows.tolist()]
    t0 = time.perf_counter()
    for q in qs:
        algo.predict(model, q)
    row = {"predict_queries": P,
           "predict_loop_ms": round((time.perf_counter() - t0) * 1e3, 3)}
    print(json.dumps(row), flush=True)
    results.append(row)

    if args.rehearse:
        print("rehearsal on the CPU: harness check only, not a measurement")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": str(dev), "results": results}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
