#!/usr/bin/env python
"""Nonnegative-ALS probe: what als_solve(nonnegative=True) costs
(csrc/als_nnls.hip) against the unconstrained half-step at the same commit.

  step      one implicit user half-step at the bench's shape (--rows rows
            of degree --degree over --cols columns, rank --rank, alpha 40,
            nonnegative factors on the fixed side): nonnegative off and on,
            alternating in one process after warm-up, and the solver's
            trips per row (mean, max, histogram) from its debug output.
  residual  max |A x - b| / |b|_inf of the unconstrained GPU als_solve
            against its own float64 system on the problems of
            tests/test_als_nnls_gpu.py::test_every_shape: the figure that
            test's KKT bound is four times.

Prints one JSON line per measurement. Times are host clocks around work
that ends in a device synchronise.
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from predictionio_amd.ops import als as als_ops  # noqa: E402

DEV = torch.device("cuda", 0)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_step(args):
    f = args.rank
    g = torch.Generator(device=DEV).manual_seed(args.seed)
    Y = (torch.randn((args.cols, f), generator=g, device=DEV) / f ** 0.5).abs()
    yty = als_ops.gramian(Y)
    indptr = torch.arange(args.rows + 1, device=DEV,
                          dtype=torch.int64) * args.degree
    cols = torch.randint(0, args.cols, (args.rows * args.degree,),
                         generator=g, device=DEV, dtype=torch.int32)
    vals = torch.ones(cols.numel(), device=DEV)
    out = torch.empty((args.rows, f), device=DEV)
    iters = torch.zeros(args.rows, dtype=torch.int32, device=DEV)
    lv = als_ops.prepare_lv(Y, yty, args.lam)

    def off():
        als_ops.als_solve(indptr, cols, vals, Y, YtY=yty, lam=args.lam,
                          alpha=40.0, implicit=True, lv=lv, out=out)

    def on():
        als_ops.als_solve(indptr, cols, vals, Y, YtY=yty, lam=args.lam,
                          alpha=40.0, implicit=True, out=out,
                          nonnegative=True, nnls_iters=iters)

    t = {"off": [], "on": []}
    off(), on()
    for _ in range(args.reps):
        t["off"].append(timed(off))
        t["on"].append(timed(on))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    emit(probe="step", f=f, rows=args.rows, degree=args.degree,
         cols=args.cols, reps=args.reps,
         seconds={k: [round(s, 4) for s in v] for k, v in t.items()},
         median_seconds={k: round(s, 4) for k, s in med.items()},
         ratio_on_over_off=round(med["on"] / med["off"], 2),
         trips_mean=round(iters.float().mean().item(), 3),
         trips_max=int(iters.max()),
         trips_hist=torch.bincount(iters).tolist(),
         zero_fraction=round((out == 0).float().mean().item(), 4))


def run_residual(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_als_nnls_gpu as t
    from _als_solve_oracle import ALPHA, LAM
    worst = 0.0
    for f in (10, 32, 64, 128):
        for implicit in (False, True):
            for abs_y in (False, True):
                _, indptr, cols, vals, Y, _ = t.shape_problem(f, implicit,
                                                              abs_y)
                X = als_ops.als_solve(indptr.cuda(), cols.cuda(), vals.cuda(),
                                      Y.cuda(), lam=LAM, alpha=ALPHA,
                                      implicit=implicit).cpu().double()
                Yd = Y.double()
                yty = als_ops.gramian(Yd)
                case = 0.0
                for r in range(X.shape[0]):
                    A, b = als_ops.normal_equations(
                        indptr, cols, vals, Yd, yty, LAM, ALPHA, implicit,
                        not implicit, r)
                    s = b.abs().max().item()
                    if s:
                        case = max(case,
                                   ((A @ X[r] - b).abs().max() / s).item())
                emit(probe="residual", f=f, implicit=implicit, abs_y=abs_y,
                     max_rel_residual=case)
                worst = max(worst, case)
    emit(probe="residual", worst=worst)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["step", "residual"])
    ap.add_argument("--rows", type=int, default=12_500_000)
    ap.add_argument("--cols", type=int, default=10_000_000)
    ap.add_argument("--degree", type=int, default=20)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--lam", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("als_nnls_probe needs a GPU: timings elsewhere say nothing")
    emit(probe="knobs", max_it=als_ops.NNLS_REF_MAX_IT,
         heavy_min=als_ops.heavy_min(), device=torch.cuda.get_device_name())
    (run_step if args.what == "step" else run_residual)(args)


if __name__ == "__main__":
    main()
