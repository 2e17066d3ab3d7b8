"""ALS training objective across ranks (CPU, gloo, world_size=2).

Modelled on test_dist_gloo.py: spawned workers, a rendezvous port of
their own, and the spawn helper's queue timeout as the guard against a
hang.
"""

import multiprocessing as mp
import os

import torch

# World 2 and a single process solve the same systems; they differ in
# the summation order of the all-reduced Gramians and of the loss sums,
# and in fp32 rounding of the per-row solves. test_dist_gloo.py holds
# the FACTORS of the two to FACTOR_TOL (atol = rtol, literals in its
# asserts); at a minimum of the objective a factor change moves the
# loss in second order only, so the loss is held to 1e-6 relative.
FACTOR_TOL = 1e-4
LOSS_RTOL = 1e-6

N_USERS, N_ITEMS, NNZ, F = 60, 40, 700, 16
LAM, ALPHA = 0.05, 2.0


def _run_worker(rank, world, port, fn_name, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        result = globals()[fn_name](rank, world)
        q.put((rank, "ok", result))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _spawn(fn_name, port, world=2):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_worker,
                         args=(r, world, port, fn_name, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, status, payload = q.get(timeout=120)
        assert status == "ok", f"rank {rank} failed:\n{payload}"
        results[rank] = payload
    for p in procs:
        p.join(timeout=30)
    return results


def _trainer(implicit, **kw):
    """A trainer on this rank's blocks of the 60 x 40 problem, with a
    fixed global init (init_factors seeds per rank)."""
    from predictionio_amd.models.als import ALSParams, ALSTrainer
    g = torch.Generator().manual_seed(20)
    cells = torch.randperm(N_USERS * N_ITEMS, generator=g)[:NNZ]
    users = (cells // N_ITEMS).to(torch.int32)
    items = (cells % N_ITEMS).to(torch.int32)
    ratings = torch.randint(1, 6, (NNZ,), generator=g).float()
    kw.setdefault("iterations", 2)
    p = ALSParams(rank=F, lambda_=LAM, alpha=ALPHA, implicit=implicit,
                  seed=0, **kw)
    t = ALSTrainer(p, N_USERS, N_ITEMS, torch.device("cpu"))
    t.set_ratings(users, items, ratings)
    gen = torch.Generator().manual_seed(99)
    X0 = torch.randn((N_USERS, F), generator=gen) / F ** 0.5
    Y0 = torch.randn((N_ITEMS, F), generator=gen) / F ** 0.5
    t.X = X0[t.u_lo:t.u_hi].clone()
    t.Y = Y0[t.i_lo:t.i_hi].clone()
    return t


def _loss_after_two_steps(implicit):
    t = _trainer(implicit)
    first = t.loss()       # before any step: loss() issues the gather
    t.step()               # ... and step() consumes that one
    t.step()
    out = t.loss()         # finishes the pipelined gather, keeps it
    again = t.loss()
    assert again == out
    X, Y = t.gather_factors()   # must still see the finished gather
    assert X.shape == (N_USERS, F) and Y.shape == (N_ITEMS, F)
    assert torch.isfinite(Y).all()
    return first, out, Y


def _dist_loss(rank, world):
    res = {}
    for implicit in (False, True):
        first, out, Y = _loss_after_two_steps(implicit)
        res[implicit] = (first, out, Y.tolist())
    return res


def _dist_tol(rank, world):
    res = {}
    for implicit in (False, True):
        t = _trainer(implicit, iterations=12, tol=0.05)
        X, Y = t.fit()
        assert X.shape == (N_USERS, F) and Y.shape == (N_ITEMS, F)
        res[implicit] = [(h["iteration"], h["loss"])
                         for h in t.loss_history]
    return res


def test_world2_loss_matches_single_process():
    res = _spawn("_dist_loss", port=29651)
    for implicit in (False, True):
        first0, out0, Y0 = res[0][implicit]
        first1, out1, Y1 = res[1][implicit]
        # the identical Python floats on both ranks
        assert first0 == first1 and out0 == out1
        assert Y0 == Y1
        sfirst, sout, sY = _loss_after_two_steps(implicit)
        assert set(out0) == set(sout)
        assert out0["nnz"] == sout["nnz"] == NNZ
        for got, want in ((first0, sfirst), (out0, sout)):
            # sq_err is one part of the loss: the same absolute bound
            for key in ("loss", "sq_err"):
                rel = abs(got[key] - want[key]) / abs(want["loss"])
                print(implicit, key, got[key], want[key], rel)
                assert rel <= LOSS_RTOL
        # loss() left the factors what test_dist_gloo.py holds them to
        assert torch.allclose(torch.tensor(Y0), sY, atol=FACTOR_TOL,
                              rtol=FACTOR_TOL)


def test_tol_stops_both_ranks_together():
    res = _spawn("_dist_tol", port=29653)
    for implicit in (False, True):
        h0, h1 = res[0][implicit], res[1][implicit]
        assert h0 == h1
        k = len(h0)
        assert 1 < k < 12
        assert [it for it, _ in h0] == list(range(1, k + 1))
        # stopped at the first evaluation that improved by <= 5 %
        rel = [(a[1] - b[1]) / abs(a[1]) for a, b in zip(h0, h0[1:])]
        assert all(r > 0.05 for r in rel[:-1]) and rel[-1] <= 0.05
