"""Row addressing of every kernel past the 2, 4 and 8 GiB offsets.

The matrices have N = 2^24 + 64 rows and are zero but for the planted
rows of _large_offsets.py; tests/test_large_offsets_cpu.py shows that a
byte offset or an element index narrowed to 32 bits changes every result
asserted here. 4 GiB tier: fp32 F = 64 (256 B rows); bf16 F = 128 for the
MFMA kernel, where the 4 GiB offset is also element 2^31. 8 GiB tier:
fp32 F = 128, whose last 64 rows lie past element 2^31.

Expected values are exact by construction (small integers) except for
the ALS solves, which are compared bit for bit with the same solve
against a compact matrix holding only the referenced rows, and within
the solver tests' TOL with the float64 reference.

One big matrix is alive at a time (the `pool` fixture); no test holds
more than 13 GiB. Every test prints its peak device memory and time.
"""

import gc
import math
import time

import pytest
import torch

import _large_offsets as lo
from _als_solve_oracle import ALPHA, LAM, TOL, _ref64
from predictionio_amd.ops import als as als_ops
from predictionio_amd.ops import ranking
from predictionio_amd.ops import topk as topk_ops

pytestmark = pytest.mark.gpu

GIB = lo.GIB
N = lo.N_ROWS
CAP = 13 * GIB
I32, I64 = torch.int32, torch.int64


def _free_all():
    gc.collect()
    torch.cuda.empty_cache()


def _need(nbytes):
    """The skip rule: run unless the device has less than 1.25 x need."""
    assert nbytes <= CAP
    _free_all()
    free = torch.cuda.mem_get_info()[0]
    if free < 1.25 * nbytes:
        msg = (f"needs {nbytes / GIB:.1f} GiB x 1.25, "
               f"{free / GIB:.1f} GiB free")
        print("SKIP:", msg)
        pytest.skip(msg)


class Pool:
    """The one big [N, F] matrix alive at a time, zero but for `rows`."""

    def __init__(self):
        self.key = self.mat = self.rows = None

    def release(self):
        self.key = self.mat = self.rows = None
        _free_all()

    def get(self, f, dtype, rows, vals, extra=0):
        """rows: int64 [P] (CPU), vals [P, F]. extra: bytes the caller
        will hold next to the matrix."""
        key = (f, dtype)
        if self.key != key:
            self.release()
            _need(N * f * dtype.itemsize + extra)
            self.mat = torch.zeros((N, f), dtype=dtype, device="cuda")
            self.key = key
        elif self.rows is not None:
            self.mat[self.rows] = 0
        self.rows = rows.cuda()
        self.mat[self.rows] = vals.to(dtype).cuda()
        return self.mat

    def planted(self, tier_name, extra=0):
        tier = lo.TIERS[tier_name]
        p = lo.Planted(tier)
        dtype = torch.float32 if tier.esize == 4 else torch.bfloat16
        return p, self.get(tier.f, dtype, *p.dense_rows(), extra=extra)


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.release()


@pytest.fixture(autouse=True)
def _report(request):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"\n[large-offsets] {request.node.name}: peak "
          f"{peak / GIB:.2f} GiB, {time.perf_counter() - t0:.2f} s")
    assert peak <= CAP


def _queries(B, f, dtype=torch.float32):
    """Query b is (1 + b % 3) * ones: scores scale, their order stays."""
    m = [1 + b % 3 for b in range(B)]
    return m, (torch.tensor(m, dtype=torch.float32)[:, None]
               * torch.ones((B, f))).to(dtype).cuda()


def _csr(lists, dtype=I32):
    ip = torch.tensor([0] + [len(c) for c in lists]).cumsum(0)
    ci = torch.tensor([j for c in lists for j in c], dtype=dtype)
    return ip.cuda(), ci.cuda()


def _ids(p):
    return p.rows + [p.rows[0] + 1, N - 2]      # two zero rows


def _assert_topk(got, want, mults):
    gv, gi = got[0].cpu(), got[1].cpu()
    assert gv.dtype == torch.float32 and gi.dtype == torch.int64
    for b, m in enumerate(mults):
        assert gi[b].tolist() == [j for _, j in want[b]], b
        assert gv[b].tolist() == [float(s) for s, _ in want[b]], b


# ------------------------------------------------------------------ top-K

@pytest.mark.parametrize("n_slices", [None, 997])
@pytest.mark.parametrize("tier", ["fp32_f64", "fp32_f128"])
def test_topk_fp32_kernel(pool, tier, n_slices):
    """topk_score_kernel with item_mask [N] and item_cats [N, 4]: the
    best row is masked, the second best carries a category bit that only
    the even queries accept. Row N - 1 sits in a tail chunk."""
    W, K, B = 4, 10, 65
    p, Y = pool.planted(tier, extra=N * (4 * W + 1))
    best = sorted(p.positive(), key=lambda r: -p.score1[r])
    mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
    mask[best[0]] = 1
    cats = torch.ones((N, W), dtype=I32, device="cuda")
    cats[best[1]] = torch.tensor([0, 0, 32, 0], dtype=I32, device="cuda")
    mults, Xq = _queries(B, p.tier.f)
    qc = torch.tensor([[31, 31, 31 + 32 * (b % 2 == 0), 31]
                       for b in range(B)], dtype=I32).cuda()
    want = [lo.op_topk(lo.View(p), K, (m,),
                       banned={best[0]} | ({best[1]} if b % 2 else set()))[0]
            for b, m in enumerate(mults)]
    assert all(N - 1 in [j for _, j in w] for w in want)
    got = topk_ops.topk_score(Xq, Y, K, item_mask=mask, item_cats=cats,
                              query_cats=qc, mode="fp32", n_slices=n_slices)
    _assert_topk(got, want, mults)


@pytest.mark.parametrize("interleave", [False, True])
def test_mfma_raw_slice_lists(pool, interleave):
    """topk_mfma_kernel through the raw binding on bf16 F = 128: every
    slice's list holds exactly the planted positive rows of that slice."""
    from predictionio_amd.ops import hip_ext
    L, S, B = 32, 1536, 17
    p, Y = pool.planted("bf16_f128")
    mults, Xq = _queries(B, 128, torch.bfloat16)
    vals, idxs = hip_ext().topk_score_mfma(
        Xq, Y, L, S, None, None, None, 0, interleave=interleave,
        gth=False if interleave else None)
    vals = vals.view(B, S, L).cpu()
    idxs = idxs.view(B, S, L).cpu()
    want = lo.op_slice_lists(lo.View(p), S, interleave)
    assert sum(len(v) for v in want.values()) == len(p.positive())
    assert len(want) >= 3                       # one per band at least
    for b, m in enumerate(mults):
        pos = vals[b] > 0
        assert int(pos.sum()) == len(p.positive()), b
        for s, exp in want.items():
            got = sorted(zip(idxs[b, s][pos[s]].tolist(),
                             vals[b, s][pos[s]].tolist()))
            assert got == [(j, float(m * v)) for j, v in exp], (b, s)
    # what is not planted scores 0 or is an empty slot
    assert bool(((vals == 0) | (vals < -1e38) | (vals > 0)).all())


@pytest.mark.parametrize("route", ["default", "union", "list"])
def test_public_routes(pool, route, monkeypatch):
    """topk_score at F = 64: the bf16 copy crosses 2 GiB, the fp32
    re-score gathers past 4 GiB."""
    K, B = 10, 65
    p, Y = pool.planted("fp32_f64", extra=N * 64 * 2 + N)
    best = max(p.positive(), key=lambda r: p.score1[r])
    mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
    mask[best] = 1
    mults, Xq = _queries(B, 64)
    want = [lo.op_topk(lo.View(p), K, (m,), banned={best})[0] for m in mults]
    kw = {}
    if route == "union":
        kw["mode"] = "union"
    if route == "list":
        monkeypatch.setenv("PIO_TOPK_UNION", "0")
    before = topk_ops.union_stats()
    got = topk_ops.topk_score(Xq, Y, K, item_mask=mask, **kw)
    after = topk_ops.union_stats()
    assert after["calls"] - before["calls"] == (0 if route == "list" else 1)
    assert after["flagged"] == before["flagged"]
    _assert_topk(got, want, mults)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("tier", ["fp32_f64", "fp32_f128"])
def test_rescore_binding(pool, tier, misaligned):
    from predictionio_amd.ops import hip_ext
    p = lo.Planted(lo.TIERS[tier])
    f = p.tier.f
    if misaligned:      # a view 4 bytes off: the one-float-per-lane loads
        pool.release()
        _need(N * f * 4 + 4)
        buf = torch.zeros(N * f + 1, device="cuda")
        Y = buf[1:].view(N, f)
        ids, vals = p.dense_rows()
        Y[ids.cuda()] = vals.cuda()
        assert Y.data_ptr() % 16 == 4
    else:
        _, Y = pool.planted(tier)
    B = 5
    mults, Xq = _queries(B, f)
    ids = _ids(p)
    idx = torch.tensor([ids[b:] + ids[:b] + [-1] for b in range(B)],
                       dtype=I32).cuda()
    out = hip_ext().topk_rescore(Xq, Y, idx).cpu()
    for b, m in enumerate(mults):
        row = ids[b:] + ids[:b]
        want = [float(s) for s in lo.op_gather_dots(lo.View(p), row, m)]
        assert out[b].tolist() == want + [float("-inf")], b
    del Y


@pytest.mark.parametrize("K", [8, 65])
@pytest.mark.parametrize("tier", ["fp32_f64", "fp32_f128"])
def test_candidate_lists(pool, tier, K):
    """topk_cand_kernel, top-K (K = 8) and scores mode (K = 65)."""
    p, Y = pool.planted(tier)
    mults, Xq = _queries(3, p.tier.f)
    ids = sorted(_ids(p))
    lists = [ids, ids[::2], ids[1:]]
    ip, ci = _csr(lists)
    gv, gi = topk_ops.topk_score(Xq, Y, K, cand_indptr=ip.long(),
                                 cand_indices=ci)
    gv, gi = gv.cpu(), gi.cpu()
    for b, m in enumerate(mults):
        sc = lo.op_gather_dots(lo.View(p), lists[b], m)
        order = sorted(zip(sc, lists[b]), key=lambda e: (-e[0], e[1]))[:K]
        pad = K - len(order)
        assert gi[b].tolist() == [j for _, j in order] + [-1] * pad, b
        assert gv[b].tolist() == [float(s) for s, _ in order] \
            + [float("-inf")] * pad, b


# ---------------------------------------------------------- held-out ranks

@pytest.mark.parametrize("tier", ["fp32_f64", "fp32_f128"])
def test_heldout_ranks(pool, tier):
    """Targets and seen items in every band; the zero-score target ties
    with all the unplanted rows, a count of about 2^24."""
    f = lo.TIERS[tier].f
    p, Y = pool.planted(tier, extra=GIB // 4)
    mults, X = _queries(2, f)
    t0 = sorted(p.rows[1::2] + [p.rows[0] + 1])
    s0 = p.rows[0::4]
    t1 = sorted([r for r in p.rows if r >= p.tier.r2] + [N - 2])
    tp, ti = _csr([t0, t1])
    sp, si = _csr([s0, []])
    want = lo.op_rank_counts(lo.View(p), t0, s0, mults[0]) \
        + lo.op_rank_counts(lo.View(p), t1, [], mults[1])
    assert max(e for _, e in want) > 2 ** 24 - 64
    for n_slices in (None, 7):
        gt, eq, nc = ranking.heldout_ranks(X, Y, tp.long(), ti, sp.long(),
                                           si, n_slices=n_slices)
        assert list(zip(gt.tolist(), eq.tolist())) == want, n_slices
        assert nc.tolist() == [N - len(s0), N]


# -------------------------------------------------------------------- ALS

def test_residual_sums_large_y(pool):
    p, Y = pool.planted("fp32_f64")
    ids = _ids(p)
    mults, X = _queries(2, 64)
    indptr = [0, 3, len(ids)]
    values = [float(1 + q % 4) for q in range(len(ids))]
    A, B, pred_w = lo.op_loss(lo.View(p), mults, indptr, ids, values)
    pred = torch.full((len(ids),), float("nan"), device="cuda")
    sums = als_ops.als_residual_sums(
        torch.tensor(indptr).cuda(), torch.tensor(ids, dtype=I32).cuda(),
        torch.tensor(values).cuda(), X, Y, pred=pred)
    assert sums.tolist() == [float(A), float(B)]
    assert pred.tolist() == [float(s) for s in pred_w]


def test_residual_sums_large_x(pool):
    """n_rows = N: the planted rows are the CSR's non-empty rows."""
    p, X = pool.planted("fp32_f64", extra=N * 8 * 3)
    Ys = (torch.arange(1, 4).float()[:, None] * torch.ones((3, 64))).cuda()
    rows = sorted(p.rows + [p.rows[0] + 1])
    counts = torch.zeros(N, dtype=I64, device="cuda")
    counts[torch.tensor(rows).cuda()] = 2
    indptr = torch.zeros(N + 1, dtype=I64, device="cuda")
    torch.cumsum(counts, 0, out=indptr[1:])
    del counts
    cols = [0, 2] * len(rows)
    values = [float(1 + q % 5) for q in range(len(cols))]
    pred_w = [p.score1.get(r, 0) * (c + 1)
              for r in rows for c in (0, 2)]
    A = sum((v - s) ** 2 for v, s in zip(values, pred_w))
    B = sum(s * s for s in pred_w)
    pred = torch.full((len(cols),), float("nan"), device="cuda")
    sums = als_ops.als_residual_sums(
        indptr, torch.tensor(cols, dtype=I32).cuda(),
        torch.tensor(values).cuda(), X, Ys, pred=pred)
    assert sums.tolist() == [float(A), float(B)]
    assert pred.tolist() == [float(s) for s in pred_w]


@pytest.mark.parametrize("tier", ["fp32_f64", "fp32_f128"])
def test_row_transform_in_place(pool, tier):
    """out aliases in: planted rows become y W exactly, every other row
    stays exactly 0 (min and max over the whole matrix)."""
    p, Y = pool.planted(tier)
    W = lo.xform_matrix(p.tier.f)
    out = als_ops.row_transform(Y, W.float().cuda(), out=Y)
    assert out.data_ptr() == Y.data_ptr()
    ids, vals = p.dense_rows(torch.float64)
    assert torch.equal(Y[ids.cuda()].cpu().double(), vals @ W)
    Y[ids.cuda()] = 0
    mn, mx = torch.aminmax(Y)
    assert float(mn) == 0.0 and float(mx) == 0.0
    pool.rows = None    # the matrix is all zero again


SOLVE_DEGREES = [20, 24, 32, 40, 48, 49, 100]


def _solve_problem(tier, seed):
    """Referenced rows in every band (the planted rows and 30 random rows
    per band), a compact random Y over them and a CSR with one row per
    degree; returns (rows [R], Yc [R, f], indptr, compact cols, vals)."""
    g = torch.Generator().manual_seed(seed)
    edges = [0] + tier.thresholds() + [tier.n]
    rows = set(lo.planted_rows(tier))
    for a, b in zip(edges[:-1], edges[1:]):
        rows |= set((a + torch.randperm(b - a, generator=g)[:30]).tolist())
    rows = torch.tensor(sorted(rows))
    R = rows.numel()
    Yc = (torch.randn((R, tier.f), generator=g) / math.sqrt(tier.f)).float()
    cols = torch.cat([torch.randint(0, R, (n,), generator=g)
                      for n in SOLVE_DEGREES]).to(I32)
    vals = (torch.rand(cols.numel(), generator=g) * 3 + 0.5).float()
    indptr = torch.tensor([0] + SOLVE_DEGREES).cumsum(0)
    return rows, Yc, indptr, cols, vals


@pytest.mark.parametrize("tier,implicit", [("fp32_f64", False),
                                           ("fp32_f64", True),
                                           ("fp32_f128", False)])
def test_solve_gathers_from_every_band(pool, tier, implicit):
    """als_woodbury_kernel (degrees 20 .. 48), the dense kernels (49,
    100): Y rows gathered by column ids in every band."""
    t = lo.TIERS[tier]
    rows, Yc, indptr, cols, vals = _solve_problem(t, 77)
    assert {t.band(int(r)) for r in rows[cols.long()]} >= \
        {t.band(int(r)) for r in rows}
    extra = N * t.f * 4 if implicit else 0      # the whitened copy
    Y = pool.get(t.f, torch.float32, rows, Yc, extra=extra)
    big_cols = rows[cols.long()].to(I32)
    kw = dict(lam=LAM, alpha=ALPHA, implicit=implicit)
    ip, vv = indptr.cuda(), vals.cuda()
    Xc = als_ops.als_solve(ip, cols.cuda(), vv, Yc.cuda(), **kw)
    Xb = als_ops.als_solve(ip, big_cols.cuda(), vv, Y, **kw)
    X64 = _ref64(indptr, cols, vals, Yc, LAM, implicit)
    for name, X in (("compact", Xc), ("large", Xb)):
        assert torch.allclose(X.cpu().double(), X64, atol=TOL, rtol=TOL), \
            name
    if not implicit:
        assert torch.equal(Xb, Xc)


@pytest.mark.parametrize("implicit", [False, True])
def test_solve_output_rows_past_4gib(pool, implicit):
    """n_rows = N at F = 64: X (and Z) rows written past 4 GiB, the block
    scan over 2^24 row pointers. Non-empty rows in every band match the
    compact solve bit for bit, all others are exactly 0, no NaN is left."""
    from _als_solve_oracle import _factors
    pool.release()
    f = 64
    _need(N * f * 4 * (2 if implicit else 1) + N * 8 * 3)
    g = torch.Generator().manual_seed(5)
    rows = lo.planted_rows(lo.TIERS["fp32_f64"])
    sizes = [SOLVE_DEGREES[i % len(SOLVE_DEGREES)] for i in range(len(rows))]
    Y = _factors(f, g).cuda()
    cols = torch.cat([torch.randint(0, Y.shape[0], (n,), generator=g)
                      for n in sizes]).to(I32).cuda()
    vals = (torch.rand(sum(sizes), generator=g) * 3 + 0.5).float().cuda()
    small_ip = torch.tensor([0] + sizes).cumsum(0).cuda()
    rows_d = torch.tensor(rows).cuda()
    counts = torch.zeros(N, dtype=I64, device="cuda")
    counts[rows_d] = torch.tensor(sizes).cuda()
    indptr = torch.zeros(N + 1, dtype=I64, device="cuda")
    torch.cumsum(counts, 0, out=indptr[1:])
    del counts
    kw = dict(lam=LAM, alpha=ALPHA, implicit=implicit)
    if implicit:
        kw["YtY"] = als_ops.gramian(Y)
    Xc = als_ops.als_solve(small_ip, cols, vals, Y, **kw)
    out = torch.full((N, f), float("nan"), device="cuda")
    res = als_ops.als_solve(indptr, cols, vals, Y, out=out, **kw)
    assert res.data_ptr() == out.data_ptr()
    assert torch.equal(out[rows_d], Xc)
    assert bool(Xc.abs().sum(1).min() > 0)
    out[rows_d] = 0
    mn, mx = torch.aminmax(out)
    assert float(mn) == 0.0 and float(mx) == 0.0    # NaN would show here
    del out, res, indptr
