"""GPU tests for the opt-in ALS solver variants, the kernels that
launch_als_solve brings in under PIO_ALS_DUAL, PIO_ALS_STAGE_BF16,
PIO_ALS_MFMA_GRAMIAN and PIO_ALS_DENSE_SPLIT, and for the ranks that pad.

The switches are read on every launch (os.environ in ops/als.py, getenv
in the launcher and the binding), so each test sets them in-process with
monkeypatch after deleting all four. Every solve is the trainer's call:
als_ops.als_solve with lv = prepare_lv(...) computed under the same
switches (implicit mode) and a NaN-prefilled `out`.

A bf16-staged variant is never compared with the unstaged truth: rows it
stages are compared with a float64 oracle that reads the same staged
values (_als_solve_oracle.py), all other rows with the float64 normal
equations. On the rows R that a configuration sends to a non-default
kernel the relative Frobenius error must stay within 4x the default
kernels' error on the same rows (measured in the same process;
test_no_accuracy_regression anchors the default path). The margin covers
differences in arithmetic (IEEE divisions and another substitution order
in the dual kernel, two half-chains in the bf16 pair loop, the workgroup
kernel's tiled Gramian and panel Cholesky), not in design: a wrong lane,
a stale LDS row or a dropped item moves the figure by orders of
magnitude.

Which case of test_every_degree reaches which instantiation (F = the
case's f; every case holds every degree 0..40, 63, 64, 65, 100):

  dual,  either mode, f    als_woodbury2_kernel<F,20,-1> (n 0..20),
                           <F,24,20> (n 21..24)
  combo, implicit, f       als_woodbury2_kernel<F,20,-1,true>,
                           <F,24,20,true>, als_woodbury_kernel<F,32,24,true>
  combo, explicit, f       the dual kernels without BF16S (= dual)
  bf16s, implicit, f       als_woodbury_kernel<F,20,-1,true>,
                           <F,24,20,true>, <F,32,24,true>
  bf16g, either mode, 64   als_solve_wave_kernel<64,true> (n > 32)
  split36, f in 16/32/64   als_solve_kernel<F> on n > 36, the wave kernel
                           keeps 33..36
  split16, f in 16/32/64   als_solve_kernel<F> on n > 16, over Woodbury
                           rows 17..32 too
"""

import functools

import pytest
import torch

from _als_solve_oracle import (
    ALPHA, LAM, N_COLS, TOL, _ref64, _rel_fro, degenerate_problem,
    every_degree_problem, expected, mfma_gramian_staged_oracle,
    woodbury_staged_oracle,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

DUAL, BF16S = "PIO_ALS_DUAL", "PIO_ALS_STAGE_BF16"
BF16G, SPLIT = "PIO_ALS_MFMA_GRAMIAN", "PIO_ALS_DENSE_SPLIT"
SWITCHES = (DUAL, BF16S, BF16G, SPLIT)
CONFIGS = {
    "default": {},
    "dual": {DUAL: "1"},
    "bf16s": {BF16S: "1"},
    "combo": {DUAL: "1", BF16S: "1"},   # the documented pair
    "bf16g": {BF16G: "1"},
    "split36": {SPLIT: "36"},
    "split16": {SPLIT: "16"},
}
MARGIN = 4.0


def _switch(monkeypatch, cfg):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in CONFIGS[cfg].items():
        monkeypatch.setenv(k, v)


def _route(cfg, pf, implicit, n):
    """(runs a non-default kernel, staging) of a row of degree n at the
    padded rank pf: staging is "w" (bf16 V, Woodbury), "g" (truncated
    bf16 Gramian) or None. Mirrors launch_als_solve."""
    env = CONFIGS[cfg]
    split = int(env.get(SPLIT, "0"))
    if n == 0:
        return False, None
    if split > 0 and pf < 128 and n > split:
        return True, None     # the workgroup kernel writes last
    if n <= 32:
        staged = BF16S in env and implicit
        return staged or (DUAL in env and n <= 24), "w" if staged else None
    if BF16G in env and pf == 64:
        return True, "g"
    return False, None


def _solve(monkeypatch, cfg, indptr, cols, vals, Y, implicit, ranges=None):
    """The trainer's call under cfg. Returns (X on the CPU, lv, YtY)."""
    from predictionio_amd.ops import als as als_ops
    _switch(monkeypatch, cfg)
    Yc = Y.cuda()
    YtY = als_ops.gramian(Yc) if implicit else None
    lv = als_ops.prepare_lv(Yc, YtY, LAM) if implicit else None
    n_rows = indptr.shape[0] - 1
    out = torch.full((n_rows, Y.shape[1]), float("nan"), device="cuda")
    csr = (indptr.cuda(), cols.cuda(), vals.cuda())
    kw = dict(YtY=YtY, lam=LAM, alpha=ALPHA, implicit=implicit, lv=lv)
    if ranges is None:
        als_ops.als_solve(*csr, Yc, out=out, **kw)
    else:
        for lo, hi in ranges:
            als_ops.als_solve(*csr, Yc, row_range=(lo, hi),
                              out=out[lo:hi], **kw)
    assert out.shape == (n_rows, Y.shape[1])
    return out.cpu(), lv, YtY


def _target(cfg, sizes, indptr, cols, vals, Y, X64, implicit, lv, YtY):
    """(comparison target, rows on a non-default kernel) for cfg."""
    from predictionio_amd.ops import als as als_ops
    f = Y.shape[1]
    routes = [_route(cfg, als_ops.pad_rank(f), implicit, n) for n in sizes]
    R = [r for r, (nd, _) in enumerate(routes) if nd]
    tgt = X64
    w_rows = [st == "w" for _, st in routes]
    if any(w_rows):
        Linv, V = lv
        assert V.dtype == torch.bfloat16
        W = woodbury_staged_oracle(indptr, cols, vals, V.cpu().double(),
                                   Linv.cpu().double(), ALPHA)
        tgt = expected(tgt, w_rows, W[:, :f])
    elif lv is not None:
        assert lv[1].dtype == torch.float32
    g_rows = [st == "g" for _, st in routes]
    if any(g_rows):
        G = mfma_gramian_staged_oracle(
            indptr, cols, vals, Y, YtY.cpu() if implicit else None, LAM,
            ALPHA, implicit, True)
        tgt = expected(tgt, g_rows, G)
    return tgt, R


_DEFAULT = {}


def _default_solution(monkeypatch, f, implicit):
    """The default kernels' result on every_degree_problem(f, implicit),
    solved once per process."""
    if (f, implicit) not in _DEFAULT:
        _, indptr, cols, vals, Y, _ = every_degree_problem(f, implicit)
        _DEFAULT[f, implicit] = _solve(monkeypatch, "default", indptr, cols,
                                       vals, Y, implicit)[0]
    return _DEFAULT[f, implicit]


def _bits_equal(A, B):
    return torch.equal(A.contiguous().view(torch.int32),
                       B.contiguous().view(torch.int32))


# ------------------------------------------------------ a. every degree

EVERY_DEGREE_CASES = [
    (cfg, f, implicit)
    for cfg in CONFIGS for f in (16, 32, 64, 128)
    for implicit in (True, False)
    if not (cfg.startswith("split") and f == 128)     # no such kernel:
    and not (cfg == "bf16g" and f != 64)              # see the ignored test
]


@requires_gpu
@pytest.mark.parametrize("cfg,f,implicit", EVERY_DEGREE_CASES)
def test_every_degree(monkeypatch, cfg, f, implicit):
    sizes, indptr, cols, vals, Y, X64 = every_degree_problem(f, implicit)
    X, lv, YtY = _solve(monkeypatch, cfg, indptr, cols, vals, Y, implicit)
    tgt, R = _target(cfg, sizes, indptr, cols, vals, Y, X64, implicit, lv,
                     YtY)
    bad = [sizes[r] for r in range(len(sizes))
           if not torch.isfinite(X[r]).all()]
    assert not bad, f"rows left unwritten or non-finite, degrees {bad}"
    maxabs = (X.double() - tgt).abs().max().item()
    print(f"{cfg} f={f} implicit={implicit} max abs diff {maxabs:.3e} "
          f"rel fro {_rel_fro(X, tgt):.3e}")
    assert torch.allclose(X.double(), tgt, atol=TOL, rtol=TOL), \
        f"max abs diff {maxabs}"
    if not R:
        return   # default kernels only (the control, an ignored switch)
    Xd = _default_solution(monkeypatch, f, implicit)
    floor = _rel_fro(Xd[R], X64[R])
    err = _rel_fro(X[R], tgt[R])
    print(f"OPTIN | {cfg} | {f} | {'implicit' if implicit else 'explicit'} "
          f"| {len(R)} | {floor:.3e} | {err:.3e} | {err / floor:.2f} |")
    worst = max(R, key=lambda r: _rel_fro(X[r], tgt[r]))
    assert err <= MARGIN * floor, \
        (f"rel fro {err:.3e} on the {len(R)} rows of the switched kernels, "
         f"default kernels {floor:.3e}; worst row {worst} of degree "
         f"{sizes[worst]}: {_rel_fro(X[worst], tgt[worst]):.3e}")


# ------------------------------------- b. ignored switches change nothing

IGNORED_CASES = (
    # (cfg, control, f, implicit, rows with n <= this)
    [("bf16s", "default", f, False, 100) for f in (16, 32, 64, 128)]
    + [("bf16g", "default", f, i, 100) for f in (16, 32, 128)
       for i in (True, False)]
    + [("split36", "default", 128, i, 100) for i in (True, False)]
    + [("bf16g", "default", 64, i, 32) for i in (True, False)]
    + [("split36", "default", f, i, 36) for f in (16, 32, 64)
       for i in (True, False)]
    + [("combo", "dual", f, False, 100) for f in (16, 32, 64, 128)]
)


@requires_gpu
@pytest.mark.parametrize("cfg,control,f,implicit,nmax", IGNORED_CASES)
def test_ignored_switch_changes_nothing(monkeypatch, cfg, control, f,
                                        implicit, nmax):
    """Where a switch has no kernel (explicit mode for the bf16 staging,
    ranks without the MFMA-Gramian or workgroup instantiation, rows below
    a kernel's range) the result is the control's, bit for bit."""
    sizes, indptr, cols, vals, Y, _ = every_degree_problem(f, implicit)
    X = _solve(monkeypatch, cfg, indptr, cols, vals, Y, implicit)[0]
    if control == "default":
        C = _default_solution(monkeypatch, f, implicit)
    else:
        C = _solve(monkeypatch, control, indptr, cols, vals, Y, implicit)[0]
    rows = [r for r, n in enumerate(sizes) if n <= nmax]
    assert len(rows) == len(sizes) or nmax < 100
    assert torch.isfinite(X).all() and torch.isfinite(C).all()
    ndiff = (X[rows].view(torch.int32) != C[rows].view(torch.int32)).sum()
    print(f"{cfg} vs {control} f={f} implicit={implicit}: {ndiff.item()} "
          f"differing words in {len(rows)} rows")
    assert _bits_equal(X[rows], C[rows])


# ------------------------------------ c. independence of the wave-mate

MATE_DEGREES = [0, 1] + list(range(19, 26)) + [32, 33, 40]


def _split_rows(indptr, cols, vals):
    ip = indptr.tolist()
    return [(cols[s:e], vals[s:e]) for s, e in zip(ip[:-1], ip[1:])]


def _join_rows(rows):
    sizes = [len(c) for c, _ in rows]
    indptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(),
                          dtype=torch.int64)
    return (indptr, torch.cat([c for c, _ in rows]).to(torch.int32),
            torch.cat([v for _, v in rows]).float())


def _replace_rows(rows, parity, seed):
    """Rows r with r % 2 == parity get another degree out of MATE_DEGREES
    and fresh columns and values; the others keep theirs."""
    g = torch.Generator().manual_seed(seed)
    out = list(rows)
    for r in range(parity, len(rows), 2):
        pool = [d for d in MATE_DEGREES if d != len(rows[r][0])]
        n = pool[torch.randint(0, len(pool), (1,), generator=g).item()]
        out[r] = (torch.randint(0, N_COLS, (n,), generator=g).int(),
                  torch.rand(n, generator=g) * 3 + 0.5)
    return out


@requires_gpu
@pytest.mark.parametrize("f", [64, 16])
@pytest.mark.parametrize("implicit", [True, False])
@pytest.mark.parametrize("cfg", ["dual", "combo"])
def test_row_independent_of_wave_mate(monkeypatch, cfg, implicit, f):
    """Rows 2k and 2k + 1 share a wave of the dual kernel, one per
    32-lane half. Changing one of them (degree, columns, values) must
    not change a bit of the other."""
    _, indptr, cols, vals, Y, _ = every_degree_problem(f, implicit)
    rows = _split_rows(indptr, cols, vals)
    base = _solve(monkeypatch, cfg, indptr, cols, vals, Y, implicit)[0]
    assert torch.isfinite(base).all()
    for parity in (1, 0):
        changed = _replace_rows(rows, parity, 31 + parity)
        assert all(len(changed[r][0]) != len(rows[r][0])
                   for r in range(parity, len(rows), 2))
        X = _solve(monkeypatch, cfg, *_join_rows(changed), Y, implicit)[0]
        assert torch.isfinite(X).all()
        keep = slice(1 - parity, None, 2)
        bad = [r for r in range(1 - parity, len(rows), 2)
               if not _bits_equal(X[r], base[r])]
        print(f"{cfg} f={f} implicit={implicit} parity {parity}: "
              f"{len(bad)} kept rows changed")
        assert _bits_equal(X[keep], base[keep]), \
            f"rows {bad} (degrees {[len(rows[r][0]) for r in bad]}) changed"


# ------------------------------- d. row ranges, tails and re-pairing

RANGES = [(0, 1), (1, 4), (4, 9), (9, 90)]


@requires_gpu
@pytest.mark.parametrize("cfg,implicit", [
    ("dual", True), ("bf16s", True), ("combo", True), ("dual", False)])
def test_row_ranges_are_bit_identical(monkeypatch, cfg, implicit):
    """90 rows whole, then in ranges of 1, 3, 5 and 81 rows (every
    n_rows % 4 but 0; the odd offsets pair each row with another partner
    and put it in the other half of the wave): the same bits."""
    sizes, indptr, cols, vals, Y, _ = every_degree_problem(64, implicit)
    assert len(sizes) == RANGES[-1][1]
    assert sorted({(hi - lo) % 4 for lo, hi in RANGES}) == [1, 3]
    assert {hi - lo for lo, hi in RANGES} == {1, 3, 5, 81}
    whole = _solve(monkeypatch, cfg, indptr, cols, vals, Y, implicit)[0]
    parts = _solve(monkeypatch, cfg, indptr, cols, vals, Y, implicit,
                   ranges=RANGES)[0]
    assert torch.isfinite(whole).all() and torch.isfinite(parts).all()
    bad = [r for r in range(len(sizes))
           if not _bits_equal(whole[r], parts[r])]
    print(f"{cfg} implicit={implicit}: {len(bad)} differing rows")
    assert not bad, f"rows {bad}, degrees {[sizes[r] for r in bad]}"


# ------------------------------------------------ e. degenerate pivots

@functools.lru_cache(maxsize=None)
def _degenerate(implicit):
    sizes, indptr, cols, vals, Y = degenerate_problem(implicit)
    return (sizes, indptr, cols, vals, Y,
            _ref64(indptr, cols, vals, Y, LAM, implicit))


@requires_gpu
@pytest.mark.parametrize("implicit", [True, False])
@pytest.mark.parametrize("cfg", ["dual", "bf16s", "combo"])
def test_degenerate_pivots(monkeypatch, cfg, implicit):
    """The problem of test_als_solve_chain_gpu.test_degenerate_pivots
    (all-zero implicit values where d clamps, one column repeated 2, 20,
    32, 40 times, empty rows) through the switched Woodbury kernels."""
    sizes, indptr, cols, vals, Y, X64 = _degenerate(implicit)
    X, lv, YtY = _solve(monkeypatch, cfg, indptr, cols, vals, Y, implicit)
    tgt, _ = _target(cfg, sizes, indptr, cols, vals, Y, X64, implicit, lv,
                     YtY)
    maxabs = (X.double() - tgt).abs().max().item()
    print(f"{cfg} implicit={implicit} max abs diff {maxabs:.3e}")
    assert torch.isfinite(X).all()
    assert torch.allclose(X.double(), tgt, atol=TOL, rtol=TOL), \
        f"max abs diff {maxabs}"
    for r, n in enumerate(sizes):
        if n == 0:
            assert X[r].abs().max().item() == 0.0


# --------------------------------- f. the dual kernel's second trip

SECOND_TRIP = 1 << 22   # the dual launcher caps its grid at 2^20 workgroups
TAIL = 4096             # of four rows: row r + 2^22 reuses row r's half-wave
# period 13 (2^22 = 10 mod 13); mean degree 7.6
PATTERN = [24, 2, 3, 1, 0, 28, 20, 4, 5, 3, 1, 6, 2]


@requires_gpu
def test_dual_second_trip_through_row_loop(monkeypatch):
    """A half-wave's second row must not see its first row's LDS (Yl, M,
    tv, dv): the last 4096 of 2^22 + 4096 rows solved as part of the
    whole equal the same rows solved alone. combo, implicit, f = 16
    (about 270 MB per [rows, 16] buffer)."""
    from predictionio_amd.ops import als as als_ops
    P, f = len(PATTERN), 16
    trips = [(PATTERN[i], PATTERN[(i + SECOND_TRIP) % P]) for i in range(P)]
    assert all(a != b for a, b in trips)
    assert any(a in (20, 24) and b == 1 for a, b in trips)
    assert any(b == 0 for a, b in trips)
    assert any(25 <= b <= 32 for a, b in trips)
    _switch(monkeypatch, "combo")
    n_rows = SECOND_TRIP + TAIL
    g = torch.Generator(device="cuda").manual_seed(4343)
    deg = torch.tensor(PATTERN, device="cuda")[
        torch.arange(n_rows, device="cuda") % P]
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(deg, 0, out=indptr[1:])
    nnz = int(indptr[-1])
    cols = torch.randint(0, N_COLS, (nnz,), generator=g, device="cuda",
                         dtype=torch.int32)
    vals = torch.rand(nnz, generator=g, device="cuda") * 3 + 0.5
    Y = torch.randn((N_COLS, f), generator=g, device="cuda") / 4.0
    YtY = als_ops.gramian(Y)
    lv = als_ops.prepare_lv(Y, YtY, LAM)
    assert lv[1].dtype == torch.bfloat16
    kw = dict(YtY=YtY, lam=LAM, alpha=ALPHA, implicit=True, lv=lv)
    whole = als_ops.als_solve(indptr, cols, vals, Y, **kw)[SECOND_TRIP:]
    alone = als_ops.als_solve(indptr, cols, vals, Y,
                              row_range=(SECOND_TRIP, n_rows), **kw)
    assert whole.shape == alone.shape == (TAIL, f)
    assert torch.isfinite(whole).all() and torch.isfinite(alone).all()
    ndiff = (whole.contiguous().view(torch.int32)
             != alone.view(torch.int32)).sum().item()
    print(f"{ndiff} differing words")
    assert ndiff == 0


# ------------------------------------------------- g. ranks that pad

@requires_gpu
@pytest.mark.parametrize("implicit", [True, False])
@pytest.mark.parametrize("f", [10, 20, 48, 100])
@pytest.mark.parametrize("cfg", ["default", "combo"])
def test_padded_rank_trainer_call(monkeypatch, cfg, f, implicit):
    """A rank that pad_rank pads (10 -> 16, 20 -> 32, 48 -> 64,
    100 -> 128), solved the trainer's way: lv from prepare_lv, two
    row_range chunks, out = rows of an unpadded [n_rows, f] buffer, so
    als_solve takes its copy-out branch."""
    sizes, indptr, cols, vals, Y, X64 = every_degree_problem(f, implicit)
    n_rows = len(sizes)
    X, lv, YtY = _solve(monkeypatch, cfg, indptr, cols, vals, Y, implicit,
                        ranges=[(0, n_rows // 2), (n_rows // 2, n_rows)])
    assert X.shape == (n_rows, f) == X64.shape
    if implicit:
        from predictionio_amd.ops import als as als_ops
        assert lv[1].shape == (N_COLS, als_ops.pad_rank(f))
    tgt, _ = _target(cfg, sizes, indptr, cols, vals, Y, X64, implicit, lv,
                     YtY)
    bad = [sizes[r] for r in range(n_rows) if not torch.isfinite(X[r]).all()]
    assert not bad, f"rows left unwritten or non-finite, degrees {bad}"
    maxabs = (X.double() - tgt).abs().max().item()
    print(f"{cfg} f={f} implicit={implicit} max abs diff {maxabs:.3e} "
          f"rel fro {_rel_fro(X, tgt):.3e}")
    assert torch.allclose(X.double(), tgt, atol=TOL, rtol=TOL), \
        f"max abs diff {maxabs}"
