"""ALS half-iteration solve: HIP kernel on GPU, torch reference on CPU.

Replaces MLlib's normal-equation construction + CholeskySolver (reference:
ALS.train/trainImplicit call sites, SURVEY.md §2.7/2.9 K1+K2). The CPU path
is the numerics reference the GPU kernel is validated against.
"""

from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch

SUPPORTED_RANKS = (16, 32, 64, 128)


def pad_rank(f: int) -> int:
    for s in SUPPORTED_RANKS:
        if f <= s:
            return s
    raise ValueError(f"rank {f} > 128 not supported")


ALS_WIDE_RANKS = (192, 256)  # the packed-triangle solver (csrc/als_wide.hip)


def als_pad_rank(f: int) -> int:
    """The rank als_solve pads f to on a GPU: pad_rank up to 128, then 192
    and 256. Only the ALS solve goes past 128; everything else that pads
    (top-K fp32 mode, held-out ranking, the Woodbury precompute) keeps
    pad_rank."""
    for s in SUPPORTED_RANKS + ALS_WIDE_RANKS:
        if f <= s:
            return s
    raise ValueError(f"rank {f} > 256 not supported by the ALS solvers")


ROW_LIMIT = 2 ** 31  # the kernels carry row counts and row ids as int


def check_row_count(**counts: int) -> None:
    """ValueError when a row count reaches 2^31. Callers run it on the
    shapes alone, before any copy, padding or launch."""
    for name, n in counts.items():
        if n >= ROW_LIMIT:
            raise ValueError(
                f"{name} = {n} rows: row counts must be below 2^31")


def gramian(Y: torch.Tensor) -> torch.Tensor:
    """YtY (f x f) — a plain library GEMM (hipBLASLt on device)."""
    return Y.t() @ Y


def row_transform(A: torch.Tensor, W: torch.Tensor,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A[N, f] @ W[f, f] on the GPU's hand-written row-transform kernel
    (fp32 in, fp32 accumulate). `out`, if given, is written in place."""
    check_row_count(A=A.shape[0])
    from predictionio_amd.ops import hip_ext
    return hip_ext().als_row_transform(A.contiguous(), W.contiguous(), out)


def woodbury_lv(Y: torch.Tensor, YtY: torch.Tensor,
                lam: float) -> tuple:
    """(Linv, V): L = chol(YtY + lam I), Linv = L^-1, V = Y L^-T — per-half-iteration
    precompute that enables the per-row Woodbury fast path
    (als_woodbury_kernel). One fxf Cholesky + one triangular-solve GEMM
    over all items (rocBLAS trsm); the whitened rows satisfy
    v_i . v_j = y_i^T B^-1 y_j."""
    f = Y.shape[1]
    eye = torch.eye(f, dtype=Y.dtype, device=Y.device)
    B = YtY + lam * eye
    L = torch.linalg.cholesky(B)
    # Materialize L^-1 (f x f, cheap) and whiten with a GEMM: hipBLAS trsm
    # with a 10M-row rhs hit HIPBLAS_STATUS_ALLOC_FAILED at bench scale,
    # while hipBLASLt GEMMs of that shape are proven.
    Linv = torch.linalg.solve_triangular(L, eye, upper=False)
    # row v_i = L^-1 y_i. On GPU the streaming fp32-MFMA row-transform
    # kernel (als_xform.hip) with W = Linv^T; the library GEMM ran this
    # tall-skinny shape several times off the HBM roofline.
    if Y.is_cuda:
        V = row_transform(Y, Linv.mT.contiguous())
    else:
        V = (Y @ Linv.mT).contiguous()
    import os as _os
    if (_os.environ.get("PIO_ALS_STAGE_BF16") == "1" and Y.is_cuda):
        V = V.to(torch.bfloat16).contiguous()
    return Linv, V


# ------------------------------------------------------------ heavy rows
#
# Rows of degree > heavy_min() leave the one-unit-per-row solvers for the
# split-row route (csrc/als_heavy.hip): chunks of heavy_chunk() consecutive
# CSR entries, one workgroup each. Both defaults are measured
# (scripts/als_heavy_probe.py, table in NOTES.md).

HEAVY_MIN_DEFAULT = 4096
HEAVY_CHUNK_DEFAULT = 8192
_HEAVY_FLOOR = 64      # the Woodbury kernels own rows up to degree 48
_INT_MAX = 2 ** 31 - 1

_heavy_stats: Dict[str, int] = {"calls": 0, "rows": 0, "chunks": 0}


def heavy_stats() -> Dict[str, int]:
    """Cumulative counters of the split-row route since import: solves that
    took it, heavy rows solved and chunks launched."""
    return dict(_heavy_stats)


_nnls_stats: Dict[str, int] = {"calls": 0, "rows": 0}


def nnls_stats() -> Dict[str, int]:
    """Cumulative counters of the nonnegative solver since import: GPU
    solves that took it (als_solve(nonnegative=True)) and rows solved."""
    return dict(_nnls_stats)


def heavy_min() -> int:
    """Rows of degree > this are heavy (PIO_ALS_HEAVY_MIN, read on every
    call). 0 disables the route; other values below 64 count as 64, so a
    heavy row is never a Woodbury row."""
    v = int(os.environ.get("PIO_ALS_HEAVY_MIN", HEAVY_MIN_DEFAULT))
    if v <= 0:
        return 0
    return min(max(v, _HEAVY_FLOOR), _INT_MAX)


def heavy_chunk() -> int:
    """CSR entries per chunk of a heavy row (PIO_ALS_HEAVY_CHUNK, read on
    every call): a positive multiple of 32."""
    v = int(os.environ.get("PIO_ALS_HEAVY_CHUNK", HEAVY_CHUNK_DEFAULT))
    if v <= 0 or v % 32 or v > 1 << 24:
        raise ValueError(
            f"PIO_ALS_HEAVY_CHUNK = {v}: need a multiple of 32 in (0, 2^24]")
    return v


def _heavy_ws_bytes() -> int:
    """Cap on the partial workspace: PIO_ALS_HEAVY_WS_MB MiB, default 256."""
    return int(float(os.environ.get("PIO_ALS_HEAVY_WS_MB", "256")) * 2 ** 20)


class HeavyPlan:
    """The heavy rows of one CSR and their chunk table, on the host:
    rows [H] (ascending row ids), chunk_ptr [H + 1] and chunks [C, 2]
    (entry start, end; absolute offsets into indices / values), all int64.
    The chunk length is fixed, so a row's chunks depend on its own degree
    only. Device copies are made once per (row range, device)."""

    def __init__(self, rows, chunk_ptr, chunks, n_rows, hmin, chunk):
        self.rows, self.chunk_ptr, self.chunks = rows, chunk_ptr, chunks
        self.n_rows, self.heavy_min, self.chunk = n_rows, hmin, chunk
        self._dev: dict = {}
        self._narrowed: dict = {}

    @classmethod
    def build(cls, indptr: torch.Tensor, hmin: Optional[int] = None,
              chunk: Optional[int] = None) -> "HeavyPlan":
        """From a row-pointer array on any device: one reduction and one
        small transfer."""
        hmin = heavy_min() if hmin is None else hmin
        chunk = heavy_chunk() if chunk is None else chunk
        n_rows = indptr.shape[0] - 1
        empty = torch.zeros(0, dtype=torch.int64)
        if hmin <= 0 or n_rows <= 0:
            return cls(empty, torch.zeros(1, dtype=torch.int64),
                       empty.view(0, 2), n_rows, hmin, chunk)
        deg = indptr[1:] - indptr[:-1]
        rows = torch.nonzero(deg > hmin).flatten()
        se = torch.stack([rows, indptr[rows], indptr[rows + 1]]).cpu()
        rows, start, end = se[0], se[1], se[2]
        n_c = (end - start + chunk - 1) // chunk
        chunk_ptr = torch.zeros(rows.numel() + 1, dtype=torch.int64)
        torch.cumsum(n_c, 0, out=chunk_ptr[1:])
        owner = torch.repeat_interleave(torch.arange(rows.numel()), n_c)
        k = torch.arange(int(chunk_ptr[-1])) - chunk_ptr[owner]
        c_lo = start[owner] + k * chunk
        c_hi = torch.minimum(c_lo + chunk, end[owner])
        return cls(rows.contiguous(), chunk_ptr,
                   torch.stack([c_lo, c_hi], 1).contiguous(), n_rows, hmin,
                   chunk)

    def narrow(self, lo: int, hi: int) -> "HeavyPlan":
        """The plan of rows [lo, hi), row ids rebased to lo (host only)."""
        if (lo, hi) == (0, self.n_rows):
            return self
        got = self._narrowed.get((lo, hi))
        if got is None:
            a, b = torch.searchsorted(
                self.rows, torch.tensor([lo, hi])).tolist()
            cp = self.chunk_ptr[a:b + 1]
            got = HeavyPlan((self.rows[a:b] - lo).contiguous(), cp - cp[0],
                            self.chunks[int(cp[0]):int(cp[-1])].contiguous(),
                            hi - lo, self.heavy_min, self.chunk)
            self._narrowed[(lo, hi)] = got
        return got

    def on(self, device) -> tuple:
        """(rows, chunk_ptr, chunks) on `device`."""
        got = self._dev.get(device)
        if got is None:
            got = tuple(t.to(device) for t in
                        (self.rows, self.chunk_ptr, self.chunks))
            self._dev[device] = got
        return got


def heavy_plan(indptr: torch.Tensor) -> HeavyPlan:
    """The HeavyPlan of a whole CSR under the knobs in force: build it once
    per CSR and hand it to every als_solve over that CSR."""
    return HeavyPlan.build(indptr)


def _heavy_pass(ext, hp: HeavyPlan, ix, vv, Yp, YtYp, X, lam, alpha,
                implicit, wr_scale, nonnegative=False, iters=None) -> None:
    """Solve hp's rows into X (rows of hp index X) on the split-row route;
    nonnegative: its partials go to the block-pivoting solver."""
    # the kernels trust the tables: check them where that costs nothing
    if (int(hp.rows[-1]) >= X.shape[0] or int(hp.rows[0]) < 0
            or int(hp.chunks.min()) < 0
            or int(hp.chunks.max()) > ix.numel()
            or bool((hp.chunks[:, 1] <= hp.chunks[:, 0]).any())):
        raise ValueError("heavy-row plan does not fit this CSR")
    rows, chunk_ptr, chunks = hp.on(X.device)
    if nonnegative:
        ext.als_heavy_solve(ix, vv, Yp, YtYp, X, rows, chunk_ptr, chunks,
                            hp.chunk_ptr, float(lam), float(alpha),
                            bool(implicit), bool(wr_scale),
                            _heavy_ws_bytes(), True, iters)
    else:
        ext.als_heavy_solve(ix, vv, Yp, YtYp, X, rows, chunk_ptr, chunks,
                            hp.chunk_ptr, float(lam), float(alpha),
                            bool(implicit), bool(wr_scale),
                            _heavy_ws_bytes())
    _heavy_stats["calls"] += 1
    _heavy_stats["rows"] += hp.rows.numel()
    _heavy_stats["chunks"] += hp.chunks.shape[0]


def als_solve(indptr: torch.Tensor, indices: torch.Tensor,
              values: torch.Tensor, Y: torch.Tensor,
              YtY: Optional[torch.Tensor] = None,
              lam: float = 0.01, alpha: float = 1.0,
              implicit: bool = False, wr_scale: bool = True,
              lv: Optional[tuple] = None,
              row_range: Optional[Tuple[int, int]] = None,
              out: Optional[torch.Tensor] = None,
              plan: Optional[HeavyPlan] = None,
              nonnegative: bool = False,
              nnls_iters: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Solve all rows of one ALS half-iteration.

    explicit: (sum y y^T + lam*nnz*I) x = sum r*y      (ALS-WR, like MLlib)
    implicit: (YtY + sum alpha*r y y^T + lam*I) x = sum (1+alpha*r) y
              (Hu-Koren; YtY required)

    On GPU, rows with nnz <= 32 take the Woodbury path (exact — the same
    linear system through the push-through identity). Implicit mode runs
    three phases: the Woodbury kernel emits whitened Z rows, one
    row-transform launch maps Z -> X = Z L^-1 for all rows, then the dense kernel fills
    the big (nnz > 32) rows directly. Rows of degree > heavy_min() are
    skipped by all of these and solved last by the split-row route
    (HeavyPlan, csrc/als_heavy.hip), which writes X directly.

    lv: optional precomputed (Linv, V) from prepare_lv() — hoist it when
    solving in row chunks (the multi-GPU gather/solve overlap path).
    row_range: solve only rows [lo, hi) of the CSR (indices/values stay
    whole; indptr offsets are absolute). out: optional [rows, f] target
    written in place (enables chunked solves into one padded buffer).
    plan: optional heavy_plan(indptr) of the whole CSR; without it (or if
    the knobs changed since it was made) the call builds its own.

    nonnegative: per row, minimise 1/2 x^T A x - b^T x over x >= 0 with
    the A and b above (MLlib's setNonnegative), exactly, by block principal
    pivoting. On GPU every row that is not heavy takes the fused kernels of
    csrc/als_nnls.hip and the heavy rows take the split-row route with the
    same solver behind its Gramians; there is no Woodbury form, so lv is
    ignored. On CPU: als_solve_nnls_ref. nnls_iters: optional int32 [rows]
    GPU tensor that receives the solver's trip count per row (a probe's
    output; needs nonnegative).

    Ranks 129..256 on GPU are padded to 192 or 256 (als_pad_rank) and
    take one pass of the packed-triangle MFMA solver (csrc/als_wide.hip)
    over all rows, explicit or implicit: no Woodbury pass (lv is ignored)
    and no heavy-row split (plan is ignored). nonnegative raises
    ValueError there, and so does any rank above 256, before any copy or
    launch. PIO_ALS_WIDE_GRID=N (read on every call) runs that solver on N
    workgroups instead of one per CU; a row's bits do not depend on it.
    """
    if nnls_iters is not None and not (nonnegative and Y.is_cuda):
        raise ValueError("nnls_iters is an output of the GPU nonnegative "
                         "solver")
    if Y.is_cuda:
        if als_pad_rank(Y.shape[1]) > 128 and nonnegative:
            raise ValueError(
                f"nonnegative solves stop at rank 128, got {Y.shape[1]}")
    check_row_count(indptr=indptr.shape[0] - 1, Y=Y.shape[0])
    n_all = indptr.shape[0] - 1
    if implicit:
        wr_scale = False  # Hu-Koren regularizes with plain lambda*I
        if YtY is None:
            YtY = gramian(Y)
    if row_range is not None:
        lo, hi = row_range
        indptr = indptr[lo:hi + 1]
    if Y.is_cuda:
        from predictionio_amd.ops import hip_ext
        ext = hip_ext()
        f = Y.shape[1]
        pf = als_pad_rank(f)
        Yp = (Y if pf == f
              else torch.nn.functional.pad(Y, (0, pf - f))).contiguous()
        YtYp = None
        if YtY is not None:
            YtYp = (YtY if pf == f
                    else torch.nn.functional.pad(YtY, (0, pf - f, 0, pf - f))
                    ).contiguous()
        ip, ix, vv = (indptr.contiguous(), indices.contiguous(),
                      values.contiguous())
        # out-of-range column ids would make the kernels gather OOB from
        # Y (undefined behavior that can wedge the device) — fail loudly
        # here instead; one .max() reduction is noise vs the solve
        if ix.numel():
            mx = int(ix.max())
            if mx >= Y.shape[0] or int(ix.min()) < 0:
                raise ValueError(
                    f"CSR column id out of range: [{int(ix.min())}, {mx}]"
                    f" vs {Y.shape[0]} factor rows")
        direct_out = (out if out is not None and pf == f
                      and out.is_contiguous() else None)
        if pf > 128:
            # one pass over every row: no Woodbury, no heavy-row split
            if ip.numel() and (int(ip[0]) < 0 or int(ip[-1]) > ix.numel()):
                raise ValueError(
                    f"CSR row pointers [{int(ip[0])}, {int(ip[-1])}] outside"
                    f" the {ix.numel()} stored ratings")
            X = ext.als_solve_wide(
                ip, ix, vv, Yp, YtYp, float(lam), float(alpha),
                bool(implicit), bool(wr_scale), direct_out,
                int(os.environ.get("PIO_ALS_WIDE_GRID", "0")))
            res = X[:, :f].contiguous() if pf != f else X
            if out is not None and res.data_ptr() != out.data_ptr():
                out.copy_(res)
                return out
            return res
        # heavy rows: the dense kernels skip them, the split-row pass at
        # the end solves them
        hp = None
        hmin = heavy_min()
        if hmin > 0 and ix.numel() > hmin:
            chunk = heavy_chunk()
            if (plan is not None and plan.n_rows == n_all
                    and (plan.heavy_min, plan.chunk) == (hmin, chunk)):
                hp = plan.narrow(*row_range) if row_range else plan
            else:
                hp = HeavyPlan.build(ip, hmin, chunk)
            if hp.rows.numel() == 0:
                hp = None
        above = hmin if hp is not None else _INT_MAX
        if nonnegative:
            X = ext.als_nnls_solve(ip, ix, vv, Yp, YtYp, float(lam),
                                   float(alpha), bool(implicit),
                                   bool(wr_scale), direct_out, above,
                                   nnls_iters)
            _nnls_stats["calls"] += 1
            _nnls_stats["rows"] += ip.shape[0] - 1
        elif implicit and pf <= 128:
            if lv is not None:
                Linv, V = lv
            else:
                Linv, V = woodbury_lv(Yp, YtYp, lam)
            # opt-in bf16 staging of the whitened factors (see the
            # BF16S kernel variant; numerics bounded by
            # profiles/bf16_numerics_study.txt)
            import os as _os
            if _os.environ.get("PIO_ALS_STAGE_BF16") == "1" \
                    and V.dtype == torch.float32:
                V = V.to(torch.bfloat16).contiguous()
            Z = ext.als_solve(ip, ix, vv, Yp, YtYp, V, float(lam),
                              float(alpha), True, False, 1, None, None,
                              above)
            # X = Z L^-1 for all rows (Woodbury rows hold z; big rows get
            # overwritten by the dense pass next)
            X = row_transform(Z, Linv, out=direct_out)
            ext.als_solve(ip, ix, vv, Yp, YtYp, None, float(lam),
                          float(alpha), True, False, 2, X, None, above)
        else:
            X = ext.als_solve(ip, ix, vv, Yp, YtYp, None, float(lam),
                              float(alpha), bool(implicit), bool(wr_scale),
                              0, direct_out, None, above)
        if hp is not None:
            if nonnegative:
                _heavy_pass(ext, hp, ix, vv, Yp, YtYp, X, lam, alpha,
                            implicit, wr_scale, True, nnls_iters)
            else:
                _heavy_pass(ext, hp, ix, vv, Yp, YtYp, X, lam, alpha,
                            implicit, wr_scale)
        res = X[:, :f].contiguous() if pf != f else X
        if out is not None and res.data_ptr() != out.data_ptr():
            out.copy_(res)
            return out
        return res
    if nonnegative:
        res = als_solve_nnls_ref(indptr, indices, values, Y, YtY, lam,
                                 alpha, implicit, wr_scale)
    else:
        res = als_solve_ref(indptr, indices, values, Y, YtY, lam, alpha,
                            implicit, wr_scale)
    if out is not None:
        out.copy_(res)
        return out
    return res


def prepare_lv(Y: torch.Tensor, YtY: torch.Tensor, lam: float):
    """Precompute the (Linv, V) Woodbury pair once per half-iteration so
    chunked solves (gather/solve overlap) don't redo the whitening GEMM
    per chunk. Pads to the supported rank like als_solve."""
    f = Y.shape[1]
    pf = pad_rank(f)
    Yp = (Y if pf == f
          else torch.nn.functional.pad(Y, (0, pf - f))).contiguous()
    YtYp = (YtY if pf == f
            else torch.nn.functional.pad(YtY, (0, pf - f, 0, pf - f))
            ).contiguous()
    return woodbury_lv(Yp, YtYp, lam)


def als_solve_ref(indptr, indices, values, Y, YtY=None, lam=0.01, alpha=1.0,
                  implicit=False, wr_scale=True) -> torch.Tensor:
    """Pure-torch fp32 reference (used on CPU and in GPU numerics tests)."""
    n_rows = indptr.shape[0] - 1
    f = Y.shape[1]
    X = torch.zeros((n_rows, f), dtype=Y.dtype, device=Y.device)
    eye = torch.eye(f, dtype=Y.dtype, device=Y.device)
    ip = indptr.tolist()
    for r in range(n_rows):
        s, e = ip[r], ip[r + 1]
        nnz = e - s
        if implicit:
            A = (YtY if YtY is not None else gramian(Y)).clone()
            b = torch.zeros(f, dtype=Y.dtype, device=Y.device)
            if nnz:
                cols = indices[s:e].long()
                Yr = Y[cols]
                v = values[s:e]
                A = A + (Yr.t() * (alpha * v)) @ Yr
                b = Yr.t() @ (1.0 + alpha * v)
            A = A + lam * eye
        else:
            if nnz == 0:
                continue
            cols = indices[s:e].long()
            Yr = Y[cols]
            v = values[s:e]
            A = Yr.t() @ Yr + lam * (nnz if wr_scale else 1.0) * eye
            b = Yr.t() @ v
        X[r] = torch.linalg.solve(A, b)
    return X


def normal_equations(indptr, indices, values, Y, YtY, lam, alpha, implicit,
                     wr_scale, r):
    """(A, b) of row r as in als_solve's docstring, in Y's dtype. An
    explicit row without ratings gives A = 0, b = 0."""
    f = Y.shape[1]
    s, e = int(indptr[r]), int(indptr[r + 1])
    Yr = Y[indices[s:e].long()]
    v = values[s:e].to(Y.dtype)
    eye = torch.eye(f, dtype=Y.dtype, device=Y.device)
    if implicit:
        A = ((YtY if YtY is not None else gramian(Y))
             + (Yr.t() * (alpha * v)) @ Yr + lam * eye)
        return A, Yr.t() @ (1.0 + alpha * v)
    return (Yr.t() @ Yr + lam * ((e - s) if wr_scale else 1.0) * eye,
            Yr.t() @ v)


NNLS_REF_MAX_IT = 64  # the kernels' NNLS_MAX_IT


def nnls_block_pivot(A: torch.Tensor, b: torch.Tensor,
                     max_it: int = NNLS_REF_MAX_IT):
    """argmin 1/2 x^T A x - b^T x over x >= 0 for symmetric positive
    definite A by block principal pivoting with the backup exchange rule
    (Kim and Park), in A's dtype: the algorithm of csrc/als_nnls.hip step
    for step. Returns (x, trips)."""
    f = A.shape[0]
    eye = torch.eye(f, dtype=A.dtype, device=A.device)
    P = torch.zeros(f, dtype=torch.bool, device=A.device)
    x, y = torch.zeros_like(b), -b
    p, ninf, it = 3, f + 1, 0
    while it < max_it:
        bad = torch.where(P, x < 0, y < 0)
        nb = int(bad.sum())
        if nb == 0:
            break
        if nb < ninf:
            ninf, p = nb, 3
        elif p > 0:
            p -= 1
        else:   # backup rule: the infeasible coordinate of largest index
            k = int(torch.nonzero(bad).max())
            bad = torch.zeros_like(bad)
            bad[k] = True
        P = P ^ bad
        M = torch.where(P[:, None] & P[None, :], A, eye)
        rhs = torch.where(P, b, torch.zeros_like(b))
        x = torch.cholesky_solve(rhs[:, None],
                                 torch.linalg.cholesky(M))[:, 0] * P
        y = (A @ x - b) * ~P
        it += 1
    return x.clamp_min(0), it


def als_solve_nnls_ref(indptr, indices, values, Y, YtY=None, lam=0.01,
                       alpha=1.0, implicit=False,
                       wr_scale=True) -> torch.Tensor:
    """Pure-torch reference of als_solve(nonnegative=True): the normal
    equations of als_solve_ref, then nnls_block_pivot, in Y's dtype (the
    CPU path; the GPU tests run it in float64). Rows without ratings give
    zeros in both modes (b = 0)."""
    n_rows = indptr.shape[0] - 1
    X = torch.zeros((n_rows, Y.shape[1]), dtype=Y.dtype, device=Y.device)
    if implicit:
        wr_scale = False
        if YtY is None:
            YtY = gramian(Y)
    for r in range(n_rows):
        if indptr[r + 1] > indptr[r]:
            A, b = normal_equations(indptr, indices, values, Y, YtY, lam,
                                    alpha, implicit, wr_scale, r)
            X[r] = nnls_block_pivot(A, b)[0]
    return X


# ------------------------------------------------------------- objective
#
# What the solvers above minimise, with s_ui = x_u . y_i, sums marked
# "obs" over the stored ratings, n_u / m_i the row degrees of the user
# and item CSR:
#
#   explicit (ALS-WR):  L = sum_obs (r - s)^2
#                           + lam (sum_u n_u |x_u|^2 + sum_i m_i |y_i|^2)
#   implicit (Hu-Koren, p = 1 and c = 1 + alpha r on stored pairs):
#                       L = sum_obs [(1 + alpha r)(1 - s)^2 - s^2]
#                           + <XtX, YtY>_F + lam (|X|_F^2 + |Y|_F^2)
#
# <XtX, YtY>_F is the sum of s^2 over ALL user-item pairs; setting the
# gradient in x_u to zero gives the systems in als_solve's docstring.
# The only part that touches every rating is the pair of sums
#   A = sum_obs w (t - s)^2,  B = sum_obs s^2
# with (w, t) = (1, r) explicit, (1 + alpha r, 1) implicit.

_LOSS_CHUNK = 1 << 20  # ratings per chunk of the torch reference


def als_residual_sums_ref(indptr, indices, values, X, Y, alpha=1.0,
                          implicit=False, pred=None) -> torch.Tensor:
    """[A, B] as a float64 [2] tensor in chunked torch: s in the factors'
    dtype, everything after it in fp64. The CPU path, and what the GPU
    kernel is validated against."""
    nnz = indices.shape[0]
    out = torch.zeros(2, dtype=torch.float64, device=X.device)
    for a in range(0, nnz, _LOSS_CHUNK):
        b = min(nnz, a + _LOSS_CHUNK)
        pos = torch.arange(a, b, device=indptr.device)
        rows = torch.searchsorted(indptr, pos, right=True) - 1
        s = (X[rows] * Y[indices[a:b].long()]).sum(1)
        if pred is not None:
            pred[a:b] = s
        s = s.double()
        r = values[a:b].double()
        if implicit:
            out[0] += ((1.0 + float(alpha) * r) * (1.0 - s) ** 2).sum()
        else:
            out[0] += ((r - s) ** 2).sum()
        out[1] += (s * s).sum()
    return out


def als_residual_sums(indptr: torch.Tensor, indices: torch.Tensor,
                      values: torch.Tensor, X: torch.Tensor,
                      Y: torch.Tensor, alpha: float = 1.0,
                      implicit: bool = False,
                      pred: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[A, B] = [sum w (t - s)^2, sum s^2] over the stored ratings of a
    CSR whose rows are X's and whose columns are Y's, as a float64 [2]
    tensor on the inputs' device.

    On GPU one streaming HIP kernel (als_loss.hip) gathers the item rows
    where they lie: any rank 1 <= f <= 128, unpadded fp32 factors, fp32
    fma-chain dots, fp64 from there on, bit-reproducible. pred, if given
    ([nnz] fp32), receives s per rating. On CPU: als_residual_sums_ref."""
    check_row_count(indptr=indptr.shape[0] - 1, X=X.shape[0], Y=Y.shape[0])
    if not X.is_cuda:
        return als_residual_sums_ref(indptr, indices, values, X, Y, alpha,
                                     implicit, pred)
    from predictionio_amd.ops import hip_ext
    ext = hip_ext()
    ip, ix, vv = indptr.contiguous(), indices.contiguous(), values.contiguous()
    # same guard as als_solve: an out-of-range id (or a row pointer past
    # the ratings) is an out-of-bounds gather
    if ix.numel():
        mn, mx = int(ix.min()), int(ix.max())
        if mx >= Y.shape[0] or mn < 0:
            raise ValueError(
                f"CSR column id out of range: [{mn}, {mx}]"
                f" vs {Y.shape[0]} factor rows")
    if ip.numel() and (int(ip[0]) < 0 or int(ip[-1]) > ix.numel()):
        raise ValueError(
            f"CSR row pointers [{int(ip[0])}, {int(ip[-1])}] outside the"
            f" {ix.numel()} stored ratings")
    # X and Y go as they are: a non-contiguous factor matrix raises in
    # the binding; it is never copied (they are multi-GB)
    return ext.als_residual_sums(ip, ix, vv, X, Y, float(alpha),
                                 bool(implicit), pred)


def sq_row_norms(F: torch.Tensor) -> torch.Tensor:
    """|row|^2 of every row of F, computed and returned in fp64 (row
    chunks, so a multi-GB factor matrix is never copied whole)."""
    out = torch.empty(F.shape[0], dtype=torch.float64, device=F.device)
    for a in range(0, F.shape[0], _LOSS_CHUNK):
        out[a:a + _LOSS_CHUNK] = F[a:a + _LOSS_CHUNK].double().square().sum(1)
    return out


def regulariser_sum(F: torch.Tensor,
                    degrees: Optional[torch.Tensor]) -> torch.Tensor:
    """sum_rows deg |row|^2 (ALS-WR) or, with degrees None, |F|_F^2, as
    an fp64 scalar tensor."""
    n2 = sq_row_norms(F)
    return n2.sum() if degrees is None else (n2 * degrees.double()).sum()


def combine_objective(A: float, B: float, reg: float, frob: float,
                      nnz: int, lam: float, implicit: bool) -> dict:
    """Assemble the objective from its (globally summed) parts. sq_err is
    A: the squared error over the stored ratings, confidence-weighted in
    implicit mode. rmse (explicit only) is sqrt(A / nnz)."""
    if implicit:
        return {"loss": A - B + frob + lam * reg, "sq_err": A, "nnz": nnz}
    return {"loss": A + lam * reg, "sq_err": A, "nnz": nnz,
            "rmse": (A / nnz) ** 0.5 if nnz else 0.0}


def als_objective(indptr: torch.Tensor, indices: torch.Tensor,
                  values: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
                  lam: float = 0.01, alpha: float = 1.0,
                  implicit: bool = False) -> dict:
    """The training objective the solvers minimise (formulas above) for a
    whole user-major CSR: {"loss", "sq_err", "nnz"} plus "rmse" in
    explicit mode, as Python numbers. The residual sums come from
    als_residual_sums; the Gramians are gramian() in the factors' dtype;
    their Frobenius product and the row-norm sums are fp64."""
    sums = als_residual_sums(indptr, indices, values, X, Y, alpha, implicit)
    if implicit:
        reg = regulariser_sum(X, None) + regulariser_sum(Y, None)
        frob = (gramian(X).double() * gramian(Y).double()).sum()
    else:
        n_u = indptr[1:] - indptr[:-1]
        m_i = torch.bincount(indices.long(), minlength=Y.shape[0])
        reg = regulariser_sum(X, n_u) + regulariser_sum(Y, m_i)
        frob = torch.zeros((), dtype=torch.float64, device=X.device)
    A, B, reg, frob = torch.stack(
        [sums[0], sums[1], reg, frob]).tolist()
    return combine_objective(A, B, reg, frob, int(indices.shape[0]),
                             float(lam), implicit)


def build_csr(rows: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor,
              n_rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(row, col, val) triples → CSR (indptr i64, indices i32, values f32).

    Device-side sort-based build — torch.sort on GPU.
    """
    order = torch.argsort(rows)
    r = rows[order]
    indices = cols[order].to(torch.int32)
    values = vals[order].to(torch.float32)
    counts = torch.bincount(r.long(), minlength=n_rows)
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    torch.cumsum(counts, 0, out=indptr[1:])
    return indptr, indices, values


def aggregate_ratings(rows: torch.Tensor, cols: torch.Tensor,
                      vals: torch.Tensor, n_cols: int,
                      mode: str = "sum"):
    """Dedup (row, col) pairs: 'sum' (e-commerce reduceByKey semantics,
    ECommAlgorithm.scala:168-205) or 'latest' (similarproduct latest-wins,
    ALSAlgorithm.scala:88-120 — caller passes vals in time order)."""
    key = rows.long() * n_cols + cols.long()
    if mode == "sum":
        uk, inv = torch.unique(key, return_inverse=True)
        out = torch.zeros(uk.numel(), dtype=torch.float32, device=vals.device)
        out.scatter_add_(0, inv, vals.float())
    elif mode == "latest":
        # stable sort keeps time order within key; take last occurrence
        sk, order = torch.sort(key, stable=True)
        last = torch.ones(sk.numel(), dtype=torch.bool, device=key.device)
        last[:-1] = sk[1:] != sk[:-1]
        uk = sk[last]
        out = vals[order][last].float()
    else:
        raise ValueError(mode)
    return (uk // n_cols).to(rows.dtype), (uk % n_cols).to(cols.dtype), out
