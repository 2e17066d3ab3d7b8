"""fp32-MFMA paths of the ALS solve: the row-transform kernel
(als_xform.hip) and the Woodbury kernel's MFMA Gramian on a wave's second
trip through its row loop."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs MI355X")

RANKS = [16, 32, 64, 128]
# one partial tile, both sides of the 32-row tile, three tiles with a tail,
# and more tiles than one workgroup pass with a 3-row tail
ROWS = [1, 31, 32, 33, 95, 4099]


def _ext():
    from predictionio_amd.ops import hip_ext
    return hip_ext()


@functools.lru_cache(maxsize=None)
def _int_problem(f):
    """Small-integer operands for the largest N, shared by every N (a
    prefix): all partial sums are exact in f32 (|sum| <= 128 * 16)."""
    g = torch.Generator().manual_seed(500 + f)
    A = torch.randint(-4, 5, (max(ROWS), f), generator=g)
    W = torch.randint(-4, 5, (f, f), generator=g)
    assert (W != W.t()).sum() > f * f // 2   # asymmetric, no c * I
    return A, W, A @ W   # int64


@requires_gpu
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("f", RANKS)
def test_row_transform_exact_layout(f, n):
    A, W, ref = _int_problem(f)
    out = _ext().als_row_transform(A[:n].float().cuda(), W.float().cuda())
    assert out.shape == (n, f) and out.dtype == torch.float32
    got = out.cpu().double()
    nbad = (got != ref[:n].double()).sum().item()
    print(f"f={f} n={n}: {nbad} wrong elements")
    assert nbad == 0


@requires_gpu
@pytest.mark.parametrize("f", RANKS)
def test_row_transform_random(f):
    """|out - ref64| <= f * 2^-23 * (|in| @ |W|): twice the standard bound
    of an f-term f32 fma chain."""
    n = 4099
    g = torch.Generator().manual_seed(900 + f)
    A = torch.randn((n, f), generator=g)
    W = torch.randn((f, f), generator=g)
    out = _ext().als_row_transform(A.cuda(), W.cuda()).cpu().double()
    ref = A.double() @ W.double()
    bound = f * 2.0 ** -23 * (A.double().abs() @ W.double().abs())
    ratio = ((out - ref).abs() / bound).max().item()
    print(f"f={f}: max |err| / bound = {ratio:.3f}")
    assert torch.isfinite(out).all()
    assert ((out - ref).abs() <= bound).all()


@requires_gpu
def test_row_transform_out_slice():
    f, total, lo, hi = 64, 200, 37, 140
    A, W, ref = _int_problem(f)
    buf = torch.full((total, f), float("nan"), device="cuda")
    res = _ext().als_row_transform(A[:hi - lo].float().cuda(),
                                   W.float().cuda(), buf[lo:hi])
    assert res.data_ptr() == buf[lo:hi].data_ptr()
    b = buf.cpu()
    assert torch.isnan(b[:lo]).all() and torch.isnan(b[hi:]).all()
    assert torch.equal(b[lo:hi].double(), ref[:hi - lo].double())


@requires_gpu
def test_row_transform_empty_and_rejects():
    ext = _ext()
    W = torch.eye(64, device="cuda")
    empty = ext.als_row_transform(torch.empty((0, 64), device="cuda"), W)
    assert empty.shape == (0, 64)
    A = torch.ones((8, 64), device="cuda")
    with pytest.raises(RuntimeError):      # non-contiguous in
        ext.als_row_transform(torch.ones((8, 128), device="cuda")[:, ::2], W)
    with pytest.raises(RuntimeError):      # wrong dtype
        ext.als_row_transform(A.double(), W.double())
    with pytest.raises(RuntimeError):      # unsupported rank
        ext.als_row_transform(torch.ones((8, 48), device="cuda"),
                              torch.eye(48, device="cuda"))
    with pytest.raises(RuntimeError):      # out of the wrong shape
        ext.als_row_transform(A, W, torch.empty((7, 64), device="cuda"))


# ---- Woodbury: a wave's second row must not see its first row's LDS ----

SECOND_TRIP = 1 << 21      # the launcher caps the grid at 2^20 workgroups
TAIL = 4096                # of two rows each: row r + 2^21 reuses row r's wave
# period 13 (2^21 = 5 mod 13): 32 then 1, 20 then 21, a 0; mean 8.3
PATTERN = [32, 1, 20, 21, 0, 2, 3, 4, 5, 6, 7, 4, 3]
N_COLS = 400
LAM, ALPHA = 0.05, 2.0


@functools.lru_cache(maxsize=None)
def _second_trip_problem():
    """CSR built on the GPU, shared by both modes and left unchanged."""
    n_rows = SECOND_TRIP + TAIL
    P = len(PATTERN)
    assert all(PATTERN[i] != PATTERN[(i + SECOND_TRIP) % P] for i in range(P))
    g = torch.Generator(device="cuda").manual_seed(4242)
    deg = torch.tensor(PATTERN, device="cuda")[
        torch.arange(n_rows, device="cuda") % P]
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(deg, 0, out=indptr[1:])
    nnz = int(indptr[-1])
    cols = torch.randint(0, N_COLS, (nnz,), generator=g, device="cuda",
                         dtype=torch.int32)
    vals = torch.rand(nnz, generator=g, device="cuda") * 3 + 0.5
    Y = torch.randn((N_COLS, 64), generator=g, device="cuda") / 8.0
    return indptr, cols, vals, Y


@requires_gpu
@pytest.mark.parametrize("implicit", [True, False])
def test_second_trip_through_row_loop(implicit):
    from predictionio_amd.ops import als as als_ops
    indptr, cols, vals, Y = _second_trip_problem()
    n_rows = indptr.shape[0] - 1
    kw = dict(lam=LAM, alpha=ALPHA, implicit=implicit)
    whole = als_ops.als_solve(indptr, cols, vals, Y, **kw)[SECOND_TRIP:]
    alone = als_ops.als_solve(indptr, cols, vals, Y,
                              row_range=(SECOND_TRIP, n_rows), **kw)
    assert whole.shape == alone.shape == (TAIL, 64)
    assert torch.isfinite(whole).all() and torch.isfinite(alone).all()
    ndiff = (whole.view(torch.int32) != alone.view(torch.int32)).sum().item()
    print(f"implicit={implicit}: {ndiff} differing words")
    assert ndiff == 0
