// Nonnegative ALS half-step on MI355X (gfx950, CDNA4): per row
//
//     min 1/2 x^T A x - b^T x   subject to x >= 0
//
// with A and b the normal matrix and right-hand side of the unconstrained
// solvers (explicit: A = sum y y^T + lam n I, b = sum r y; implicit:
// A = YtY + sum alpha r y y^T + lam I, b = sum (1 + alpha r) y).
//
// Solver: block principal pivoting (Kim and Park) with the backup exchange
// rule. State per row: the passive set P (a bit per coordinate), x, the
// gradient y = A x - b, and two counters p (3) and ninf (F + 1). Starting
// from P = {}, x = 0, y = -b, every trip
//   1. marks the infeasible coordinates (x < 0 on P, y < 0 off P) and ends
//      when there are none;
//   2. flips all of them in P, or, once their number has failed to drop
//      for p trips in a row, only the one with the largest index;
//   3. solves A_PP x_P = b_P and recomputes y off P.
// Step 3 is one full-size Cholesky of M = P A P + (I - P) with right-hand
// side P b: rows and columns outside P are the identity's, selected per
// lane when the working copy is loaded. The instruction sequence of a trip
// does not depend on P, so control flow is wave-uniform throughout. The
// trip count is bounded by NNLS_MAX_IT; on reaching it the kernel writes
// max(x, 0). No loop here waits on anything but its own counter.
//
// Padded columns (rank 10 in F = 16) have a zero row in A and b = 0, so
// y = 0 there: y >= 0 counts as feasible, they never enter P, and their
// pivot is the mask's unit diagonal.
//
// Kernels:
//  - als_nnls_wave_kernel<F>, F <= 64: one wave per row, two per
//    workgroup. A lives in wave-private LDS (row stride F + 4, read as
//    b128 quads); lane i holds row i of the working copy M in registers;
//    pivots and x go out through literal-lane readlane; each lane keeps
//    dl = rsqrt(m_ii); finished L columns go to a second wave-private LDS
//    matrix for the trailing update (broadcast quads) and the back
//    substitution. The exchange decision is a ballot and two SGPR
//    counters; P is one 64-bit SGPR mask.
//  - als_nnls_block_kernel<128>: one 256-thread workgroup per row, A and M
//    both in LDS (row stride F + 1, so column walks are conflict-free);
//    P is two 64-bit masks.
//  - als_heavy_nnls_solve_kernel<F>: the heavy rows. The split-row Gramian
//    kernel of als_heavy.hip leaves the partials; this kernel adds them in
//    chunk order exactly as als_heavy_solve_kernel does (same workspace,
//    same carry slots) and runs the workgroup iteration body.
//
// A and b of the first two are built on the matrix pipe by the tile loop
// of als_heavy_gramian_kernel with the row in place of the chunk: column
// ids staged through LDS so the b128 factor-row gathers issue back to
// back, the next tile's gathers issued before the current tile's MFMAs,
// sum (w_a y_i) y_j on v_mfma_f32_32x32x2_f32 (16x16x4 at F = 16), tiles
// on and below the diagonal only. The staging tile shares its LDS with
// the matrix the solve overwrites first (L columns / M).
//
// All entry, row and slot offsets are 64-bit. This file includes only the
// HIP runtime and is built with packed fp32 VALU ops off.

#include <hip/hip_runtime.h>

#include <type_traits>

#define NNLS_MAX_IT 64  // trips per row; see docs/KERNELS.md

typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

extern "C" void launch_als_heavy_gramian(
    const long long* chunks, int n_chunks, const int* indices,
    const float* values, const float* Y, float* ws, int f, float alpha,
    int implicit_mode, hipStream_t stream);

namespace {

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int uniform_i32(int v) {
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ long long uniform_i64(long long v) {
  const unsigned int lo = (unsigned int)uniform_i32((int)(unsigned long long)v);
  const unsigned int hi =
      (unsigned int)uniform_i32((int)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
// lane k's value, k a literal after unrolling: one v_readlane_b32
__device__ __forceinline__ float lane_bcast(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

template <int F>
struct NnlsCfg {
  static constexpr int TS = F < 32 ? 16 : 32;      // output tile edge
  static constexpr int NT = F / TS;                // tiles per side
  static constexpr int NLT = NT * (NT + 1) / 2;    // tiles on/below diagonal
  static constexpr int KM = F < 32 ? 4 : 2;        // entries per MFMA
  static constexpr int AR = F < 32 ? 4 : 16;       // accumulators per tile
  static constexpr int LP = F + 4;                 // quad-read row stride
  static constexpr int SP = F + 1;                 // workgroup-body row stride
  static constexpr int NQ = F / 8;                 // b128 gathers per lane
  static constexpr int QR = F / 4;                 // quads per factor row
  static constexpr int NB = (F + 63) / 64;         // b columns per lane
  static constexpr int SR = F < 32 ? 32 : F;       // rows of the wave's L/tile
  static constexpr int SLOT = F * F + F;           // floats per heavy partial
  using acc_t = std::conditional_t<(F < 32), f32x4_t, f32x16_t>;
};

template <int F>
__device__ __forceinline__ typename NnlsCfg<F>::acc_t nnls_mfma(
    float a, float b, typename NnlsCfg<F>::acc_t c) {
  if constexpr (F < 32)
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// (row, col) inside its tile of accumulator e of lane l
template <int F>
__device__ __forceinline__ void frag_pos(int l, int e, int& row, int& col) {
  if constexpr (F < 32) {
    col = l & 15;
    row = 4 * (l >> 4) + e;
  } else {
    col = l & 31;
    row = (e & 3) + 8 * (e >> 2) + 4 * (l >> 5);
  }
}

// The row's 32-entry tiles wv, wv + NWV, ... into this wave's accumulators:
// acc[t] = sum (w_a y_i) y_j over tile t of the lower triangle, bacc the
// wave's share of b (lane = column). tile [32][LP], ids, was, wbs [32] are
// wave-private LDS. len >= 1 is not required (no tile, nothing read).
template <int F, int NWV>
__device__ __forceinline__ void nnls_gramian(
    const int* __restrict__ indices, const float* __restrict__ values,
    const float* __restrict__ Y, long long start, int len, float alpha,
    int implicit_mode, int wv, int lane, float* tile, int* ids, float* was,
    float* wbs, typename NnlsCfg<F>::acc_t (&acc)[NnlsCfg<F>::NLT],
    float (&bacc)[NnlsCfg<F>::NB])
{
  using C = NnlsCfg<F>;
  const int l32 = lane & 31;
  const int r = lane & (C::TS - 1);   // fragment row / column
  const int kh = lane / C::TS;        // fragment k: 0..KM-1
  const int ntiles = (len + 31) >> 5;

#pragma unroll
  for (int t = 0; t < C::NLT; ++t)
#pragma unroll
    for (int e = 0; e < C::AR; ++e) acc[t][e] = 0.f;
#pragma unroll
  for (int j = 0; j < C::NB; ++j) bacc[j] = 0.f;

  // entry l32 of tile n: id and weights. Entries past the row read its
  // last entry and weigh nothing.
  auto load_entry = [&](int n, int& id, float& wa, float& wb) {
    const int pos = n * 32 + l32;
    const bool live = pos < len;
    const long long p = start + (live ? pos : len - 1);
    id = indices[p];
    const float rv = values[p];
    const float a = implicit_mode ? alpha * rv : 1.f;
    const float b = implicit_mode ? 1.f + alpha * rv : rv;
    wa = live ? a : 0.f;
    wb = live ? b : 0.f;
  };
  f32x4_t g[C::NQ];
  // gather the 32 rows named by ids: quad q = lane + 64 j of the tile
  auto gather = [&]() {
#pragma unroll
    for (int j = 0; j < C::NQ; ++j) {
      const int q = lane + 64 * j;
      const long long col = ids[q / C::QR];
      g[j] = *reinterpret_cast<const f32x4_t*>(
          Y + col * F + 4 * (q % C::QR));
    }
  };

  int n = wv;
  int id2 = 0;
  float wa1 = 0.f, wb1 = 0.f, wa2 = 0.f, wb2 = 0.f;
  if (n < ntiles) {
    int id1;
    load_entry(n, id1, wa1, wb1);
    if (lane < 32) ids[lane] = id1;
    wave_sync();
    gather();
    if (n + NWV < ntiles) load_entry(n + NWV, id2, wa2, wb2);
  }
  for (; n < ntiles; n += NWV) {
    // stage tile n
#pragma unroll
    for (int j = 0; j < C::NQ; ++j) {
      const int q = lane + 64 * j;
      *reinterpret_cast<f32x4_t*>(
          &tile[(q / C::QR) * C::LP + 4 * (q % C::QR)]) = g[j];
    }
    if (lane < 32) {
      was[lane] = wa1;
      wbs[lane] = wb1;
    }
    // the wave's next tile: gathers now, ids of the one after it
    if (n + NWV < ntiles) {
      if (lane < 32) ids[lane] = id2;
      wa1 = wa2;
      wb1 = wb2;
      wave_sync();
      gather();
      if (n + 2 * NWV < ntiles) load_entry(n + 2 * NWV, id2, wa2, wb2);
    }
    wave_sync();

    // A: lane (r, kh) feeds entry p KM + kh of the tile
#pragma unroll 4
    for (int p = 0; p < 32 / C::KM; ++p) {
      const int e = p * C::KM + kh;
      const float w = was[e];
      float v[C::NT], a[C::NT];
#pragma unroll
      for (int t = 0; t < C::NT; ++t) {
        v[t] = tile[e * C::LP + t * C::TS + r];
        a[t] = w * v[t];
      }
      int idx = 0;
#pragma unroll
      for (int ti = 0; ti < C::NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj) {
          acc[idx] = nnls_mfma<F>(a[ti], v[tj], acc[idx]);
          ++idx;
        }
    }
    // b: lane = column
#pragma unroll
    for (int j = 0; j < C::NB; ++j) {
      const int c = lane + 64 * j;
      if (c < F) {
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < 32; ++k)
          s = fmaf(wbs[k], tile[k * C::LP + c], s);
        bacc[j] += s;
      }
    }
    wave_sync();   // the next trip overwrites the tile
  }
}

// The wave's accumulators into a full symmetric matrix D (row stride ld):
// stored (first) or added to what the waves before it left.
template <int F>
__device__ __forceinline__ void nnls_deposit(
    const typename NnlsCfg<F>::acc_t (&acc)[NnlsCfg<F>::NLT], float* D,
    int ld, int lane, bool first)
{
  using C = NnlsCfg<F>;
  int idx = 0;
#pragma unroll
  for (int ti = 0; ti < C::NT; ++ti)
#pragma unroll
    for (int tj = 0; tj <= ti; ++tj) {
#pragma unroll
      for (int e = 0; e < C::AR; ++e) {
        int row, col;
        frag_pos<F>(lane, e, row, col);
        const int gi = ti * C::TS + row;
        const int gj = tj * C::TS + col;
        const float val = (first ? 0.f : D[gi * ld + gj]) + acc[idx][e];
        D[gi * ld + gj] = val;
        if (ti != tj) D[gj * ld + gi] = val;
      }
      ++idx;
    }
}

// rows base + l whose degree is <= hi, as a wave-uniform mask
__device__ __forceinline__ unsigned long long nnls_rows_mask(
    const long long* __restrict__ indptr, long long base, int n_rows,
    int lane, int hi) {
  const long long r = base + lane;
  const long long r0 = r < n_rows ? r : n_rows;
  const long long r1 = r + 1 < n_rows ? r + 1 : n_rows;
  const int deg = (int)(indptr[r1] - indptr[r0]);
  return __builtin_amdgcn_ballot_w64(r < n_rows && deg <= hi);
}

// 2 waves x (A + L) x 4 B: 9.6 / 18.4 / 69.6 KB at F = 16 / 32 / 64
template <int F>
__global__ __launch_bounds__(128) void als_nnls_wave_kernel(
    const long long* __restrict__ indptr,
    const int* __restrict__ indices,
    const float* __restrict__ values,
    const float* __restrict__ Y,
    const float* __restrict__ YtY,
    float* __restrict__ X,
    int* __restrict__ iters,     // trips per row, or nullptr
    int n_rows,
    float lambda,
    float alpha,
    int implicit_mode,
    int wr_scale,
    int skip_above)              // rows with nnz > this are heavy
{
  using C = NnlsCfg<F>;
  using acc_t = typename C::acc_t;
  static_assert(F <= 64, "one wave per row needs rank <= 64");
  constexpr int LP = C::LP;
  __shared__ __attribute__((aligned(16))) float As[2][F * LP];
  // staging tile of the build, then Ls[k][j] = L[j][k]
  __shared__ __attribute__((aligned(16))) float Ls[2][C::SR * LP];
  __shared__ int ids[2][32];
  __shared__ float was[2][32];
  __shared__ float wbs[2][32];

  const int lane = threadIdx.x & 63;
  const int wave = uniform_i32((int)(threadIdx.x >> 6));
  float* A = As[wave];
  float* L = Ls[wave];
  const int li = lane < F ? lane : 0;    // the row this lane reads
  const int lc = lane < F ? lane : F;    // lanes >= F park in the pad column

  for (long long base = ((long long)blockIdx.x * 2 + wave) * 64;
       base < n_rows; base += (long long)gridDim.x * 128) {
    unsigned long long todo =
        nnls_rows_mask(indptr, base, n_rows, lane, skip_above);
  while (todo != 0) {
    const long long row = base + __builtin_ctzll(todo);
    todo &= todo - 1;
    const long long start = uniform_i64(indptr[row]);
    const int nnz = uniform_i32((int)(indptr[row + 1] - start));
    if (nnz == 0) {   // b = 0: x = 0 is the minimiser, no solve
      if (lane < F) X[row * (long long)F + lane] = 0.f;
      if (iters != nullptr && lane == 0) iters[row] = 0;
      continue;
    }

    // ---- A and b on the matrix pipe ----
    float b;
    {
      acc_t acc[C::NLT];
      float bacc[C::NB];
      nnls_gramian<F, 1>(indices, values, Y, start, nnz, alpha,
                         implicit_mode, 0, lane, L, ids[wave], was[wave],
                         wbs[wave], acc, bacc);
      nnls_deposit<F>(acc, A, LP, lane, true);
      b = lane < F ? bacc[0] : 0.f;
    }
    wave_sync();
    // YtY base (implicit) and the regulariser: lane i owns row i
    if (lane < F) {
      const float reg = wr_scale ? lambda * (float)nnz : lambda;
#pragma unroll
      for (int q = 0; q < F / 4; ++q) {
        f32x4_t a4 = *reinterpret_cast<f32x4_t*>(&A[lane * LP + 4 * q]);
        if (YtY != nullptr)
          a4 += *reinterpret_cast<const f32x4_t*>(
              &YtY[(long long)lane * F + 4 * q]);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (4 * q + c == lane) a4[c] += reg;
        *reinterpret_cast<f32x4_t*>(&A[lane * LP + 4 * q]) = a4;
      }
    }
    wave_sync();

    // ---- block principal pivoting ----
    unsigned long long P = 0;
    int p = 3, ninf = F + 1, it;
    float x = 0.f, y = -b;
    for (it = 0; it < NNLS_MAX_IT; ++it) {
      const bool was_in = (P >> lane) & 1;
      const bool bad = lane < F && (was_in ? x < 0.f : y < 0.f);
      const unsigned long long badm = __builtin_amdgcn_ballot_w64(bad);
      if (badm == 0) break;
      const int nb = __builtin_popcountll(badm);
      unsigned long long sw = badm;
      if (nb < ninf) {
        ninf = nb;
        p = 3;
      } else if (p > 0) {
        --p;
      } else {
        sw = 1ull << (63 - __builtin_clzll(badm));   // backup rule
      }
      P ^= sw;
      const bool in = (P >> lane) & 1;
      // == lane, but opaque and formed in this trip, so the per-k lane
      // compares of the solve are made where they are used: hoisted out
      // of the loop, the 3 F exec masks overflow the SGPR file
      int ln = lane;
      asm volatile("" : "+v"(ln));

      // lane's row of M = P A P + (I - P), rhs = P b
      float m[F];
#pragma unroll
      for (int q = 0; q < F / 4; ++q) {
        const f32x4_t a4 =
            *reinterpret_cast<const f32x4_t*>(&A[li * LP + 4 * q]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = 4 * q + c;
          const bool pj = (P >> j) & 1;   // literal j: a scalar test
          m[j] = (in && pj) ? a4[c] : (j == ln ? 1.f : 0.f);
        }
      }
      float r = in ? b : 0.f;

      // Cholesky: pivot by literal-lane readlane, L strictly lower, each
      // lane keeps dl = 1 / L[lane][lane]. Slot k holds L[lane][k] after
      // step k; column k also goes to LDS for the trailing update (quads
      // all lanes read alike) and the back substitution.
      float dl = 0.f;
#pragma unroll
      for (int k = 0; k < F; ++k) {
        float lkk = lane_bcast(m[k], k);
        lkk = lkk > 1e-30f ? lkk : 1e-30f;   // no pivot is 0
        const float dinv = rsqrtf(lkk);
        const float ljk = ln > k ? m[k] * dinv : 0.f;
        dl = ln == k ? dinv : dl;
        L[k * LP + lc] = ljk;
        m[k] = ljk;
        wave_sync();
#pragma unroll
        for (int m4 = (k + 1) & ~3; m4 < F; m4 += 4) {
          const f32x4_t lq =
              *reinterpret_cast<const f32x4_t*>(&L[k * LP + m4]);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (m4 + c > k) m[m4 + c] = fmaf(-ljk, lq[c], m[m4 + c]);
        }
        wave_sync();
      }
      // L z = rhs: a register chain
#pragma unroll
      for (int k = 0; k < F; ++k) {
        const float zk = lane_bcast(r * dl, k);
        r = fmaf(-m[k], zk, r);
      }
      r *= dl;
      // L^T x = z: lane j walks Ls[j][k] = L[k][j], consecutive over k
      {
        f32x4_t lq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = F - 1; k >= 0; --k) {
          if ((k & 3) == 3)
            lq = *reinterpret_cast<const f32x4_t*>(&L[li * LP + (k & ~3)]);
          const float xk = lane_bcast(r * dl, k);
          r = fmaf(ln < k ? -lq[k & 3] : 0.f, xk, r);
        }
        r *= dl;
      }
      wave_sync();   // the next trip's column stores follow these reads
      x = in ? r : 0.f;
      // y = A x - b off P, over the unspoiled A
      float s = -b;
#pragma unroll
      for (int q = 0; q < F / 4; ++q) {
        const f32x4_t a4 =
            *reinterpret_cast<const f32x4_t*>(&A[li * LP + 4 * q]);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          s = fmaf(a4[c], lane_bcast(x, 4 * q + c), s);
      }
      y = in ? 0.f : s;
    }
    if (lane < F) X[row * (long long)F + lane] = x > 0.f ? x : 0.f;
    if (iters != nullptr && lane == 0) iters[row] = it;
    wave_sync();   // the next row's build overwrites L
  }  // rows of the block
  }
}

// ---------------------------------------------------------------------------
// Workgroup iteration body: 256 threads, A (full, symmetric) and the
// working copy M in LDS with row stride F + 1, b in bs. Leaves max(x, 0)
// in xout[0..F) and returns the trip count (uniform). Every thread of the
// workgroup must call it; it ends on a barrier-free path only after one.
// ---------------------------------------------------------------------------
template <int F>
__device__ __forceinline__ int nnls_block_iterate(
    const float* A, float* M, const float* bs, float* rs, float* zs,
    float* xs, float* dinv, unsigned long long* bm, int tid, float* xout)
{
  constexpr int SP = NnlsCfg<F>::SP;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const bool own = tid < F;   // thread i < F owns coordinate i
  unsigned long long P0 = 0, P1 = 0;
  auto in_set = [&](int i) -> bool {
    return ((i < 64 ? P0 : P1) >> (i & 63)) & 1;
  };
  int p = 3, ninf = F + 1, it;
  float x = 0.f, y = own ? -bs[tid] : 0.f;
  for (it = 0; it < NNLS_MAX_IT; ++it) {
    const bool was_in = own && in_set(tid);
    const bool bad = own && (was_in ? x < 0.f : y < 0.f);
    const unsigned long long bw = __builtin_amdgcn_ballot_w64(bad);
    if (lane == 0 && wave < 2) bm[wave] = bw;
    __syncthreads();
    const unsigned long long b0 = (unsigned long long)uniform_i64(bm[0]);
    const unsigned long long b1 = (unsigned long long)uniform_i64(bm[1]);
    if ((b0 | b1) == 0) break;
    const int nb = __builtin_popcountll(b0) + __builtin_popcountll(b1);
    unsigned long long s0 = b0, s1 = b1;
    if (nb < ninf) {
      ninf = nb;
      p = 3;
    } else if (p > 0) {
      --p;
    } else if (b1 != 0) {   // backup rule: the largest index alone
      s1 = 1ull << (63 - __builtin_clzll(b1));
      s0 = 0;
    } else {
      s0 = 1ull << (63 - __builtin_clzll(b0));
    }
    P0 ^= s0;
    P1 ^= s1;
    const bool in = own && in_set(tid);

    // M = P A P + (I - P), lower triangle; rhs = P b
    for (int e = tid; e < F * F; e += 256) {
      const int i = e / F;
      const int j = e % F;
      if (j <= i)
        M[i * SP + j] = (in_set(i) && in_set(j)) ? A[i * SP + j]
                                                 : (i == j ? 1.f : 0.f);
    }
    if (own) rs[tid] = in ? bs[tid] : 0.f;

    // right-looking Cholesky: 16 x 16 threads over the trailing block
    const int ty = tid >> 4;
    const int tx = tid & 15;
    for (int k = 0; k < F; ++k) {
      __syncthreads();
      float d = M[k * SP + k];
      d = d > 0.f ? sqrtf(d) : 1e-20f;   // no pivot is 0
      const float di = 1.f / d;
      if (tid == k) dinv[k] = di;
      if (tid > k && own) M[tid * SP + k] *= di;
      __syncthreads();
      for (int i = k + 1 + ty; i < F; i += 16) {
        const float lik = M[i * SP + k];
        for (int j = k + 1 + tx; j <= i; j += 16)
          M[i * SP + j] = fmaf(-lik, M[j * SP + k], M[i * SP + j]);
      }
    }
    // L z = rhs
    for (int k = 0; k < F; ++k) {
      __syncthreads();
      const float zk = rs[k] * dinv[k];
      if (tid == k) zs[k] = zk;
      if (tid > k && own) rs[tid] = fmaf(-M[tid * SP + k], zk, rs[tid]);
    }
    // L^T x = z
    for (int k = F - 1; k >= 0; --k) {
      __syncthreads();
      const float xk = zs[k] * dinv[k];
      if (tid == k) xs[k] = xk;
      if (tid < k) zs[tid] = fmaf(-M[k * SP + tid], xk, zs[tid]);
    }
    __syncthreads();
    x = in ? xs[tid] : 0.f;
    __syncthreads();
    if (own) xs[tid] = x;
    __syncthreads();
    // y = A x - b off P: A is symmetric, so thread i walks column i
    if (own) {
      float s = -bs[tid];
      for (int j = 0; j < F; ++j) s = fmaf(A[j * SP + tid], xs[j], s);
      y = in ? 0.f : s;
    }
  }
  if (own) xout[tid] = x > 0.f ? x : 0.f;
  return it;
}

// A (65.0 KB) + M / staging (66.0 KB) at F = 128: one workgroup per CU
template <int F>
__global__ __launch_bounds__(256) void als_nnls_block_kernel(
    const long long* __restrict__ indptr,
    const int* __restrict__ indices,
    const float* __restrict__ values,
    const float* __restrict__ Y,
    const float* __restrict__ YtY,
    float* __restrict__ X,
    int* __restrict__ iters,
    int n_rows,
    float lambda,
    float alpha,
    int implicit_mode,
    int wr_scale,
    int skip_above)
{
  using C = NnlsCfg<F>;
  using acc_t = typename C::acc_t;
  constexpr int SP = C::SP;
  static_assert(F >= 128, "four 32-row staging tiles fit M");
  __shared__ float As[F * SP];
  // four wave-private staging tiles during the build, then M
  __shared__ __attribute__((aligned(16))) float Ms[4 * 32 * C::LP];
  static_assert(4 * 32 * C::LP >= F * SP, "M fits the staging tiles");
  __shared__ int ids[4][32];
  __shared__ float was[4][32];
  __shared__ float wbs[4][32];
  __shared__ float bs[F], rs[F], zs[F], xs[F], dinv[F];
  __shared__ unsigned long long bm[2];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = uniform_i32(tid >> 6);

  for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const long long start = uniform_i64(indptr[row]);
    const int nnz = uniform_i32((int)(indptr[row + 1] - start));
    if (nnz > skip_above) continue;
    if (nnz == 0) {
      if (tid < F) X[row * (long long)F + tid] = 0.f;
      if (iters != nullptr && tid == 0) iters[row] = 0;
      continue;
    }
    {
      acc_t acc[C::NLT];
      float bacc[C::NB];
      nnls_gramian<F, 4>(indices, values, Y, start, nnz, alpha,
                         implicit_mode, wave, lane, Ms + wave * 32 * C::LP,
                         ids[wave], was[wave], wbs[wave], acc, bacc);
      // the four waves in wave order
      for (int w = 0; w < 4; ++w) {
        if (wave == w) {
          nnls_deposit<F>(acc, As, SP, lane, w == 0);
#pragma unroll
          for (int j = 0; j < C::NB; ++j) {
            const int c = lane + 64 * j;
            if (c < F) bs[c] = (w == 0 ? 0.f : bs[c]) + bacc[j];
          }
        }
        __syncthreads();
      }
    }
    // YtY base (its lower triangle, both ways) and the regulariser
    {
      const float reg = wr_scale ? lambda * (float)nnz : lambda;
      for (int e = tid; e < F * F; e += 256) {
        const int i = e / F;
        const int j = e % F;
        float v = As[i * SP + j];
        if (YtY != nullptr) v += YtY[i > j ? i * F + j : j * F + i];
        As[i * SP + j] = i == j ? v + reg : v;
      }
    }
    __syncthreads();
    const int it = nnls_block_iterate<F>(As, Ms, bs, rs, zs, xs, dinv, bm,
                                         tid, X + row * (long long)F);
    if (iters != nullptr && tid == 0) iters[row] = it;
    __syncthreads();   // the next row's build overwrites M and A
  }
}

// The heavy rows: partials of als_heavy_gramian_kernel in chunk order,
// carry slots and batch walk as in als_heavy_solve_kernel.
template <int F>
__global__ __launch_bounds__(256) void als_heavy_nnls_solve_kernel(
    const long long* __restrict__ rows,       // heavy row -> row of X
    const long long* __restrict__ chunk_ptr,  // heavy row -> first chunk
    const long long* __restrict__ chunks,     // [n_chunks][2]
    const float* __restrict__ ws,             // slots of chunks [c0, c1)
    float* __restrict__ carry,                // [2][F*F + F]
    const float* __restrict__ YtY,            // F x F or nullptr
    float* __restrict__ X,
    int* __restrict__ iters,
    int r0,                                   // first heavy row of the batch
    long long c0, long long c1,               // the batch's chunks
    int parity,                               // batch number & 1
    float lambda,
    int wr_scale)
{
  using C = NnlsCfg<F>;
  constexpr int SP = C::SP;
  __shared__ float As[F * SP];
  __shared__ float Ms[F * SP];
  __shared__ float bs[F], rs[F], zs[F], xs[F], dinv[F];
  __shared__ unsigned long long bm[2];

  const int tid = threadIdx.x;
  const long long h = (long long)r0 + blockIdx.x;
  const long long fc = chunk_ptr[h];
  const long long lc = chunk_ptr[h + 1];
  const long long a = fc > c0 ? fc : c0;
  const long long b = lc < c1 ? lc : c1;
  const bool use_carry = fc < c0;    // the row began in an earlier batch
  const bool finalize = lc <= c1;    // and ends in this one
  const float* cin = carry + (parity ^ 1) * C::SLOT;
  float* cout = carry + parity * C::SLOT;

  if (tid < 2) bm[tid] = 0;
  // partials in chunk order
  for (int i = tid; i < C::SLOT; i += 256) {
    float s = use_carry ? cin[i] : 0.f;
    long long c = a;
    for (; c + 8 <= b; c += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ws[(c + u - c0) * C::SLOT + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < b; ++c) s += ws[(c - c0) * C::SLOT + i];
    if (!finalize) {
      cout[i] = s;
    } else if (i < F * F) {
      const int gi = i / F;
      const int gj = i % F;
      if (YtY != nullptr) s += YtY[gi > gj ? gi * F + gj : gj * F + gi];
      As[gi * SP + gj] = s;
    } else {
      bs[i - F * F] = s;
    }
  }
  if (!finalize) return;
  __syncthreads();
  if (tid < F) {
    const long long deg = chunks[2 * (lc - 1) + 1] - chunks[2 * fc];
    As[tid * SP + tid] += wr_scale ? lambda * (float)deg : lambda;
  }
  __syncthreads();
  const int it = nnls_block_iterate<F>(As, Ms, bs, rs, zs, xs, dinv, bm, tid,
                                       X + rows[h] * F);
  if (iters != nullptr && tid == 0) iters[rows[h]] = it;
}

template <int F>
void launch_heavy_nnls(const long long* chunks, const long long* chunk_ptr,
                       const long long* rows, const long long* chunk_ptr_host,
                       int n_heavy, const int* indices, const float* values,
                       const float* Y, const float* YtY, float* X, int* iters,
                       float* ws, long long ws_slots, float* carry,
                       float lambda, float alpha, int implicit_mode,
                       int wr_scale, hipStream_t stream) {
  const long long n_chunks = chunk_ptr_host[n_heavy];
  int r0 = 0;
  int batch = 0;
  for (long long c0 = 0; c0 < n_chunks; ++batch) {
    const long long c1 = c0 + ws_slots < n_chunks ? c0 + ws_slots : n_chunks;
    // heavy rows with a chunk in [c0, c1): r0 holds chunk c0
    while (chunk_ptr_host[r0 + 1] <= c0) ++r0;
    int r1 = r0 + 1;
    while (r1 < n_heavy && chunk_ptr_host[r1] < c1) ++r1;
    launch_als_heavy_gramian(chunks + 2 * c0, (int)(c1 - c0), indices, values,
                             Y, ws, F, alpha, implicit_mode, stream);
    hipLaunchKernelGGL((als_heavy_nnls_solve_kernel<F>), dim3(r1 - r0),
                       dim3(256), 0, stream, rows, chunk_ptr, chunks, ws,
                       carry, YtY, X, iters, r0, c0, c1, batch & 1, lambda,
                       wr_scale);
    c0 = c1;
  }
}

}  // namespace

extern "C" int als_nnls_max_it() { return NNLS_MAX_IT; }

// Every row of degree <= skip_above; rows above it are left alone.
extern "C" void launch_als_nnls(
    const long long* indptr, const int* indices, const float* values,
    const float* Y, const float* YtY, float* X, int* iters, int n_rows,
    int f, float lambda, float alpha, int implicit_mode, int wr_scale,
    int skip_above, hipStream_t stream)
{
  if (n_rows <= 0) return;
  const long long wg = ((long long)n_rows + 127) / 128;
  const int grid_w = (int)(wg < (1 << 20) ? wg : (1 << 20));
  const int grid_b = n_rows < (1 << 20) ? n_rows : (1 << 20);
#define NNLS_WAVE(FF)                                                        \
  hipLaunchKernelGGL((als_nnls_wave_kernel<FF>), dim3(grid_w), dim3(128), 0, \
                     stream, indptr, indices, values, Y, YtY, X, iters,      \
                     n_rows, lambda, alpha, implicit_mode, wr_scale,         \
                     skip_above)
  switch (f) {
    case 16: NNLS_WAVE(16); break;
    case 32: NNLS_WAVE(32); break;
    case 64: NNLS_WAVE(64); break;
    case 128:
      hipLaunchKernelGGL((als_nnls_block_kernel<128>), dim3(grid_b),
                         dim3(256), 0, stream, indptr, indices, values, Y,
                         YtY, X, iters, n_rows, lambda, alpha, implicit_mode,
                         wr_scale, skip_above);
      break;
    default: break;  // caller validates
  }
#undef NNLS_WAVE
}

// Same tables, workspace and carry buffer as launch_als_heavy.
extern "C" void launch_als_heavy_nnls(
    const long long* chunks, const long long* chunk_ptr,
    const long long* rows, const long long* chunk_ptr_host, int n_heavy,
    const int* indices, const float* values, const float* Y,
    const float* YtY, float* X, int* iters, float* ws, long long ws_slots,
    float* carry, int f, float lambda, float alpha, int implicit_mode,
    int wr_scale, hipStream_t stream)
{
  if (n_heavy <= 0 || ws_slots <= 0) return;
#define HEAVY_NNLS(FF)                                                       \
  launch_heavy_nnls<FF>(chunks, chunk_ptr, rows, chunk_ptr_host, n_heavy,    \
                        indices, values, Y, YtY, X, iters, ws, ws_slots,     \
                        carry, lambda, alpha, implicit_mode, wr_scale, stream)
  switch (f) {
    case 16: HEAVY_NNLS(16); break;
    case 32: HEAVY_NNLS(32); break;
    case 64: HEAVY_NNLS(64); break;
    case 128: HEAVY_NNLS(128); break;
    default: break;  // caller validates
  }
#undef HEAVY_NNLS
}
