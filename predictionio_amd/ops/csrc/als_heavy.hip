// Split-row ALS solver for heavy rows on MI355X (gfx950, CDNA4).
//
// Every other ALS solver gives a row to one wave or one workgroup, which
// then walks the row's n rated columns one after another. A row with 10^5
// or 10^6 entries (a popular item) keeps that one unit busy while the rest
// of the device idles. Here such a row is cut into chunks of a fixed number
// of consecutive CSR entries and solved in two kernels:
//
//  1. als_heavy_gramian_kernel<F>: one 256-thread workgroup per chunk forms
//     the partial normal matrix A_c = sum w_a y y^T and right-hand side
//     b_c = sum w_b y and writes them to the workspace slot it owns. No
//     atomics. The weights are those of the fp32 kernels (explicit:
//     w_a = 1, w_b = r; implicit: w_a = alpha r, w_b = 1 + alpha r).
//
//     - The four waves split the chunk's 32-entry tiles (tile i goes to
//       wave i & 3) and run free of each other: ids, weights and the staged
//       factor rows live in wave-private LDS, ordered by wave barriers
//       only. One combine through LDS at the end, in wave order.
//     - Column ids go through LDS so that the tile's factor-row gathers
//       (b128, F/8 per lane) issue back to back. The gathers of the wave's
//       next tile are issued into registers before the current tile's
//       MFMAs, and the ids and values of the tile after that are loaded
//       at the same point, so no gather waits on an id load.
//     - A_c is exact fp32 on the matrix pipe: v_mfma_f32_32x32x2_f32
//       (16x16x4 at F = 16). The A operand is the staged value times w_a,
//       the B operand the staged value, so the sum is sum (w y_i) y_j as in
//       the fp32 kernels, r = 0 included. Only the tiles on or below the
//       diagonal are built (3 of 4 at F = 64, 10 of 16 at F = 128); the
//       store mirrors them.
//     - b_c is a column sum over the same LDS tile on the vector ALU.
//     - The tail tile clamps its loads to the chunk's last entry and zeroes
//       the weights of the entries past it.
//
//  2. als_heavy_solve_kernel<F>: one workgroup per heavy row adds the row's
//     partials in chunk order (a fixed order: a row's result does not
//     depend on the other rows of the call), adds YtY and the regulariser,
//     and runs a plain in-LDS Cholesky and the two substitutions. Heavy
//     rows are few; this kernel is simple, not fast.
//
// The launcher walks the chunk table in batches that fit the workspace: a
// Gramian launch, then one solve launch for the rows the batch touches. A
// row cut by a batch boundary carries its running sum (still in chunk
// order) to the next batch in one of two carry slots, alternating by
// batch, so the row that reads a carry and the row that writes one in the
// same launch never share a slot.
//
// All entry offsets, row offsets and slot offsets are 64-bit. This file
// includes only the HIP runtime and is built with packed fp32 VALU ops off.

#include <hip/hip_runtime.h>

#include <type_traits>

typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

namespace {

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
}

template <int F>
struct HeavyCfg {
  static constexpr int TS = F < 32 ? 16 : 32;      // output tile edge
  static constexpr int NT = F / TS;                // tiles per side
  static constexpr int NLT = NT * (NT + 1) / 2;    // tiles on/below diagonal
  static constexpr int KM = F < 32 ? 4 : 2;        // entries per MFMA
  static constexpr int AR = F < 32 ? 4 : 16;       // accumulators per tile
  static constexpr int LP = F + 4;                 // staged row stride
  static constexpr int NQ = F / 8;                 // b128 gathers per lane
  static constexpr int QR = F / 4;                 // quads per factor row
  static constexpr int NB = (F + 63) / 64;         // b columns per lane
  static constexpr int SLOT = F * F + F;           // floats per partial
  using acc_t = std::conditional_t<(F < 32), f32x4_t, f32x16_t>;
};

// D += A . B for one tile: a = (w y)[row], b = y[col]
template <int F>
__device__ __forceinline__ typename HeavyCfg<F>::acc_t heavy_mfma(
    float a, float b, typename HeavyCfg<F>::acc_t c) {
  if constexpr (F < 32)
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

template <int F>
__global__ __launch_bounds__(256) void als_heavy_gramian_kernel(
    const long long* __restrict__ chunks,   // [grid][2]: entry (start, end)
    const int* __restrict__ indices,
    const float* __restrict__ values,
    const float* __restrict__ Y,            // n_cols x F
    float* __restrict__ ws,                 // [grid][F*F + F]
    float alpha,
    int implicit_mode)
{
  using C = HeavyCfg<F>;
  using acc_t = typename C::acc_t;
  // wave-private staging; the end-of-chunk combine reuses it
  __shared__ float tile[4][32][C::LP];
  __shared__ int ids[4][32];
  __shared__ float was[4][32];
  __shared__ float wbs[4][32];
  __shared__ float bred[F];
  static_assert(C::NLT * C::AR * 64 <= 4 * 32 * C::LP, "combine fits tile");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31;
  const int r = lane & (C::TS - 1);   // fragment row / column
  const int kh = lane / C::TS;        // fragment k: 0..KM-1

  const long long cstart = chunks[2 * (long long)blockIdx.x];
  const long long cend = chunks[2 * (long long)blockIdx.x + 1];
  const int len = cend > cstart ? (int)(cend - cstart) : 0;
  const int ntiles = (len + 31) >> 5;

  acc_t acc[C::NLT];
#pragma unroll
  for (int t = 0; t < C::NLT; ++t)
#pragma unroll
    for (int e = 0; e < C::AR; ++e) acc[t][e] = 0.f;
  float bacc[C::NB];
#pragma unroll
  for (int j = 0; j < C::NB; ++j) bacc[j] = 0.f;

  // entry l32 of tile n: id and weights. Entries past the chunk read its
  // last entry and weigh nothing.
  auto load_entry = [&](int n, int& id, float& wa, float& wb) {
    const int pos = n * 32 + l32;
    const bool live = pos < len;
    const long long p = cstart + (live ? pos : len - 1);
    id = indices[p];
    const float rv = values[p];
    const float a = implicit_mode ? alpha * rv : 1.f;
    const float b = implicit_mode ? 1.f + alpha * rv : rv;
    wa = live ? a : 0.f;
    wb = live ? b : 0.f;
  };
  f32x4_t g[C::NQ];
  // gather the 32 rows named by ids[wave]: quad q = lane + 64 j of the tile
  auto gather = [&]() {
#pragma unroll
    for (int j = 0; j < C::NQ; ++j) {
      const int q = lane + 64 * j;
      const long long col = ids[wave][q / C::QR];
      g[j] = *reinterpret_cast<const f32x4_t*>(
          Y + col * F + 4 * (q % C::QR));
    }
  };

  int n = wave;
  int id2 = 0;
  float wa1 = 0.f, wb1 = 0.f, wa2 = 0.f, wb2 = 0.f;
  if (n < ntiles) {
    int id1;
    load_entry(n, id1, wa1, wb1);
    if (lane < 32) ids[wave][lane] = id1;
    wave_sync();
    gather();
    if (n + 4 < ntiles) load_entry(n + 4, id2, wa2, wb2);
  }
  for (; n < ntiles; n += 4) {
    // stage tile n
#pragma unroll
    for (int j = 0; j < C::NQ; ++j) {
      const int q = lane + 64 * j;
      *reinterpret_cast<f32x4_t*>(&tile[wave][q / C::QR][4 * (q % C::QR)]) =
          g[j];
    }
    if (lane < 32) {
      was[wave][lane] = wa1;
      wbs[wave][lane] = wb1;
    }
    // the wave's next tile: gathers now, ids of the one after it
    if (n + 4 < ntiles) {
      if (lane < 32) ids[wave][lane] = id2;
      wa1 = wa2;
      wb1 = wb2;
      wave_sync();
      gather();
      if (n + 8 < ntiles) load_entry(n + 8, id2, wa2, wb2);
    }
    wave_sync();

    // A_c: lane (r, kh) feeds entry p KM + kh of the tile
#pragma unroll 4
    for (int p = 0; p < 32 / C::KM; ++p) {
      const int e = p * C::KM + kh;
      const float w = was[wave][e];
      float v[C::NT], a[C::NT];
#pragma unroll
      for (int t = 0; t < C::NT; ++t) {
        v[t] = tile[wave][e][t * C::TS + r];
        a[t] = w * v[t];
      }
      int idx = 0;
#pragma unroll
      for (int ti = 0; ti < C::NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj) {
          acc[idx] = heavy_mfma<F>(a[ti], v[tj], acc[idx]);
          ++idx;
        }
    }
    // b_c: lane = column
#pragma unroll
    for (int j = 0; j < C::NB; ++j) {
      const int c = lane + 64 * j;
      if (c < F) {
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < 32; ++k)
          s = fmaf(wbs[wave][k], tile[wave][k][c], s);
        bacc[j] += s;
      }
    }
    wave_sync();   // the next trip overwrites the tile
  }

  // combine the four waves in wave order, fragment layout kept
  float* red = &tile[0][0][0];
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < C::NLT; ++t)
#pragma unroll
        for (int e = 0; e < C::AR; ++e) {
          const int i = (t * C::AR + e) * 64 + lane;
          red[i] = (w == 0 ? 0.f : red[i]) + acc[t][e];
        }
#pragma unroll
      for (int j = 0; j < C::NB; ++j) {
        const int c = lane + 64 * j;
        if (c < F) bred[c] = (w == 0 ? 0.f : bred[c]) + bacc[j];
      }
    }
    __syncthreads();
  }

  // store, mirroring the tiles below the diagonal
  float* slot = ws + (long long)blockIdx.x * C::SLOT;
  for (int i = tid; i < C::NLT * C::AR * 64; i += 256) {
    const int l = i & 63;
    const int e = (i >> 6) % C::AR;
    const int t = i / (64 * C::AR);
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    int row, col;
    if constexpr (F < 32) {
      col = l & 15;
      row = 4 * (l >> 4) + e;
    } else {
      col = l & 31;
      row = (e & 3) + 8 * (e >> 2) + 4 * (l >> 5);
    }
    const int gi = ti * C::TS + row;
    const int gj = tj * C::TS + col;
    const float val = red[i];
    slot[gi * F + gj] = val;
    if (ti != tj) slot[gj * F + gi] = val;
  }
  for (int c = tid; c < F; c += 256) slot[F * F + c] = bred[c];
}

template <int F>
__global__ __launch_bounds__(256) void als_heavy_solve_kernel(
    const long long* __restrict__ rows,       // heavy row -> row of X
    const long long* __restrict__ chunk_ptr,  // heavy row -> first chunk
    const long long* __restrict__ chunks,     // [n_chunks][2]
    const float* __restrict__ ws,             // slots of chunks [c0, c1)
    float* __restrict__ carry,                // [2][F*F + F]
    const float* __restrict__ YtY,            // F x F or nullptr
    float* __restrict__ X,
    int r0,                                   // first heavy row of the batch
    long long c0, long long c1,               // the batch's chunks
    int parity,                               // batch number & 1
    float lambda,
    int wr_scale)
{
  using C = HeavyCfg<F>;
  __shared__ float As[F][F + 1];
  __shared__ float bs[F];
  __shared__ float zs[F];
  __shared__ float xs[F];
  __shared__ float dinv[F];

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

  // partials in chunk order
  for (int i = tid; i < C::SLOT; i += 256) {
    float s = use_carry ? cin[i] : 0.f;
    long long c = a;
    // eight loads in flight, added in chunk order all the same
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
      As[i / F][i % F] = s + (YtY != nullptr ? YtY[i] : 0.f);
    } else {
      bs[i - F * F] = s;
    }
  }
  if (!finalize) return;
  __syncthreads();
  if (tid < F) {
    const long long deg = chunks[2 * (lc - 1) + 1] - chunks[2 * fc];
    As[tid][tid] += wr_scale ? lambda * (float)deg : lambda;
  }

  // right-looking Cholesky, lower triangle
  for (int k = 0; k < F; ++k) {
    __syncthreads();
    float d = As[k][k];
    d = d > 0.f ? sqrtf(d) : 1e-20f;
    const float di = 1.f / d;
    if (tid == k) dinv[k] = di;
    if (tid > k && tid < F) As[tid][k] *= di;
    __syncthreads();
    const int rem = F - k - 1;
    for (int e = tid; e < rem * rem; e += 256) {
      const int i = k + 1 + e / rem;
      const int j = k + 1 + e % rem;
      if (j <= i) As[i][j] = fmaf(-As[i][k], As[j][k], As[i][j]);
    }
  }
  // L z = b
  for (int k = 0; k < F; ++k) {
    __syncthreads();
    const float zk = bs[k] * dinv[k];
    if (tid == k) zs[k] = zk;
    if (tid > k && tid < F) bs[tid] = fmaf(-As[tid][k], zk, bs[tid]);
  }
  // L^T x = z
  for (int k = F - 1; k >= 0; --k) {
    __syncthreads();
    const float xk = zs[k] * dinv[k];
    if (tid == k) xs[k] = xk;
    if (tid < k) zs[tid] = fmaf(-As[k][tid], xk, zs[tid]);
  }
  __syncthreads();
  if (tid < F) X[rows[h] * F + tid] = xs[tid];
}

template <int F>
void launch_heavy(const long long* chunks, const long long* chunk_ptr,
                  const long long* rows, const long long* chunk_ptr_host,
                  int n_heavy, const int* indices, const float* values,
                  const float* Y, const float* YtY, float* X, float* ws,
                  long long ws_slots, float* carry, float lambda, float alpha,
                  int implicit_mode, int wr_scale, hipStream_t stream) {
  const long long n_chunks = chunk_ptr_host[n_heavy];
  int r0 = 0;
  int batch = 0;
  for (long long c0 = 0; c0 < n_chunks; ++batch) {
    const long long c1 = c0 + ws_slots < n_chunks ? c0 + ws_slots : n_chunks;
    // heavy rows with a chunk in [c0, c1): r0 holds chunk c0
    while (chunk_ptr_host[r0 + 1] <= c0) ++r0;
    int r1 = r0 + 1;
    while (r1 < n_heavy && chunk_ptr_host[r1] < c1) ++r1;
    hipLaunchKernelGGL((als_heavy_gramian_kernel<F>), dim3((int)(c1 - c0)),
                       dim3(256), 0, stream, chunks + 2 * c0, indices,
                       values, Y, ws, alpha, implicit_mode);
    hipLaunchKernelGGL((als_heavy_solve_kernel<F>), dim3(r1 - r0), dim3(256),
                       0, stream, rows, chunk_ptr, chunks, ws, carry, YtY, X,
                       r0, c0, c1, batch & 1, lambda, wr_scale);
    c0 = c1;
  }
}

}  // namespace

// floats per workspace slot (one chunk's A_c and b_c); two of them make
// the carry buffer
extern "C" long long als_heavy_slot_floats(int f) {
  return (long long)f * f + f;
}

// The Gramian launch alone, over n_chunks chunks into ws slots 0.. in
// table order: for a solver of its own over the same partials (the
// nonnegative one in als_nnls.hip).
extern "C" void launch_als_heavy_gramian(
    const long long* chunks, int n_chunks, const int* indices,
    const float* values, const float* Y, float* ws, int f, float alpha,
    int implicit_mode, hipStream_t stream)
{
  if (n_chunks <= 0) return;
#define GRAMIAN(FF)                                                          \
  hipLaunchKernelGGL((als_heavy_gramian_kernel<FF>), dim3(n_chunks),         \
                     dim3(256), 0, stream, chunks, indices, values, Y, ws,   \
                     alpha, implicit_mode)
  switch (f) {
    case 16: GRAMIAN(16); break;
    case 32: GRAMIAN(32); break;
    case 64: GRAMIAN(64); break;
    case 128: GRAMIAN(128); break;
    default: break;  // caller validates
  }
#undef GRAMIAN
}

// chunk_ptr_host is chunk_ptr on the host: n_heavy + 1 ascending entries
// from 0, every row with at least one chunk. ws holds ws_slots >= 1 slots.
extern "C" void launch_als_heavy(
    const long long* chunks, const long long* chunk_ptr,
    const long long* rows, const long long* chunk_ptr_host, int n_heavy,
    const int* indices, const float* values, const float* Y,
    const float* YtY, float* X, float* ws, long long ws_slots, float* carry,
    int f, float lambda, float alpha, int implicit_mode, int wr_scale,
    hipStream_t stream)
{
  if (n_heavy <= 0 || ws_slots <= 0) return;
#define HEAVY(FF)                                                            \
  launch_heavy<FF>(chunks, chunk_ptr, rows, chunk_ptr_host, n_heavy,         \
                   indices, values, Y, YtY, X, ws, ws_slots, carry, lambda,  \
                   alpha, implicit_mode, wr_scale, stream)
  switch (f) {
    case 16: HEAVY(16); break;
    case 32: HEAVY(32); break;
    case 64: HEAVY(64); break;
    case 128: HEAVY(128); break;
    default: break;  // caller validates
  }
#undef HEAVY
}
