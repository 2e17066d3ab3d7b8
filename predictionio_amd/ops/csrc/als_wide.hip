// Dense ALS solver for factor ranks 129..256 on MI355X (gfx950, CDNA4).
//
// als_solve_kernel<F> keeps the whole F x (F + 4) normal matrix in LDS and
// its Gramian in 4x4 VALU register tiles; at F = 256 that is 266 KB of LDS
// against 160 KB per CU and 256 accumulators per thread. This kernel is the
// wider ranks' own design, F in {192, 256}:
//
//  - One 512-thread workgroup (8 waves) per row, persistent grid-stride.
//    The LDS admits one workgroup per CU, so the eight waves own the whole
//    register file: 256 registers per lane.
//
//  - The normal matrix lives in LDS as its lower triangle only, in 16x16
//    blocks stored block by block: block (bi, bj), bj <= bi, is the
//    contiguous 1 KB at index bi (bi + 1) / 2 + bj (136 blocks = 136 KB at
//    F = 256, 78 blocks = 78 KB at F = 192). Inside a block element (i, j)
//    sits at ((i >> 2) * 16 + j) * 4 + (i & 3): the C/D fragment order of
//    v_mfma_f32_16x16x4_f32, so a lane's four accumulators of a block are
//    one aligned b128.
//
//  - Gramian on the matrix cores, accumulators in registers. The tile loop
//    is that of als_heavy_gramian_kernel with the split turned round: all
//    eight waves read the same staged tile of 32 entries x F and the
//    OUTPUT blocks are dealt round the waves (block t to wave t & 7: 17
//    per wave at F = 256, 10 or 9 at F = 192; the loop body is instantiated
//    per wave, so a wave's block list is a constant and each staged column
//    slice it needs is read once per k-step). Column ids go through LDS so the
//    b128 gathers issue back to back; the next tile's gathers and the ids
//    and values of the tile after that are issued before the current
//    tile's MFMAs; the tail tile re-reads the row's last entry with weight
//    0. A = w_a y on the VALU, B = y, so the sum is sum (w_a y_i) y_j as in
//    the fp32 kernels. b is a column sum over the same staged tile. The
//    two staging buffers alias the triangle, which is not needed until the
//    deposit. Staged rows have stride F + 16 floats: a 16x16x4 fragment
//    read touches 4 entries x 16 columns at once, and a stride that is 16
//    modulo 32 banks puts them on distinct banks (F + 4 would fold them).
//
//  - Blocked Cholesky in place, panels of 16: (1) wave 0 factors the
//    diagonal block in registers, lane i holding row i, pivot columns
//    broadcast with v_readlane (no LDS trip, no s_barrier); pivots are
//    clamped as in als_solve_kernel and their reciprocals kept; (2) panel
//    solve, one row per thread; (3) rank-16 trailing update on the matrix
//    cores, four 16x16x4 fp32 MFMAs per block with C loaded from and D
//    stored to the block's own 1 KB, blocks dealt round the waves. Three
//    workgroup barriers per panel. The two substitutions are blocked the
//    same way (two barriers per panel); the back solve reads L^T from the
//    stored lower blocks.
//
// Every loop is bounded by its own counter, nothing waits on another
// workgroup and there are no atomics. A row's arithmetic depends on the
// row alone: not on the grid, the workgroup that ran it or the row range.
// Rows and rating offsets are 64-bit. This file includes only the HIP
// runtime and is built with packed fp32 VALU ops off.

#include <hip/hip_runtime.h>

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

namespace {

constexpr int WIDE_THREADS = 512;
constexpr int WIDE_WAVES = WIDE_THREADS / 64;

template <int F>
struct WideCfg {
  static constexpr int NBK = F / 16;                 // blocks per side
  static constexpr int NLB = NBK * (NBK + 1) / 2;    // on/below the diagonal
  static constexpr int NS = (NLB + WIDE_WAVES - 1) / WIDE_WAVES;
  static constexpr int LP = F + 16;                  // staged row stride
  static constexpr int QR = F / 4;                   // quads per factor row
  static constexpr int NQ = 32 * QR / WIDE_THREADS;  // b128 gathers per thread
  // LDS map, in floats
  static constexpr int TRI = NLB * 256;
  static constexpr int OFF_B = TRI;
  static constexpr int OFF_DINV = OFF_B + F;
  static constexpr int OFF_WA = OFF_DINV + F;        // [2][32]
  static constexpr int OFF_WB = OFF_WA + 64;         // [2][32]
  static constexpr int OFF_IDS = OFF_WB + 64;        // [2][32] int
  static constexpr int OFF_TAB = OFF_IDS + 64;       // [NLB] int
  static constexpr int LDS_FLOATS = OFF_TAB + NLB;
  static_assert(F % 64 == 0, "gathers split evenly over 512 threads");
  static_assert(NQ * WIDE_THREADS == 32 * QR, "whole tile gathered");
  static_assert(2 * 32 * LP <= TRI, "staging buffers alias the triangle");
  static_assert(LDS_FLOATS * 4 <= 160 * 1024, "one CU's LDS");
};

// element (i, j) of a 16x16 block: the MFMA C/D fragment order
__device__ __forceinline__ int bpos(int i, int j) {
  return (((i >> 2) * 16 + j) << 2) + (i & 3);
}
// float offset of block (bi, bj), bj <= bi, in the packed triangle
__device__ __forceinline__ int boff(int bi, int bj) {
  return (bi * (bi + 1) / 2 + bj) * 256;
}
// lane k's value as a wave-uniform scalar (one v_readlane_b32)
__device__ __forceinline__ float lane_bcast(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// row of the t-th block of a triangle laid out row by row; t is a literal
// wherever this is called, so it folds to a constant
__device__ __forceinline__ constexpr int tri_row(int t) {
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
  return bi;
}

// One staged tile into wave W's Gramian blocks W, W + 8, ... The block
// list is a compile-time constant per wave, so every staged column slice
// the wave needs is one ds_read at an immediate offset, read once per
// k-step and shared by all blocks in that block row or column.
template <int F, int W>
__device__ __forceinline__ void gram_tile(
    const float* st, const float* wa, int r, int kh,
    f32x4_t (&acc)[WideCfg<F>::NS]) {
  using C = WideCfg<F>;
  // lane (r, kh) feeds entry 4 p + kh of the tile
#pragma unroll 2
  for (int p = 0; p < 8; ++p) {
    const int e = 4 * p + kh;
    const float w = wa[e];
    const float* rp = st + e * C::LP + r;
    float v[C::NBK], a[C::NBK];
#pragma unroll
    for (int c = 0; c < C::NBK; ++c) {
      v[c] = rp[16 * c];
      a[c] = w * v[c];
    }
#pragma unroll
    for (int s = 0; s < C::NS; ++s) {
      const int t = W + WIDE_WAVES * s;
      if (t < C::NLB) {
        const int bi = tri_row(t);
        const int bj = t - bi * (bi + 1) / 2;
        acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[bi], v[bj], acc[s],
                                                      0, 0, 0);
      }
    }
  }
}

template <int F>
__global__ __launch_bounds__(WIDE_THREADS) void als_solve_wide_kernel(
    const long long* __restrict__ indptr,   // n_rows + 1
    const int* __restrict__ indices,
    const float* __restrict__ values,
    const float* __restrict__ Y,            // n_cols x F
    const float* __restrict__ YtY,          // F x F or nullptr
    float* __restrict__ X,                  // n_rows x F
    int n_rows,
    float lambda,
    float alpha,
    int implicit_mode,
    int wr_scale,
    int skip_below,                         // rows with nnz <= this and
    int skip_above)                         // rows with nnz > this are skipped
{
  using C = WideCfg<F>;
  extern __shared__ __align__(16) float lds[];
  float* tri = lds;
  float* bs = lds + C::OFF_B;
  float* dinv = lds + C::OFF_DINV;
  float* was = lds + C::OFF_WA;
  float* wbs = lds + C::OFF_WB;
  int* ids = reinterpret_cast<int*>(lds + C::OFF_IDS);
  int* tab = reinterpret_cast<int*>(lds + C::OFF_TAB);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15;    // fragment row (A) / column (B, D)
  const int kh = lane >> 4;   // fragment k; D rows 4 kh .. 4 kh + 3

  // tab[t] = (bi << 8) | bj of the t-th block of a triangle, row by row.
  // Block t of the whole matrix, and block t of any trailing triangle.
  for (int t = tid; t < C::NLB; t += WIDE_THREADS) {
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
    tab[t] = (bi << 8) | (t - bi * (bi + 1) / 2);
  }
  __syncthreads();
  for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const long long start = indptr[row];
    const long long end = indptr[row + 1];
    const int nnz = (int)(end - start);
    if (nnz <= skip_below || nnz > skip_above) continue;
    if (nnz == 0 && !implicit_mode) {   // no ratings: x = 0
      if (tid < F) X[row * (long long)F + tid] = 0.f;
      continue;
    }

    // ---- Gramian: 32-entry tiles, output blocks split over the waves ----
    f32x4_t acc[C::NS];
#pragma unroll
    for (int s = 0; s < C::NS; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[s][e] = 0.f;
    float bacc = 0.f;
    const int ntiles = (nnz + 31) >> 5;

    // entry (tid & 31) of tile n: id and weights. Entries past the row
    // read its last entry and weigh nothing.
    auto load_entry = [&](int n, int& id, float& wa, float& wb) {
      const int pos = n * 32 + (tid & 31);
      const bool live = pos < nnz;
      const long long p = start + (live ? pos : nnz - 1);
      id = indices[p];
      const float rv = values[p];
      const float a = implicit_mode ? alpha * rv : 1.f;
      const float b = implicit_mode ? 1.f + alpha * rv : rv;
      wa = live ? a : 0.f;
      wb = live ? b : 0.f;
    };
    f32x4_t g[C::NQ];
    // the 32 rows named by idb: quad q = tid + 512 j of the tile
    auto gather = [&](const int* idb) {
#pragma unroll
      for (int j = 0; j < C::NQ; ++j) {
        const int q = tid + WIDE_THREADS * j;
        const long long col = idb[q / C::QR];
        g[j] = *reinterpret_cast<const f32x4_t*>(
            Y + col * F + 4 * (q % C::QR));
      }
    };

    int id2 = 0;
    float wa1 = 0.f, wb1 = 0.f, wa2 = 0.f, wb2 = 0.f;
    if (ntiles > 0) {
      if (tid < 32) {
        int id1;
        load_entry(0, id1, wa1, wb1);
        ids[tid] = id1;
      }
      __syncthreads();
      gather(ids);
      if (ntiles > 1 && tid < 32) load_entry(1, id2, wa2, wb2);
    }
    for (int n = 0; n < ntiles; ++n) {
      const int buf = n & 1;
      float* st = tri + buf * 32 * C::LP;
      // stage tile n
#pragma unroll
      for (int j = 0; j < C::NQ; ++j) {
        const int q = tid + WIDE_THREADS * j;
        *reinterpret_cast<f32x4_t*>(
            st + (q / C::QR) * C::LP + 4 * (q % C::QR)) = g[j];
      }
      if (tid < 32) {
        was[buf * 32 + tid] = wa1;
        wbs[buf * 32 + tid] = wb1;
        if (n + 1 < ntiles) {
          ids[(buf ^ 1) * 32 + tid] = id2;
          wa1 = wa2;
          wb1 = wb2;
        }
      }
      // One barrier per tile. Everything written above was last read two
      // tiles ago (stage, weights) or by the gathers of the tile before
      // (ids), and every thread has passed a barrier since.
      __syncthreads();
      // the next tile: gathers now, ids and values of the one after it
      if (n + 1 < ntiles) {
        gather(ids + (buf ^ 1) * 32);
        if (n + 2 < ntiles && tid < 32) load_entry(n + 2, id2, wa2, wb2);
      }

      switch (wave) {
        case 0: gram_tile<F, 0>(st, was + buf * 32, r, kh, acc); break;
        case 1: gram_tile<F, 1>(st, was + buf * 32, r, kh, acc); break;
        case 2: gram_tile<F, 2>(st, was + buf * 32, r, kh, acc); break;
        case 3: gram_tile<F, 3>(st, was + buf * 32, r, kh, acc); break;
        case 4: gram_tile<F, 4>(st, was + buf * 32, r, kh, acc); break;
        case 5: gram_tile<F, 5>(st, was + buf * 32, r, kh, acc); break;
        case 6: gram_tile<F, 6>(st, was + buf * 32, r, kh, acc); break;
        default: gram_tile<F, 7>(st, was + buf * 32, r, kh, acc); break;
      }
      // b: thread = column
      if (tid < F) {
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < 32; ++k)
          s = fmaf(wbs[buf * 32 + k], st[k * C::LP + tid], s);
        bacc += s;
      }
    }
    __syncthreads();   // the staging buffers become the triangle

    // ---- deposit: + YtY, + regulariser on the diagonal ----
    {
      const float reg = wr_scale ? lambda * (float)nnz : lambda;
#pragma unroll
      for (int s = 0; s < C::NS; ++s) {
        const int t = wave + WIDE_WAVES * s;
        if (t < C::NLB) {
          f32x4_t v = acc[s];
          const int bb = __builtin_amdgcn_readfirstlane(tab[t]);
          const int gi = (bb >> 8) * 16 + 4 * kh;
          const int gj = (bb & 255) * 16 + r;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (YtY != nullptr) v[e] += YtY[(gi + e) * F + gj];
            if (gi + e == gj) v[e] += reg;
          }
          *reinterpret_cast<f32x4_t*>(tri + t * 256 + lane * 4) = v;
        }
      }
      if (tid < F) bs[tid] = bacc;
    }
    __syncthreads();

    // ---- blocked Cholesky in place, lower triangle, panels of 16 ----
    for (int k = 0; k < C::NBK; ++k) {
      const int k0 = 16 * k;
      float* dblk = tri + boff(k, k);
      if (wave == 0) {
        // (1) diagonal block in registers: lane i (and its copies at
        // i + 16, 32, 48, never stored) holds row i
        float a[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = dblk[bpos(r, j)];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          float d = lane_bcast(a[kk], kk);
          d = d > 0.f ? sqrtf(d) : 1e-20f;
          const float di = 1.f / d;
          const float lik = a[kk] * di;
          a[kk] = r == kk ? d : lik;
#pragma unroll
          for (int j = kk + 1; j < 16; ++j)
            a[j] = fmaf(-lik, lane_bcast(lik, j), a[j]);
          if (lane == 0) dinv[k0 + kk] = di;
        }
        if (lane < 16) {
#pragma unroll
          for (int j = 0; j < 16; ++j) dblk[bpos(r, j)] = a[j];
        }
      }
      __syncthreads();
      if (k == C::NBK - 1) break;   // no panel below the last block
      // (2) panel solve: row i of the blocks below <- row * L_kk^-T
      {
        const int i = k0 + 16 + tid;
        if (i < F) {
          float* pb = tri + boff(i >> 4, k);
          const int ri = i & 15;
          float w[16];
#pragma unroll
          for (int m = 0; m < 16; ++m) w[m] = pb[bpos(ri, m)];
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            float s = w[j];
#pragma unroll
            for (int m = 0; m < 16; ++m)
              if (m < j) s = fmaf(-w[m], dblk[bpos(j, m)], s);
            w[j] = s * dinv[k0 + j];
          }
#pragma unroll
          for (int m = 0; m < 16; ++m) pb[bpos(ri, m)] = w[m];
        }
      }
      __syncthreads();
      // (3) A[i][j] -= sum_m L[i][m] L[j][m] over the trailing triangle
      const int rem = C::NBK - k - 1;
      const int cnt = rem * (rem + 1) / 2;
      for (int u = wave; u < cnt; u += WIDE_WAVES) {
        const int v = __builtin_amdgcn_readfirstlane(tab[u]);
        const int bi = k + 1 + (v >> 8);
        const int bj = k + 1 + (v & 255);
        const float* pa = tri + boff(bi, k);
        const float* pb = tri + boff(bj, k);
        f32x4_t* pc =
            reinterpret_cast<f32x4_t*>(tri + boff(bi, bj) + lane * 4);
        f32x4_t c = *pc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = 4 * q + kh;
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(
              -pa[bpos(r, m)], pb[bpos(r, m)], c, 0, 0, 0);
        }
        *pc = c;
      }
      __syncthreads();
    }

    // ---- forward solve L z = b ----
    for (int k = 0; k < C::NBK; ++k) {
      const int k0 = 16 * k;
      if (wave == 0) {
        const float* dblk = tri + boff(k, k);
        float a[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = dblk[bpos(r, j)];
        float bv = bs[k0 + r];
        const float dl = dinv[k0 + r];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          const float zk = lane_bcast(bv * dl, kk);
          if (r == kk) bv = zk;
          if (r > kk) bv = fmaf(-a[kk], zk, bv);
        }
        if (lane < 16) bs[k0 + lane] = bv;
      }
      __syncthreads();
      const int j = k0 + 16 + tid;
      if (j < F) {
        const float* pb = tri + boff(j >> 4, k);
        const int rj = j & 15;
        float s = bs[j];
#pragma unroll
        for (int m = 0; m < 16; ++m)
          s = fmaf(-pb[bpos(rj, m)], bs[k0 + m], s);
        bs[j] = s;
      }
      __syncthreads();
    }
    // ---- back solve L^T x = z, L^T read from the lower blocks ----
    for (int k = C::NBK - 1; k >= 0; --k) {
      const int k0 = 16 * k;
      if (wave == 0) {
        const float* dblk = tri + boff(k, k);
        float c[16];   // column r of the block: c[m] = L[k0 + m][k0 + r]
#pragma unroll
        for (int m = 0; m < 16; ++m) c[m] = dblk[bpos(m, r)];
        float bv = bs[k0 + r];
        const float dl = dinv[k0 + r];
#pragma unroll
        for (int kk = 15; kk >= 0; --kk) {
          const float xk = lane_bcast(bv * dl, kk);
          if (r == kk) bv = xk;
          if (r < kk) bv = fmaf(-c[kk], xk, bv);
        }
        if (lane < 16) bs[k0 + lane] = bv;
      }
      __syncthreads();
      if (tid < k0) {
        const float* pb = tri + boff(k, tid >> 4);
        const int rj = tid & 15;
        float s = bs[tid];
#pragma unroll
        for (int m = 0; m < 16; ++m)
          s = fmaf(-pb[bpos(m, rj)], bs[k0 + m], s);
        bs[tid] = s;
      }
      __syncthreads();
    }

    if (tid < F) X[row * (long long)F + tid] = bs[tid];
    __syncthreads();   // the next row restages over the triangle
  }
}

template <int F>
void launch_wide(const long long* indptr, const int* indices,
                 const float* values, const float* Y, const float* YtY,
                 float* X, int n_rows, float lambda, float alpha,
                 int implicit_mode, int wr_scale, int skip_below,
                 int skip_above, int grid, hipStream_t stream) {
  constexpr size_t lds_bytes = WideCfg<F>::LDS_FLOATS * sizeof(float);
  // above the 64 KB default: raise the kernel's own limit to the CU's LDS
  (void)hipFuncSetAttribute(
      reinterpret_cast<const void*>(als_solve_wide_kernel<F>),
      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL((als_solve_wide_kernel<F>), dim3(grid),
                     dim3(WIDE_THREADS), lds_bytes, stream, indptr, indices,
                     values, Y, YtY, X, n_rows, lambda, alpha, implicit_mode,
                     wr_scale, skip_below, skip_above);
}

}  // namespace

// Dynamic LDS bytes of one workgroup (the docs and the probe quote it).
extern "C" int als_wide_lds_bytes(int f) {
  if (f == 192) return WideCfg<192>::LDS_FLOATS * (int)sizeof(float);
  if (f == 256) return WideCfg<256>::LDS_FLOATS * (int)sizeof(float);
  return 0;
}

// Rows with skip_below < nnz <= skip_above, one workgroup per row on a
// grid of `grid` persistent workgroups (the caller sizes it: one per CU).
extern "C" void launch_als_solve_wide(
    const long long* indptr, const int* indices, const float* values,
    const float* Y, const float* YtY, float* X, int n_rows, int f,
    float lambda, float alpha, int implicit_mode, int wr_scale,
    int skip_below, int skip_above, int grid, hipStream_t stream)
{
  if (n_rows <= 0 || grid <= 0) return;
#define WIDE(FF)                                                             \
  launch_wide<FF>(indptr, indices, values, Y, YtY, X, n_rows, lambda, alpha, \
                  implicit_mode, wr_scale, skip_below, skip_above, grid,     \
                  stream)
  switch (f) {
    case 192: WIDE(192); break;
    case 256: WIDE(256); break;
    default: break;  // caller validates
  }
#undef WIDE
}
