// Row transform out[N, F] = in[N, F] . W[F, F] for MI355X (gfx950, CDNA4).
//
// The two tall-skinny GEMMs of an implicit ALS half-iteration — whitening
// V = Y L^-T and the map back X = Z L^-1 — move N x F floats in and out
// against an F x F matrix that fits in registers. They are pure streaming
// problems (256 B in + 256 B out per row at F = 64 against 8 KFLOP), so
// the kernel is built around the memory stream, not around a GEMM tiling:
//
//  - persistent waves, each grid-striding over 32-row tiles; no LDS, no
//    barriers, no inter-wave cooperation;
//  - W lives in registers for the whole kernel, already laid out as the
//    MFMA fragment (F/2 VGPRs per 32-column tile);
//  - exact fp32 on the matrix pipe: v_mfma_f32_32x32x2_f32 (f32 in, f32
//    accumulate — bit-for-bit a k-ordered fmaf chain);
//  - the product is formed TRANSPOSED, D = W^T . in^T: W^T is the A
//    fragment and the data rows are the B fragment, so the C/D layout
//    (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
//    leaves lane (r, h) holding columns 8b + 4h .. 8b + 4h + 3 of data row
//    r in acc[4b .. 4b + 3] — contiguous quads, stored with b128 writes;
//  - the k sum may run in any order, so lane (r, h) loads row r's b128
//    quads at k = 8q + 4h (32 contiguous bytes per row per instruction)
//    and W's fragment follows the same k permutation;
//  - the next tile's loads are issued before the current tile's MFMAs,
//    and all of a tile's loads precede its stores.
//
// F = 16 uses the top-left 16 columns of one 32x32 tile; F = 128 spreads
// its four column tiles over the four waves of a workgroup (the W fragment
// of all four would not fit the register file), which then share one row
// tile through L1.

#include <hip/hip_runtime.h>

typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// NCT = 32-column tiles per wave
template <int F, int NCT>
__global__ __launch_bounds__(256) void als_xform_kernel(
    const float* __restrict__ in, const float* __restrict__ W,
    float* __restrict__ out, long long n_rows)
{
  constexpr int NQ = F / 8;               // b128 quads per lane per row
  constexpr int TC = F < 32 ? F : 32;     // live columns of a column tile
  constexpr int CG = (F / TC) / NCT;      // waves sharing one row tile
  constexpr int TPW = 4 / CG;             // row tiles per workgroup pass
  static_assert(CG * NCT * TC == F && TPW * CG == 4, "tile split");

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = lane & 31, h = lane >> 5;
  const int cbase = (wave % CG) * NCT * TC;   // first column of this wave

  // A fragment of W^T: lane (r, h) holds W[k][cbase + ct*TC + r] for
  // k = 8q + 4h + t, the same k order the data quads arrive in
  float w[NCT][NQ * 4];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = 8 * q + 4 * h + t;
        const float v = W[k * F + cbase + ct * TC + (r < TC ? r : 0)];
        w[ct][4 * q + t] = r < TC ? v : 0.f;
      }

  const long long n_tiles = (n_rows + 31) / 32;
  const long long stride = (long long)gridDim.x * TPW;
  long long tile = (long long)blockIdx.x * TPW + wave / CG;
  if (tile >= n_tiles) return;

  // rows past the end read the last row (in bounds) and are never stored
  auto row_ptr = [&](long long tl) {
    long long row = tl * 32 + r;
    row = row < n_rows ? row : n_rows - 1;
    return reinterpret_cast<const f32x4_t*>(in + row * F + 4 * h);
  };

  f32x4_t a[NQ];
  {
    const f32x4_t* p = row_ptr(tile);
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] = p[2 * q];
  }

  for (; tile < n_tiles; tile += stride) {
    f32x4_t an[NQ];
    const long long next = tile + stride;
    if (next < n_tiles) {
      const f32x4_t* p = row_ptr(next);
#pragma unroll
      for (int q = 0; q < NQ; ++q) an[q] = p[2 * q];
    } else {
#pragma unroll
      for (int q = 0; q < NQ; ++q) an[q] = a[q];
    }

    f32x16_t acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[ct][e] = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(
              w[ct][4 * q + t], a[q][t], acc[ct], 0, 0, 0);

    const long long row = tile * 32 + r;
    if (row < n_rows) {
      float* orow = out + row * F + cbase + 4 * h;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int b = 0; b < TC / 8; ++b) {
          const f32x4_t o = {acc[ct][4 * b + 0], acc[ct][4 * b + 1],
                             acc[ct][4 * b + 2], acc[ct][4 * b + 3]};
          *reinterpret_cast<f32x4_t*>(orow + ct * TC + 8 * b) = o;
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] = an[q];
  }
}

template <int F, int NCT>
static void launch_xform(const float* in, const float* W, float* out,
                         long long n_rows, int n_cu, hipStream_t stream) {
  constexpr int TC = F < 32 ? F : 32;
  constexpr int TPW = 4 / ((F / TC) / NCT);
  // persistent grid: what the device holds at once (cached per rank), or
  // fewer when there is less work
  static int wg_per_cu = 0;
  if (wg_per_cu == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &nb, als_xform_kernel<F, NCT>, 256, 0) != hipSuccess || nb < 1)
      nb = 1;
    wg_per_cu = nb;
  }
  const long long n_tiles = (n_rows + 31) / 32;
  const long long want = (n_tiles + TPW - 1) / TPW;
  const long long cap = (long long)n_cu * wg_per_cu;
  const int grid = (int)(want < cap ? want : cap);
  hipLaunchKernelGGL((als_xform_kernel<F, NCT>), dim3(grid), dim3(256), 0,
                     stream, in, W, out, n_rows);
}

extern "C" void launch_als_row_transform(
    const float* in, const float* W, float* out, long long n_rows, int f,
    int n_cu, hipStream_t stream)
{
  if (n_rows <= 0) return;
  switch (f) {
    case 16: launch_xform<16, 1>(in, W, out, n_rows, n_cu, stream); break;
    case 32: launch_xform<32, 1>(in, W, out, n_rows, n_cu, stream); break;
    case 64: launch_xform<64, 2>(in, W, out, n_rows, n_cu, stream); break;
    case 128: launch_xform<128, 1>(in, W, out, n_rows, n_cu, stream); break;
    default: break;  // caller validates
  }
}
