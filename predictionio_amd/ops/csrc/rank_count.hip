// Held-out rank counts for MI355X (gfx950, CDNA4).
//
//   s[b][j] = x_b . y_j, exact fp32. For every held-out pair (b, t) the
//   wrapper (ops/ranking.py) wants gt = #{j candidate : s[b][j] > s[b][t]}
//   and ge = #{j candidate : s[b][j] >= s[b][t]}; candidates are all items
//   but the user's seen list. Nothing is ranked or kept: the kernels count.
//
// Unit of work: a slot = one user with at most RK_TMAX targets (a user with
// more takes several slots; slot_user names the X row, rows are not copied).
// The slot arrays are padded to a multiple of 128 by the wrapper: a padding
// slot has user 0 and no targets.
//
// Scoring, shared by both kernels (rk_tile_scores): one 32 x 32 tile of
// v_mfma_f32_32x32x2_f32, items as the A operand and slots as the B operand,
// so that the C/D layout (col = lane & 31, row = (reg & 3) + 8 (reg >> 2)
// + 4 (lane >> 5)) gives lane (c, h) sixteen item rows of ONE slot c. The
// k sum runs in the order the LDS quads arrive in, step (q, t) taking
// k = 8q + t from the h = 0 lanes and k = 8q + 4 + t from the h = 1 lanes;
// the slot's X fragment is held in that order in F/2 VGPRs. A score is a
// function of (x_b, y_j) alone: the same instruction sequence on the same
// operands wherever the item row sits in a tile, in either kernel.
//
// rank_list_kernel runs first. A wave gathers, in round r, the r-th list
// entry of each of its 32 slots into a private 32-row LDS tile, scores the
// whole tile and keeps the diagonal (row c, column c): 31/32 of the tile is
// thrown away so that the value has the bits the stream will produce.
// Rounds 0 .. TMAX-1 are the targets (tscore), the following rounds walk
// the slot's seen list and count corr_gt / corr_ge against the targets.
//
// rank_stream_kernel is the hot path: grid = slot groups (128 slots, four
// waves of 32) x item slices. The four waves share a 64-item fp32 chunk in
// LDS (rows padded to F + 4 floats: the b128 read of lane (r, h) at
// r * (F + 4) + 8q + 4h is conflict free), double buffered and register
// staged: chunk c + 1's global loads are issued before chunk c's MFMAs and
// written to the other buffer after them, one barrier per chunk. After a
// tile's MFMAs every accumulator is compared with the lane's TMAX target
// scores: gt[m] += acc > t[m], ge[m] += acc >= t[m]. Rows >= N are NaN in
// LDS and a missing target is NaN, so both compares are false. Seen items
// and the target itself are counted here and taken out by the wrapper:
//   gt = sum_slices partial_gt - corr_gt,
//   eq = (sum_slices partial_ge - corr_ge) - gt - 1.
// Lanes l and l ^ 32 (the two row halves of a slot) add up at the end; lane
// h = 0 stores the four gt, lane h = 1 the four ge as one b128 each into
// partial[slice][slot][h][m]. Plain vector stores, no atomics, and every
// slot of every slice is written (an empty slice writes zeros).
//
// No fp32 VALU arithmetic touches a score: the chain is on the matrix pipe
// and the epilogue is compares and integer adds.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_common.h"

typedef __attribute__((ext_vector_type(4))) float rk_f32x4;
typedef __attribute__((ext_vector_type(16))) float rk_f32x16;
typedef __attribute__((ext_vector_type(4))) int rk_i32x4;

#define RK_TMAX 4     // targets per slot
#define RK_CHUNK 64   // item rows per LDS buffer (two 32-row tiles)
#define RK_GROUP 128  // slots per workgroup

// Scores of the 32 item rows at `tile` (row stride F + 4 floats) against
// the wave's 32 slots. x[4q + t] = X[slot lane & 31][8q + 4h + t].
template <int F>
__device__ __forceinline__ rk_f32x16 rk_tile_scores(
    const float* tile, const float (&x)[F / 2], int r, int h)
{
  const rk_f32x4* row =
      reinterpret_cast<const rk_f32x4*>(tile + r * (F + 4) + 4 * h);
  rk_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
  for (int q = 0; q < F / 8; ++q) {
    const rk_f32x4 a = row[2 * q];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], x[4 * q + t], acc,
                                                 0, 0, 0);
  }
  return acc;
}

template <int F>
__device__ __forceinline__ void rk_load_x(const float* __restrict__ X,
                                          int user, int h, float (&x)[F / 2])
{
  const rk_f32x4* p =
      reinterpret_cast<const rk_f32x4*>(X + (long long)user * F + 4 * h);
#pragma unroll
  for (int q = 0; q < F / 8; ++q) {
    const rk_f32x4 v = p[2 * q];
#pragma unroll
    for (int t = 0; t < 4; ++t) x[4 * q + t] = v[t];
  }
}

__device__ __forceinline__ rk_f32x4 rk_nan4()
{
  const float n = __uint_as_float(0x7FC00000u);
  return rk_f32x4{n, n, n, n};
}

// Pins the four counters in their VGPRs at this point (no instruction).
// Without it the sixteen adds per counter of a tile are reassociated into
// a tree: every compare mask is then live at once, far more SGPR pairs
// than there are. Pinned, each add stays a v_cmp + v_addc_co pair.
__device__ __forceinline__ void rk_pin(int (&c)[RK_TMAX])
{
  asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
}

template <int F, bool TIES>
__global__ __launch_bounds__(256) void rank_stream_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, long long N,
    const int* __restrict__ slot_user,  // S
    const float* __restrict__ tscore,   // S x TMAX
    int n_slots,                        // S, a multiple of RK_GROUP
    int chunks_per_slice,
    int* __restrict__ partial)          // slices x S x 2 x TMAX
{
  constexpr int FP = F + 4;
  constexpr int QR = F / 4;                  // b128 quads per row
  constexpr int NV = RK_CHUNK * QR / 256;    // quads per thread per chunk
  static_assert(NV * 256 == RK_CHUNK * QR, "chunk split");
  extern __shared__ __align__(16) float rk_lds[];  // 2 x RK_CHUNK x FP

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int slot = blockIdx.x * RK_GROUP + wave * 32 + r;

  float x[F / 2];
  rk_load_x<F>(X, slot_user[slot], h, x);
  float ts[RK_TMAX];
  {
    const rk_f32x4 v =
        *reinterpret_cast<const rk_f32x4*>(tscore + (long long)slot * RK_TMAX);
#pragma unroll
    for (int m = 0; m < RK_TMAX; ++m) ts[m] = v[m];
  }
  int gt[RK_TMAX], ge[RK_TMAX];
#pragma unroll
  for (int m = 0; m < RK_TMAX; ++m) gt[m] = ge[m] = 0;

  const long long n_chunks = (N + RK_CHUNK - 1) / RK_CHUNK;
  const long long c0 = (long long)blockIdx.y * chunks_per_slice;
  const long long c1 =
      c0 + chunks_per_slice < n_chunks ? c0 + chunks_per_slice : n_chunks;

  // thread's quads of a chunk: index i = tid + 256 s, row i / QR, quad i % QR
  rk_f32x4 st[NV];
  auto load_chunk = [&](long long c) {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const int i = tid + 256 * s;
      const long long row = c * RK_CHUNK + i / QR;
      st[s] = row < N ? *reinterpret_cast<const rk_f32x4*>(
                            Y + row * F + 4 * (i % QR))
                      : rk_nan4();
    }
  };
  auto store_chunk = [&](float* buf) {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const int i = tid + 256 * s;
      *reinterpret_cast<rk_f32x4*>(buf + (i / QR) * FP + 4 * (i % QR)) = st[s];
    }
  };

  if (c0 < c1) {
    load_chunk(c0);
    store_chunk(rk_lds);
  }
  __syncthreads();

  for (long long c = c0; c < c1; ++c) {
    const float* cur = rk_lds + ((c - c0) & 1) * (RK_CHUNK * FP);
    float* nxt = rk_lds + (((c - c0) & 1) ^ 1) * (RK_CHUNK * FP);
    const bool more = c + 1 < c1;  // uniform
    if (more) load_chunk(c + 1);
#pragma unroll
    for (int tl = 0; tl < RK_CHUNK / 32; ++tl) {
      const rk_f32x16 acc = rk_tile_scores<F>(cur + tl * 32 * FP, x, r, h);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
#pragma unroll
        for (int m = 0; m < RK_TMAX; ++m) {
          gt[m] += acc[e] > ts[m] ? 1 : 0;
          if constexpr (TIES) ge[m] += acc[e] >= ts[m] ? 1 : 0;
        }
        rk_pin(gt);
        if constexpr (TIES) rk_pin(ge);
      }
    }
    // nxt was last read in the iteration before this one, which every
    // wave left through the barrier below
    if (more) store_chunk(nxt);
    __syncthreads();
  }

  rk_i32x4 o;
#pragma unroll
  for (int m = 0; m < RK_TMAX; ++m) {
    const int g = gt[m] + __shfl_xor(gt[m], 32);
    const int e = TIES ? ge[m] + __shfl_xor(ge[m], 32) : 0;
    o[m] = h == 0 ? g : e;
  }
  if (h == 0 || TIES)
    *reinterpret_cast<rk_i32x4*>(
        partial +
        (((long long)blockIdx.y * n_slots + slot) * 2 + h) * RK_TMAX) = o;
}

template <int F>
__global__ __launch_bounds__(256) void rank_list_kernel(
    const float* __restrict__ X, const float* __restrict__ Y,
    const int* __restrict__ slot_user,          // S
    const int* __restrict__ slot_tgt,           // S x TMAX, -1 = none
    const long long* __restrict__ seen_indptr,  // users + 1, or null
    const int* __restrict__ seen_indices,
    float* __restrict__ tscore,                 // S x TMAX
    int* __restrict__ corr)                     // S x 2 x TMAX
{
  constexpr int FP = F + 4;
  constexpr int QR = F / 4;
  constexpr int NV = 32 * QR / 64;  // quads per lane per round
  extern __shared__ __align__(16) float rk_lds[];  // 4 x 32 x FP, 4 ints
  float* tiles = rk_lds;
  int* wave_rounds = reinterpret_cast<int*>(rk_lds + 4 * 32 * FP);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int slot = blockIdx.x * RK_GROUP + wave * 32 + r;
  float* tile = tiles + wave * 32 * FP;

  const int user = slot_user[slot];
  float x[F / 2];
  rk_load_x<F>(X, user, h, x);
  int tg[RK_TMAX];
  {
    const rk_i32x4 v =
        *reinterpret_cast<const rk_i32x4*>(slot_tgt + (long long)slot * RK_TMAX);
#pragma unroll
    for (int m = 0; m < RK_TMAX; ++m) tg[m] = v[m];
  }
  long long s_lo = 0;
  int s_len = 0;
  if (seen_indptr != nullptr && tg[0] >= 0) {  // a slot without targets
    s_lo = seen_indptr[user];                  // has nothing to correct
    s_len = (int)(seen_indptr[user + 1] - s_lo);
  }
  // seen rounds of the workgroup: the longest list of its 128 slots
  int rounds = s_len;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const int o = __shfl_xor(rounds, d);
    rounds = o > rounds ? o : rounds;
  }
  if (lane == 0) wave_rounds[wave] = rounds;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w)
    rounds = wave_rounds[w] > rounds ? wave_rounds[w] : rounds;
  rounds = __builtin_amdgcn_readfirstlane(rounds);

  // Score of item `id` (this lane's slot's entry of the round; < 0 = none,
  // NaN) against the lane's slot: gather the wave's 32 rows, score the
  // tile, keep the diagonal. Called by all 256 threads.
  auto diag_score = [&](int id) -> float {
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      const int i = lane + 64 * s;
      const int row = i / QR;
      const int rid = __shfl(id, row);
      const rk_f32x4 v = rid >= 0 ? *reinterpret_cast<const rk_f32x4*>(
                                        Y + (long long)rid * F + 4 * (i % QR))
                                  : rk_nan4();
      *reinterpret_cast<rk_f32x4*>(tile + row * FP + 4 * (i % QR)) = v;
    }
    __syncthreads();
    const rk_f32x16 acc = rk_tile_scores<F>(tile, x, r, h);
    __syncthreads();  // before the next round's gather
    // row r of column r: register (r & 3) + 4 (r >> 3) of the lane whose
    // h is bit 2 of r. Unrolled select, no runtime register index.
    const int want = (r & 3) + 4 * (r >> 3);
    float v = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) v = e == want ? acc[e] : v;
    const float o = __shfl_xor(v, 32);
    return h == ((r >> 2) & 1) ? v : o;
  };

  float ts[RK_TMAX];
#pragma unroll
  for (int m = 0; m < RK_TMAX; ++m) ts[m] = diag_score(tg[m]);
  if (h == 0)
    *reinterpret_cast<rk_f32x4*>(tscore + (long long)slot * RK_TMAX) =
        rk_f32x4{ts[0], ts[1], ts[2], ts[3]};

  int cg[RK_TMAX], ce[RK_TMAX];
#pragma unroll
  for (int m = 0; m < RK_TMAX; ++m) cg[m] = ce[m] = 0;
  for (int i = 0; i < rounds; ++i) {
    const int id = i < s_len ? seen_indices[s_lo + i] : -1;
    const float v = diag_score(id);
#pragma unroll
    for (int m = 0; m < RK_TMAX; ++m) {
      cg[m] += v > ts[m] ? 1 : 0;
      ce[m] += v >= ts[m] ? 1 : 0;
    }
  }
  rk_i32x4 o;
#pragma unroll
  for (int m = 0; m < RK_TMAX; ++m) o[m] = h == 0 ? cg[m] : ce[m];
  *reinterpret_cast<rk_i32x4*>(corr + ((long long)slot * 2 + h) * RK_TMAX) = o;
}

extern "C" int rank_count_tmax() { return RK_TMAX; }

extern "C" int rank_count_group() { return RK_GROUP; }

// Dynamic LDS of rank_stream_kernel<f>: two chunk buffers.
extern "C" int rank_stream_lds_bytes(int f)
{
  return 2 * RK_CHUNK * (f + 4) * (int)sizeof(float);
}

// n_slots: a multiple of RK_GROUP. f: 16 / 32 / 64 / 128 (caller validates).
extern "C" void launch_rank_list(
    const float* X, const float* Y, const int* slot_user, const int* slot_tgt,
    const long long* seen_indptr, const int* seen_indices, float* tscore,
    int* corr, int n_slots, int f, hipStream_t stream)
{
  if (n_slots <= 0) return;
  const dim3 grid((unsigned)(n_slots / RK_GROUP));
  // a 32-row tile per wave and the four waves' round counts
  const size_t lds = (size_t)(4 * 32 * (f + 4) + 4) * sizeof(float);
#define RK_LIST(FF)                                                        \
  launch_dyn_lds<rank_list_kernel<FF>>(grid, dim3(256), lds, stream, X, Y, \
                                       slot_user, slot_tgt, seen_indptr,   \
                                       seen_indices, tscore, corr)
  switch (f) {
    case 16: RK_LIST(16); break;
    case 32: RK_LIST(32); break;
    case 64: RK_LIST(64); break;
    case 128: RK_LIST(128); break;
    default: break;
  }
#undef RK_LIST
}

// Slice s takes the 64-item chunks [s * cps, (s + 1) * cps), cps =
// ceil(chunks / n_slices); n_slices in [1, 65535].
extern "C" void launch_rank_stream(
    const float* X, const float* Y, long long N, const int* slot_user,
    const float* tscore, int n_slots, int n_slices, int ties, int* partial,
    int f, hipStream_t stream)
{
  if (n_slots <= 0 || n_slices <= 0 || N <= 0) return;
  const long long n_chunks = (N + RK_CHUNK - 1) / RK_CHUNK;
  const int cps = (int)((n_chunks + n_slices - 1) / n_slices);
  const dim3 grid((unsigned)(n_slots / RK_GROUP), (unsigned)n_slices);
  const size_t lds = (size_t)rank_stream_lds_bytes(f);
#define RK_STREAM(FF)                                                        \
  do {                                                                       \
    if (ties)                                                                \
      launch_dyn_lds<rank_stream_kernel<FF, true>>(                          \
          grid, dim3(256), lds, stream, X, Y, N, slot_user, tscore, n_slots, \
          cps, partial);                                                     \
    else                                                                     \
      launch_dyn_lds<rank_stream_kernel<FF, false>>(                         \
          grid, dim3(256), lds, stream, X, Y, N, slot_user, tscore, n_slots, \
          cps, partial);                                                     \
  } while (0)
  switch (f) {
    case 16: RK_STREAM(16); break;
    case 32: RK_STREAM(32); break;
    case 64: RK_STREAM(64); break;
    case 128: RK_STREAM(128); break;
    default: break;
  }
#undef RK_STREAM
}
