// Candidate-list top-K for MI355X (gfx950, CDNA4).
//
//   query b owns the candidates cand[indptr[b] .. indptr[b + 1]), item ids
//   strictly ascending; score(b, j) = dot(Xq[b, :], Y[j, :]) in fp32.
//   Result: the K best candidates of b that pass item_mask, b's ban list
//   and the category test, score descending then id ascending: the
//   descending order of the key (ord(score) << 32) | (0xFFFFFFFF - j),
//   ord = the order-preserving float -> u32 map (tm_enc of topk_mfma.hip).
//
// The catalog kernels stream all N rows of Y per batch and filter after
// the read; this one reads the listed rows where they lie and nothing
// else, so a whitelist / re-rank request costs O(|list|), not O(N).
//
// Work split. The wrapper (ops/topk.py) cuts every list into segments
// (query, lo, hi) of absolute positions into cand, sorts them by length
// descending and routes them by length to one of two instantiations of
// the same body: 64 threads (one wave) for short segments, 256 threads
// for long ones. The grid is persistent: workgroup w takes segments w,
// w + gridDim, ... A 16-lane group takes one candidate per trip and the
// THREADS / 16 groups stride the segment. Every group holds the query
// row in registers for the whole segment (the x_u layout of
// als_loss.hip: with VEC the float4s at k = 4 sub and 64 + 4 sub,
// otherwise the floats at k = sub + 16 i), gathers the item row, runs an
// fmaf chain in that fixed k order and finishes with a 4-step cross-lane
// butterfly that all 64 lanes take. The score of a candidate therefore
// does not depend on the group, wave, segment or instantiation that
// computes it: results are bit-reproducible whatever the segmentation.
//
// Pipeline. A gather's address hangs on its id, and the filter on the
// id's mask byte and category words. So in trip t the id of trip t + 2
// and the mask byte / category words of trip t + 1 are loaded before
// trip t's row gather is issued. Those loads are unconditional and
// clamped to the segment's last candidate (a branch round a load makes
// the compiler wait for everything outstanding). A candidate that fails
// a filter issues no row load; the ban test is a binary search in the
// query's sorted ban list and runs only when the list is non-empty. The
// query's category words and ban bounds are wave-uniform and kept in
// SGPRs.
//
// Selection (K <= 64), the invariant of cooc_topn.hip: keys above a
// workgroup-shared threshold thr are appended to buf[TC_BUF] through an
// LDS counter. A step is TC_TRIPS trips and appends at most
// S = TC_TRIPS * THREADS / 16 keys, S <= TC_BUF - TC_KMAX. After a step
// that leaves fewer than S free slots a compaction runs: K rounds of
// workgroup arg-max move the K largest keys to the front, thr becomes
// buf[K - 1] and the length K <= TC_KMAX <= TC_BUF - S. So a step always
// starts with S free slots and an append index is < TC_BUF by
// construction. Ids are distinct within a query, so keys are distinct
// and a key <= thr is never among the K largest. The final selection is
// the same routine and leaves the segment's K pairs in order. No loop
// waits on another thread; the only atomics are LDS atomics.
//
// Scores mode (SCORES): the same body writes the fp32 score of every
// candidate to scores[position], -inf where it is filtered, and selects
// nothing. The wrapper uses it for K > 64.
//
// Item weights (WT): the served score is dot * item_weights[j]. The
// weight is one more piece of the candidate's metadata: loaded in the
// trip t + 1 prefetch with the mask byte and the category words, and
// multiplied in after the butterfly, before the key is formed or the
// score written. The product plus 0.0f: a zero weight must give +0.0,
// because ord(-0.0) != ord(+0.0) and the key order would otherwise put a
// zero score with a negative dot below one with a positive dot. A NaN
// product is the caller's doing and is not special-cased. WT == false is
// unchanged.
//
// Ids and segments are trusted: the wrapper range-checks the ids and
// builds the segments itself (a bad id would be an out-of-bounds gather).
//
// Expected resources (what the compiler gives is in NOTES.md):
//   64 threads:  <= 64 VGPRs, 4128 B LDS, 32 one-wave workgroups per CU
//   256 threads: <= 64 VGPRs, 4128 B LDS,  8 workgroups = 32 waves per CU
// and no scratch.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "topk_common.h"

#define TC_BUF 512    // u64 keys in the selection buffer
#define TC_KMAX 64    // largest K the selection takes
#define TC_GROUP 16   // lanes per candidate
#define TC_TRIPS 8    // trips per selection step
#define TC_RL 8       // floats of a row a lane holds (f <= 128)

typedef unsigned long long tc_u64;

struct TcSel {
  tc_u64 buf[TC_BUF];
  tc_u64 best[2];  // arg-max cell of compaction round r: best[r & 1]
  tc_u64 thr;      // keys <= thr cannot be among the K largest
  int len;         // keys in buf
};

__device__ __forceinline__ unsigned tc_ord(float s)
{
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float tc_unord(unsigned k)
{
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// The K largest of buf[0..L) to buf[0..min(K, L)), descending; len and
// (when K were found) thr updated. Every thread calls it with the same L
// after a barrier that follows the last append; ends on a barrier.
template <int THREADS>
__device__ void tc_compact(TcSel& sel, int L, int K)
{
  const int tid = threadIdx.x;
  if (tid == 0) sel.best[0] = 0;
  __syncthreads();
  int r = 0;
  for (; r < K; ++r) {
    tc_u64 m = 0;
    int mi = 0;
    for (int k = r + tid; k < L; k += THREADS) {
      const tc_u64 v = sel.buf[k];
      if (v > m) { m = v; mi = k; }
    }
    if (m != 0) atomicMax(&sel.best[r & 1], m);
    __syncthreads();
    const tc_u64 b = sel.best[r & 1];
    if (b == 0) break;  // buf[r..L) is empty: uniform
    if (m == b) {       // keys are distinct: one thread
      sel.buf[mi] = sel.buf[r];
      sel.buf[r] = b;
    }
    if (tid == 0) sel.best[(r + 1) & 1] = 0;
    __syncthreads();
  }
  if (tid == 0) {
    sel.len = r;
    if (r == K) sel.thr = sel.buf[K - 1];
  }
  __syncthreads();
}

// A lane's share of one factor row (see the header). Past f: zeros.
template <bool VEC>
__device__ __forceinline__ void tc_load_row(
    const float* __restrict__ p, int f, int sub, float (&v)[TC_RL])
{
  if constexpr (VEC) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = 64 * h + 4 * sub;
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < f) q = *reinterpret_cast<const float4*>(p + k);
      v[4 * h + 0] = q.x;
      v[4 * h + 1] = q.y;
      v[4 * h + 2] = q.z;
      v[4 * h + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < TC_RL; ++i) {
      const int k = sub + TC_GROUP * i;
      v[i] = k < f ? p[k] : 0.f;
    }
  }
}

// mask byte, category words and (WT) weight of one candidate
template <int CW, bool WT>
struct TcMeta {
  int banned;
  int c[CW > 0 ? CW : 1];
  float w[WT ? 1 : 0];
};

template <int THREADS, bool VEC, int CW, bool SCORES, bool WT>
__global__ __launch_bounds__(THREADS)
void topk_cand_kernel(
    const float* __restrict__ Xq,            // B x f
    const float* __restrict__ Y,             // N x f
    const int* __restrict__ cand,            // nnz, ascending per query
    const long long* __restrict__ segs,      // n_segs x (query, lo, hi)
    int n_segs,
    const uint8_t* __restrict__ item_mask,   // N, 1 = banned, or null
    const long long* __restrict__ ban_indptr,  // B + 1, or null
    const int* __restrict__ ban_indices,
    const int* __restrict__ item_cats,       // N x CW
    const int* __restrict__ query_cats,      // B x CW
    const float* __restrict__ item_weights,  // N (WT)
    int f, int K,
    float* __restrict__ out_val,             // n_segs x K
    int* __restrict__ out_idx,               // n_segs x K
    float* __restrict__ scores)              // SCORES: nnz
{
  constexpr int NG = THREADS / TC_GROUP;
  constexpr int S = TC_TRIPS * NG;
  static_assert(S <= TC_BUF - TC_KMAX, "step too large");

  __shared__ TcSel sel;

  const int tid = threadIdx.x;
  const int grp = tid / TC_GROUP;
  const int sub = tid % TC_GROUP;

  for (int s = blockIdx.x; s < n_segs; s += gridDim.x) {
    const int q = __builtin_amdgcn_readfirstlane((int)segs[3 * (long long)s]);
    const long long lo = segs[3 * (long long)s + 1];
    const long long hi = segs[3 * (long long)s + 2];
    if constexpr (!SCORES) {
      if (tid == 0) {
        sel.len = 0;
        sel.thr = 0;
      }
      __syncthreads();
    }

    if (lo < hi) {  // uniform
      float x[TC_RL];
      tc_load_row<VEC>(Xq + (long long)q * f, f, sub, x);

      int qc[CW > 0 ? CW : 1];
      if constexpr (CW > 0) {
#pragma unroll
        for (int w = 0; w < CW; ++w)
          qc[w] = __builtin_amdgcn_readfirstlane(
              query_cats[(long long)q * CW + w]);
      }
      const int* bl = nullptr;
      int bn = 0;
      if (ban_indptr != nullptr) {
        const long long b0 = ban_indptr[q];
        bl = ban_indices + b0;
        bn = __builtin_amdgcn_readfirstlane((int)(ban_indptr[q + 1] - b0));
      }

      const long long last = hi - 1;
      auto fetch_id = [&](long long p) { return cand[p < hi ? p : last]; };
      auto fetch_meta = [&](int j, TcMeta<CW, WT>& m) {
        m.banned = item_mask != nullptr ? (int)item_mask[j] : 0;
        if constexpr (WT) m.w[0] = item_weights[j];
        if constexpr (CW > 0) {
#pragma unroll
          for (int w = 0; w < CW; ++w)
            m.c[w] = item_cats[(long long)j * CW + w];
        }
      };

      long long p = lo + grp;
      int j0 = fetch_id(p);
      int j1 = fetch_id(p + NG);
      TcMeta<CW, WT> m0, m1;
      fetch_meta(j0, m0);

      for (long long base = lo; base < hi;) {
        tc_u64 thr = 0;
        if constexpr (!SCORES) thr = sel.thr;
        for (int t = 0; t < TC_TRIPS && base < hi;
             ++t, base += NG, p += NG) {
          // ids two trips ahead, mask byte and category words one trip
          // ahead: both go out before this trip's gather
          const int j2 = fetch_id(p + 2 * NG);
          fetch_meta(j1, m1);

          const bool live = p < hi;
          bool pass = live && m0.banned == 0;
          if constexpr (CW > 0) {
            int hit = 0;
#pragma unroll
            for (int w = 0; w < CW; ++w) hit |= m0.c[w] & qc[w];
            pass = pass && hit != 0;
          }
          if (bn > 0 && pass) pass = !in_sorted(bl, bn, j0);

          float y[TC_RL];
          if (pass) {
            tc_load_row<VEC>(Y + (long long)j0 * f, f, sub, y);
          } else {
#pragma unroll
            for (int i = 0; i < TC_RL; ++i) y[i] = 0.f;
          }
          float sc = 0.f;
#pragma unroll
          for (int i = 0; i < TC_RL; ++i) sc = fmaf(x[i], y[i], sc);
          // every lane of the wave takes part, candidate or not
#pragma unroll
          for (int o = TC_GROUP / 2; o > 0; o >>= 1) sc += __shfl_xor(sc, o);
          if constexpr (WT) sc = sc * m0.w[0] + 0.0f;

          if (sub == 0 && live) {
            if constexpr (SCORES) {
              scores[p] = pass ? sc : -INFINITY;
            } else if (pass) {
              const tc_u64 key = ((tc_u64)tc_ord(sc) << 32) |
                                 (tc_u64)(0xFFFFFFFFu - (unsigned)j0);
              if (key > thr) {
                const int k = atomicAdd(&sel.len, 1);  // < TC_BUF, see above
                sel.buf[k] = key;
              }
            }
          }
          j0 = j1;
          j1 = j2;
          m0 = m1;
        }
        if constexpr (!SCORES) {
          __syncthreads();
          const int L = sel.len;
          __syncthreads();  // everyone holds L before anyone appends again
          if (base >= hi || L > TC_BUF - S) tc_compact<THREADS>(sel, L, K);
        }
      }
    }

    if constexpr (!SCORES) {
      // buf[0..len) holds the segment's best, in order
      const int L = sel.len;
      for (int t = tid; t < K; t += THREADS) {
        const tc_u64 key = t < L ? sel.buf[t] : 0;
        const long long o = (long long)s * K + t;
        out_val[o] = t < L ? tc_unord((unsigned)(key >> 32)) : -INFINITY;
        out_idx[o] = t < L ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
      }
      __syncthreads();  // before the next segment resets len
    }
  }
}

// threads: 64 or 256. K = 0 selects scores mode (scores != null, always
// the 256-thread body); otherwise 1 <= K <= TC_KMAX. cw: category words
// per item, 0 / 1 / 2 / 4. item_weights: nullptr = unweighted. The caller
// sizes the grid.
extern "C" void launch_topk_cand(
    const float* Xq, const float* Y, const int* cand, const long long* segs,
    int n_segs, const uint8_t* item_mask, const long long* ban_indptr,
    const int* ban_indices, const int* item_cats, const int* query_cats,
    const float* item_weights, int cw, int f, int K, int threads,
    float* out_val, int* out_idx, float* scores, int grid,
    hipStream_t stream)
{
  if (n_segs <= 0 || grid <= 0) return;
  const bool vec = f % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(Xq) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(Y) % 16 == 0;
#define TC_LAUNCH_WT(T, V, C, SC, WT)                                     \
  hipLaunchKernelGGL((topk_cand_kernel<T, V, C, SC, WT>),                 \
                     dim3((unsigned)grid), dim3(T), 0, stream, Xq, Y,     \
                     cand, segs, n_segs, item_mask, ban_indptr,           \
                     ban_indices, item_cats, query_cats, item_weights, f, \
                     K, out_val, out_idx, scores)
#define TC_LAUNCH(T, V, C, SC)                                 \
  do {                                                         \
    if (item_weights != nullptr) TC_LAUNCH_WT(T, V, C, SC, true); \
    else TC_LAUNCH_WT(T, V, C, SC, false);                     \
  } while (0)
#define TC_BY_CW(T, V, SC)                 \
  do {                                     \
    if (cw == 0) TC_LAUNCH(T, V, 0, SC);   \
    else if (cw == 1) TC_LAUNCH(T, V, 1, SC); \
    else if (cw == 2) TC_LAUNCH(T, V, 2, SC); \
    else TC_LAUNCH(T, V, 4, SC);           \
  } while (0)
  if (K == 0) {
    if (vec) TC_BY_CW(256, true, true);
    else TC_BY_CW(256, false, true);
  } else if (threads == 64) {
    if (vec) TC_BY_CW(64, true, false);
    else TC_BY_CW(64, false, false);
  } else {
    if (vec) TC_BY_CW(256, true, false);
    else TC_BY_CW(256, false, false);
  }
#undef TC_BY_CW
#undef TC_LAUNCH
#undef TC_LAUNCH_WT
}
