// Indicator top-K for MI355X (gfx950, CDNA4): serve a co-occurrence /
// cross-occurrence indicator table [Nr, n] (ids, -1 padded; scores >= 0,
// int32 counts or fp32 LLR — what cooc_topn.hip writes).
//
//   query b owns the table rows q_items[q_indptr[b] .. q_indptr[b + 1]),
//   strictly ascending. s[b][j] = sum of top_scores[i][c] over the rows i
//   of b and the columns c with top_ids[i][c] == j. Candidates are the j
//   that occur at least once and pass the filters (not a row of the query
//   itself, not in b's ban list, in b's allow list, category words hit).
//   Result: the K candidates with the largest s, score descending then id
//   ascending — the descending order of (ord(s) << 32) | (0xFFFFFFFF - j)
//   as in cooc_topn.hip and topk_cand.hip; unused slots are id -1, score 0.
//
// A sparse problem with no factor matrix: E = |rows of b| * n table
// entries per query, typically a thousand. The whole query lives in LDS
// and is grouped by sorting, not by hashing or atomics, which makes the
// float sum canonical (below).
//
// Mapping. One workgroup owns one query at a time; the grid is persistent
// over a work list sorted by E descending (ops/cooccurrence.py builds it,
// one list per instantiation). P = the power of two >= max(E, 2), computed
// per query and wave-uniform. ind_kernel<64, 512> is one wave,
// ind_kernel<256, 8192> takes the larger queries; E > 8192 never reaches
// this file. Dynamic LDS is sized by the first (largest) query of the
// launch, see ind_lds_bytes.
//
// Gather. The query's row ids go to LDS first, so that the table gathers
// all issue back to back and none starts from an id still in flight.
// Lane e takes entry e of the concatenated rows: row rows[e / n], column
// e % n, and writes the u64 (j << 32) | bits(score). Scores are >= 0, so
// for both int32 and fp32 the order of the bits is the order of the
// values (-0.0f is made +0.0f by adding 0). A -1 entry and every slot in
// [E, P) become ~0 and sort last; a real j is below 2^31, so no real key
// has the high word 0xFFFFFFFF.
//
// Sort 1, ascending bitonic in LDS: groups the entries by j and, inside a
// group, puts the addends in ascending value order.
//
// Segment sums, three passes, each ended by a barrier; in no pass does a
// thread read a slot that another thread writes in that pass.
//   A: position p writes the byte hf[p] = (p == 0 or id(p) != id(p - 1)).
//      Reads buf, writes hf.
//   B: a head walks forward to the next head flag and adds the low words
//      in that order (int32 add, or one fp32 add per addend: an ordered
//      chain), then writes (j << 32) | bits(sum) into its own slot. Reads
//      hf, its own slot and non-head slots; writes head slots only.
//   C: every position rewrites its own slot: a head whose j passes all
//      filters writes the selection key, everything else 0. The key of a
//      real candidate is never 0 (0xFFFFFFFF - j >= 2^31) and keys are
//      distinct per j.
// Canonical sum: the value of s[b][j] is a function of the multiset of
// its addends alone (they are added smallest first in fp32), whatever the
// order of the table row, of the query list or of the threads. Two calls,
// and a table whose rows are permuted column-wise, agree bit for bit.
//
// Filters run in pass C, once per distinct j: binary searches (in_sorted)
// in the query's own CSR segment, ban list and allow list, whose bounds
// are wave-uniform, and CW category-word loads.
//
// Sort 2: the same routine, descending, over the keys; the first
// min(K, #non-zero) are decoded and stored, the rest of the row is -1 / 0.
//
// Every loop is bounded by P <= PMAX or by a list length; no loop waits on
// another thread; there are no atomics. Ids are trusted: the wrapper
// range-checks the query rows, the table's ids and the lists before any
// launch (a bad id would be an out-of-bounds gather). A query that does
// not fit the launch's LDS (never, with a sorted list) is skipped.
//
// Expected resources (what the compiler gives is in NOTES.md): under 64
// VGPRs, no static LDS and no scratch in every instantiation.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_common.h"

typedef unsigned long long it_u64;

#define IT_WAVE_PMAX 512
#define IT_WG_PMAX 8192
#define IT_LDS_CU (160 * 1024)

// Dynamic LDS of a launch whose largest query has P keys and M rows:
//   it_u64  buf[P]     entries, then sums, then selection keys
//   int     rows[M']   the query's row ids, M' = M rounded up to even
//   uint8_t hf[P]      head flags
static size_t ind_lds_bytes(int P, int M)
{
  return (size_t)P * sizeof(it_u64) + (size_t)((M + 1) & ~1) * sizeof(int) +
         (size_t)P;
}

static int ind_pow2(long long E)
{
  int P = 2;
  while (P < E) P <<= 1;
  return P;
}

// order-preserving float -> u32 map and back (tm_enc of topk_mfma.hip)
__device__ __forceinline__ unsigned it_ord(float s)
{
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float it_unord(unsigned k)
{
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// Bitonic sort of buf[0..P), P a power of two >= 2, ascending or (DESC)
// descending. Called by every thread after a barrier; ends on a barrier.
template <int THREADS, bool DESC>
__device__ void it_sort(it_u64* buf, int P)
{
  const int tid = threadIdx.x;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (P >> 1); i += THREADS) {
        const int l = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int r = l | j;
        const it_u64 a = buf[l];
        const it_u64 b = buf[r];
        const bool up = ((l & k) == 0) != DESC;
        if ((a > b) == up) {
          buf[l] = b;
          buf[r] = a;
        }
      }
      __syncthreads();
    }
  }
}

template <int THREADS, int PMAX, bool FLOAT, int CW>
__global__ __launch_bounds__(THREADS)
void ind_kernel(
    const int* __restrict__ top_ids,          // Nr x n, -1 padded
    const unsigned* __restrict__ top_sc,      // Nr x n, int32 or fp32 bits
    int n,
    const long long* __restrict__ q_indptr,   // B + 1
    const int* __restrict__ q_items,          // ascending per query
    const int* __restrict__ work,             // queries, E descending
    int n_work,
    const long long* __restrict__ ban_indptr,    // B + 1, or null
    const int* __restrict__ ban_indices,
    const long long* __restrict__ allow_indptr,  // B + 1, or null
    const int* __restrict__ allow_indices,
    const int* __restrict__ item_cats,        // n_cols x CW
    const int* __restrict__ query_cats,       // B x CW
    int exclude_own, int K,
    int p_cap, int rows_cap,                  // the launch's LDS carve-up
    int* __restrict__ out_ids,                // B x K
    unsigned* __restrict__ out_sc)            // B x K
{
  extern __shared__ __align__(8) char it_lds[];
  it_u64* buf = reinterpret_cast<it_u64*>(it_lds);
  int* rows = reinterpret_cast<int*>(it_lds + (size_t)p_cap * sizeof(it_u64));
  uint8_t* hf = reinterpret_cast<uint8_t*>(rows + ((rows_cap + 1) & ~1));

  const int tid = threadIdx.x;

  for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int q = __builtin_amdgcn_readfirstlane(work[w]);
    const long long lo = q_indptr[q];
    const int m = __builtin_amdgcn_readfirstlane((int)(q_indptr[q + 1] - lo));
    const long long E64 = (long long)m * n;
    if (m < 1 || m > rows_cap || E64 > p_cap || E64 > PMAX) continue;  // uniform
    const int E = (int)E64;
    int P = 2;
    while (P < E) P <<= 1;  // <= p_cap: p_cap is a power of two >= E
    const int* own = q_items + lo;

    for (int t = tid; t < m; t += THREADS) rows[t] = own[t];
    __syncthreads();

    for (int e = tid; e < P; e += THREADS) {
      it_u64 key = ~0ull;
      if (e < E) {
        const int ri = e / n;
        const long long at = (long long)rows[ri] * n + (e - ri * n);
        const int id = top_ids[at];
        unsigned sc = top_sc[at];
        if constexpr (FLOAT) sc = __float_as_uint(__uint_as_float(sc) + 0.0f);
        if (id >= 0) key = ((it_u64)(unsigned)id << 32) | sc;
      }
      buf[e] = key;
    }
    __syncthreads();

    it_sort<THREADS, false>(buf, P);

    // pass A: head flags
    for (int p = tid; p < P; p += THREADS) {
      const unsigned j = (unsigned)(buf[p] >> 32);
      hf[p] = (p == 0 || j != (unsigned)(buf[p - 1] >> 32)) ? 1 : 0;
    }
    __syncthreads();

    // pass B: a head sums its run, smallest addend first
    for (int p = tid; p < P; p += THREADS) {
      if (hf[p] == 0) continue;
      const it_u64 v = buf[p];
      const unsigned j = (unsigned)(v >> 32);
      if (j == 0xFFFFFFFFu) continue;  // the run of empty slots
      unsigned acc = (unsigned)v;
      for (int t = p + 1; t < P && hf[t] == 0; ++t) {
        const unsigned a = (unsigned)buf[t];
        if constexpr (FLOAT)
          acc = __float_as_uint(__uint_as_float(acc) + __uint_as_float(a));
        else
          acc += a;
      }
      buf[p] = ((it_u64)j << 32) | acc;
    }
    __syncthreads();

    // pass C: filters, selection keys
    int qc[CW > 0 ? CW : 1];
    if constexpr (CW > 0) {
#pragma unroll
      for (int c = 0; c < CW; ++c)
        qc[c] = __builtin_amdgcn_readfirstlane(
            query_cats[(long long)q * CW + c]);
    }
    const int* bl = nullptr;
    int bn = 0;
    if (ban_indptr != nullptr) {
      const long long b0 = ban_indptr[q];
      bl = ban_indices + b0;
      bn = __builtin_amdgcn_readfirstlane((int)(ban_indptr[q + 1] - b0));
    }
    const int* al = nullptr;
    int an = 0;
    if (allow_indptr != nullptr) {
      const long long a0 = allow_indptr[q];
      al = allow_indices + a0;
      an = __builtin_amdgcn_readfirstlane((int)(allow_indptr[q + 1] - a0));
    }
    for (int p = tid; p < P; p += THREADS) {
      it_u64 key = 0;
      const it_u64 v = buf[p];
      const unsigned ju = (unsigned)(v >> 32);
      if (hf[p] != 0 && ju != 0xFFFFFFFFu) {
        const int j = (int)ju;
        bool pass = true;
        if (exclude_own) pass = !in_sorted(own, m, j);
        if (pass && bn > 0) pass = !in_sorted(bl, bn, j);
        if (pass && allow_indptr != nullptr) pass = in_sorted(al, an, j);
        if constexpr (CW > 0) {
          if (pass) {
            int hit = 0;
#pragma unroll
            for (int c = 0; c < CW; ++c)
              hit |= item_cats[(long long)j * CW + c] & qc[c];
            pass = hit != 0;
          }
        }
        if (pass) {
          const unsigned s = (unsigned)v;
          const unsigned o = FLOAT ? it_ord(__uint_as_float(s)) : s;
          key = ((it_u64)o << 32) | (it_u64)(0xFFFFFFFFu - ju);
        }
      }
      buf[p] = key;
    }
    __syncthreads();

    it_sort<THREADS, true>(buf, P);

    for (int t = tid; t < K; t += THREADS) {
      const it_u64 key = t < P ? buf[t] : 0;
      const long long o = (long long)q * K + t;
      const unsigned hi = (unsigned)(key >> 32);
      out_ids[o] = key != 0 ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
      out_sc[o] = key == 0 ? 0u
                  : FLOAT  ? __float_as_uint(it_unord(hi))
                           : hi;
    }
    __syncthreads();  // before the next query overwrites buf
  }
}

// Largest entry count per query of the two instantiations.
extern "C" int indicator_topk_cap(int threads)
{
  return threads == 64 ? IT_WAVE_PMAX : IT_WG_PMAX;
}

// threads: 64 (every listed query has E <= 512) or 256 (E <= 8192).
// max_items: the row count of work[0], the largest of the launch; it
// sizes the dynamic LDS. top_sc / out_sc: int32 counts, or fp32 with
// is_float. cw: category words per item, 0 / 1 / 2 / 4. Rows of out_ids /
// out_sc that are not listed are left alone.
extern "C" void launch_indicator_topk(
    const int* top_ids, const void* top_sc, int n, const long long* q_indptr,
    const int* q_items, const int* work, int n_work, int max_items,
    const long long* ban_indptr, const int* ban_indices,
    const long long* allow_indptr, const int* allow_indices,
    const int* item_cats, const int* query_cats, int cw, int is_float,
    int exclude_own, int K, int threads, int n_cu, int* out_ids, void* out_sc,
    hipStream_t stream)
{
  if (n_work <= 0 || max_items <= 0 || n <= 0) return;
  const int pmax = indicator_topk_cap(threads);
  const long long e_max = (long long)max_items * n;
  if (e_max > pmax) return;  // the caller routes such queries elsewhere
  const int p_cap = ind_pow2(e_max);
  const size_t lds = ind_lds_bytes(p_cap, max_items);
  long long per_cu = (long long)(IT_LDS_CU / lds);
  const long long most = threads == 64 ? 32 : 8;  // 32 waves per CU
  per_cu = per_cu < 1 ? 1 : per_cu > most ? most : per_cu;
  long long grid = per_cu * (n_cu > 0 ? n_cu : 1);
  if (grid > n_work) grid = n_work;
  const unsigned* sc = static_cast<const unsigned*>(top_sc);
  unsigned* osc = static_cast<unsigned*>(out_sc);
#define IT_LAUNCH(T, PM, FL, C)                                              \
  launch_dyn_lds<ind_kernel<T, PM, FL, C>>(                                  \
      dim3((unsigned)grid), dim3(T), lds, stream, top_ids, sc, n, q_indptr,  \
      q_items, work, n_work, ban_indptr, ban_indices, allow_indptr,          \
      allow_indices, item_cats, query_cats, exclude_own, K, p_cap,           \
      max_items, out_ids, osc)
#define IT_BY_CW(T, PM, FL)                    \
  do {                                         \
    if (cw == 0) IT_LAUNCH(T, PM, FL, 0);      \
    else if (cw == 1) IT_LAUNCH(T, PM, FL, 1); \
    else if (cw == 2) IT_LAUNCH(T, PM, FL, 2); \
    else IT_LAUNCH(T, PM, FL, 4);              \
  } while (0)
  if (threads == 64) {
    if (is_float) IT_BY_CW(64, IT_WAVE_PMAX, true);
    else IT_BY_CW(64, IT_WAVE_PMAX, false);
  } else {
    if (is_float) IT_BY_CW(256, IT_WG_PMAX, true);
    else IT_BY_CW(256, IT_WG_PMAX, false);
  }
#undef IT_BY_CW
#undef IT_LAUNCH
}
