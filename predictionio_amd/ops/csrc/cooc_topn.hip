// Co-occurrence top-N for MI355X (gfx950, CDNA4).
//
//   c[i][j] = |users(i) ∩ users(j)|,  i != j
//   row i of the result = the n items j with the largest c[i][j] > 0,
//   count descending then id ascending: the descending order of the key
//   (count << 32) | (0xFFFFFFFF - j).
//
// The sparse product A^T A that holds every c[i][j] has one entry per
// (user, item, item) triple before it is coalesced; this file never
// forms it. One workgroup owns one item row at a time and does
//
//   count    for every user u of the row (item-major CSR) and every item
//            j != i of u (user-major CSR): counter[j] += 1
//   harvest  visit each distinct j once with its final count
//   select   keep the n largest keys, write row i
//
// and the only thing that leaves the chip is the row's n pairs.
//
// Where the counters live is decided per row before the launch from
// ub_i = min(N - 1, sum_{u in users(i)} d_u - deg_i), a bound on the
// row's distinct neighbours (ops/cooccurrence.py: cooccurrence_plan):
//
//   T = 1024,  64 threads   ub <= 768    open-addressing table in LDS
//   T = 8192, 256 threads   ub <= 6144   the same, 64 KB
//   T = 0,    256 threads   any ub       one [N] int32 counter row of a
//                                        zero-initialised global pool per
//                                        persistent workgroup
//   T = -1,   256 threads   any ub,      the same dense counters in LDS
//                           N <= 28672   (112 KB), one workgroup per CU
//
// ub <= 3/4 T bounds the distinct keys, so an insert always finds a
// slot; the probe loop still runs at most T times and then gives up, and
// no loop in this file waits for another thread.
//
// Lane mapping: a 16-lane group takes one user at a time (groups stride
// the row's user list), its lanes stride that user's items. View lists
// are short (tens of items), so a whole wave per user would idle most
// lanes; 16 keeps a 20-item user at 62 % lane use and a 64-byte request
// per group. The group's NEXT user id is loaded before the current
// user's row pointers and items are, so the dependent chain
// id -> indptr -> items never starts from a cold id.
//
// Dense harvest is the count walk again with c = atomicExch(&cnt[j], 0):
// exactly one visitor of each distinct j sees c != 0, and that visit
// both yields (j, c) and puts the counter row back to all zero for the
// workgroup's next row. Nothing crosses workgroups: one barrier between
// count and harvest, no flags.
//
// Selection (both tiers): keys above a workgroup-shared threshold thr
// are appended to buf[CO_SELECT_BUF] through an LDS counter. Harvest
// runs in steps that append at most S = K * THREADS keys (K slots or K
// walk iterations per thread), S <= CO_SELECT_BUF - 64. After a step
// that leaves fewer than S free slots a compaction runs: n rounds of
// workgroup arg-max move the n largest keys to the front, thr becomes
// buf[n - 1] and the length n <= 64 <= CO_SELECT_BUF - S. So a step
// always starts with S free slots and an append index is always
// < CO_SELECT_BUF. Keys are distinct (distinct j), so a key <= thr is
// never among the n largest and dropping it loses nothing. The final
// selection is the same routine.
//
// Ids are trusted: the Python wrapper range-checks both CSRs before the
// launch (a bad id would be an out-of-bounds atomic).

#include <hip/hip_runtime.h>
#include <stdint.h>

#define CO_SELECT_BUF 1024  // u64 keys in the selection buffer
#define CO_NMAX 64          // largest n
#define CO_GROUP 16         // lanes per user
#define CO_DENSE_LDS 28672  // largest N whose dense counters fit in LDS

typedef unsigned long long co_u64;

struct CoSel {
  co_u64 buf[CO_SELECT_BUF];
  co_u64 best[2];  // arg-max cell of compaction round r: best[r & 1]
  co_u64 thr;      // keys <= thr cannot be among the n largest
  int len;         // keys in buf
};

__device__ __forceinline__ co_u64 co_pack(int c, int j)
{
  return ((co_u64)(unsigned)c << 32) | (co_u64)(0xFFFFFFFFu - (unsigned)j);
}

__device__ __forceinline__ void co_append(CoSel& sel, co_u64 key, co_u64 thr)
{
  if (key > thr) {
    const int k = atomicAdd(&sel.len, 1);  // < CO_SELECT_BUF, see above
    sel.buf[k] = key;
  }
}

// The n largest of buf[0..L) to buf[0..min(n, L)), descending; len and
// (when n were found) thr updated. Every thread calls it with the same L
// after a barrier that follows the last append; ends on a barrier.
template <int THREADS>
__device__ void co_compact(CoSel& sel, int L, int n)
{
  const int tid = threadIdx.x;
  if (tid == 0) sel.best[0] = 0;
  __syncthreads();
  int r = 0;
  for (; r < n; ++r) {
    co_u64 m = 0;
    int mi = 0;
    for (int k = r + tid; k < L; k += THREADS) {
      const co_u64 v = sel.buf[k];
      if (v > m) { m = v; mi = k; }
    }
    if (m != 0) atomicMax(&sel.best[r & 1], m);
    __syncthreads();
    const co_u64 b = sel.best[r & 1];
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
    if (r == n) sel.thr = sel.buf[n - 1];
  }
  __syncthreads();
}

// End of a harvest step that appended at most S keys.
template <int THREADS>
__device__ __forceinline__ void co_step_end(CoSel& sel, int n, int S,
                                            bool final)
{
  __syncthreads();
  const int L = sel.len;
  __syncthreads();  // everyone holds L before anyone appends again
  if (final || L > CO_SELECT_BUF - S) co_compact<THREADS>(sel, L, n);
}

// A 16-lane group's resumable walk over (user of the row, item of the
// user): users ustart + grp, + NG, ...; `un` is the id of the next user
// to open (-1 = none), [q, e) what is left of the open user's items.
struct CoWalk {
  long long p, uend, q, e;
  int un;
};

template <int NG>
__device__ __forceinline__ void co_walk_init(
    CoWalk& w, const int* __restrict__ i_users, long long ustart,
    long long uend, int grp)
{
  w.p = ustart + grp;
  w.uend = uend;
  w.un = w.p < uend ? i_users[w.p] : -1;
  w.q = w.e = 0;
}

// Up to `quota` group iterations, each calling f(j) for at most one item
// j != self per lane. Returns true when the group's share is finished.
template <int NG, class F>
__device__ __forceinline__ bool co_walk(
    CoWalk& w, const long long* __restrict__ u_indptr,
    const int* __restrict__ u_items, const int* __restrict__ i_users,
    int self, int sub, int quota, F f)
{
  while (quota > 0) {
    if (w.q >= w.e) {
      if (w.un < 0) return true;
      const int u = w.un;
      // the next user's id goes out ahead of this user's dependent loads
      w.p += NG;
      w.un = w.p < w.uend ? i_users[w.p] : -1;
      w.q = u_indptr[u];
      w.e = u_indptr[u + 1];
      continue;
    }
    const long long qq = w.q + sub;
    if (qq < w.e) {
      const int j = u_items[qq];
      if (j != self) f(j);
    }
    w.q += CO_GROUP;
    --quota;
  }
  return w.q >= w.e && w.un < 0;
}

template <int THREADS, int T>
__global__ __launch_bounds__(THREADS)
void cooc_kernel(
    const long long* __restrict__ u_indptr,  // U + 1
    const int* __restrict__ u_items,         // nnz, user-major
    const long long* __restrict__ i_indptr,  // N + 1
    const int* __restrict__ i_users,         // nnz, item-major
    const int* __restrict__ rows,            // n_rows item ids, heavy first
    int n_rows, int n,
    int* __restrict__ pool,                  // T == 0: [gridDim.x, N] zeros
    long long n_items,
    int* __restrict__ top_ids,               // [N, n]
    int* __restrict__ top_cnt)               // [N, n]
{
  constexpr int NG = THREADS / CO_GROUP;
  constexpr int K = (CO_SELECT_BUF - CO_NMAX) / THREADS;
  constexpr int S = K * THREADS;
  constexpr int TS = T > 0 ? T : 1;
  constexpr int DS = T < 0 ? CO_DENSE_LDS : 1;
  static_assert(K >= 1 && S <= CO_SELECT_BUF - CO_NMAX, "step too large");
  static_assert(T <= 0 || (T & (T - 1)) == 0, "table size: a power of two");

  __shared__ CoSel sel;
  __shared__ int keys[TS];
  __shared__ int cnts[TS];
  __shared__ int dcnt[DS];  // T < 0: the dense counters, n_items <= DS

  const int tid = threadIdx.x;
  const int grp = tid / CO_GROUP;
  const int sub = tid % CO_GROUP;

  if constexpr (T > 0) {
    for (int s = tid; s < T; s += THREADS) {
      keys[s] = -1;
      cnts[s] = 0;
    }
  }
  if constexpr (T < 0) {
    for (int s = tid; s < (int)n_items; s += THREADS) dcnt[s] = 0;
  }
  int* const gcnt =
      T == 0 ? pool + (long long)blockIdx.x * n_items : nullptr;
  __syncthreads();

  for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int self = rows[r];
    const long long ustart = i_indptr[self];
    const long long uend = i_indptr[self + 1];
    if (tid == 0) {
      sel.len = 0;
      sel.thr = 0;
    }

    // ---- count
    CoWalk w;
    co_walk_init<NG>(w, i_users, ustart, uend, grp);
    co_walk<NG>(w, u_indptr, u_items, i_users, self, sub, 0x7fffffff,
                [&](int j) {
      if constexpr (T > 0) {
        unsigned h = ((unsigned)j * 0x9E3779B1u) >> (32 - __builtin_ctz(TS));
        for (int p = 0; p < T; ++p) {
          const int prev = atomicCAS(&keys[h], -1, j);
          if (prev == -1 || prev == j) {
            atomicAdd(&cnts[h], 1);
            break;
          }
          h = (h + 1) & (T - 1);
        }
      } else if constexpr (T == 0) {
        atomicAdd(&gcnt[j], 1);
      } else {
        atomicAdd(&dcnt[j], 1);
      }
    });
    // dense: the adds have been performed before any exchange is issued
    if constexpr (T == 0) __threadfence();
    __syncthreads();

    // ---- harvest and select
    if constexpr (T > 0) {
      for (int base = 0; base < T; base += S) {
        const co_u64 thr = sel.thr;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int s = base + k * THREADS + tid;
          if (s < T) {
            const int j = keys[s];
            if (j >= 0) {
              const int c = cnts[s];
              keys[s] = -1;  // the table is empty again for the next row
              cnts[s] = 0;
              co_append(sel, co_pack(c, j), thr);
            }
          }
        }
        co_step_end<THREADS>(sel, n, S, base + S >= T);
      }
    } else {
      co_walk_init<NG>(w, i_users, ustart, uend, grp);
      for (;;) {
        const co_u64 thr = sel.thr;
        const bool done = co_walk<NG>(
            w, u_indptr, u_items, i_users, self, sub, K, [&](int j) {
              int c;
              if constexpr (T == 0) c = atomicExch(&gcnt[j], 0);
              else c = atomicExch(&dcnt[j], 0);
              if (c != 0) co_append(sel, co_pack(c, j), thr);
            });
        const int pending = __syncthreads_or(!done);
        co_step_end<THREADS>(sel, n, S, !pending);
        if (!pending) break;
      }
    }

    // ---- buf[0..len) holds the row, in order
    const int L = sel.len;
    for (int t = tid; t < n; t += THREADS) {
      const co_u64 key = t < L ? sel.buf[t] : 0;
      const long long o = (long long)self * n + t;
      top_ids[o] = t < L ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
      top_cnt[o] = (int)(key >> 32);
    }
    __syncthreads();  // before the next row resets len
  }
}

// tier 0: <64, 1024>, tier 1: <256, 8192>, tier 2: dense over `pool`
// (grid = its counter rows), tier 3: dense in LDS (n_items <=
// CO_DENSE_LDS). The caller sizes the grid.
extern "C" void launch_cooc_topn(
    const long long* u_indptr, const int* u_items, const long long* i_indptr,
    const int* i_users, const int* rows, int n_rows, int n, int tier,
    int* pool, long long n_items, int* top_ids, int* top_cnt, int grid,
    hipStream_t stream)
{
  if (n_rows <= 0 || grid <= 0) return;
  if (tier == 0)
    hipLaunchKernelGGL((cooc_kernel<64, 1024>), dim3((unsigned)grid),
                       dim3(64), 0, stream, u_indptr, u_items, i_indptr,
                       i_users, rows, n_rows, n, pool, n_items, top_ids,
                       top_cnt);
  else if (tier == 1)
    hipLaunchKernelGGL((cooc_kernel<256, 8192>), dim3((unsigned)grid),
                       dim3(256), 0, stream, u_indptr, u_items, i_indptr,
                       i_users, rows, n_rows, n, pool, n_items, top_ids,
                       top_cnt);
  else if (tier == 2)
    hipLaunchKernelGGL((cooc_kernel<256, 0>), dim3((unsigned)grid),
                       dim3(256), 0, stream, u_indptr, u_items, i_indptr,
                       i_users, rows, n_rows, n, pool, n_items, top_ids,
                       top_cnt);
  else if (n_items <= CO_DENSE_LDS)
    hipLaunchKernelGGL((cooc_kernel<256, -1>), dim3((unsigned)grid),
                       dim3(256), 0, stream, u_indptr, u_items, i_indptr,
                       i_users, rows, n_rows, n, pool, n_items, top_ids,
                       top_cnt);
}

extern "C" int cooc_dense_lds_max() { return CO_DENSE_LDS; }
