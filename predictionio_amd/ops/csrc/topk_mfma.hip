// MFMA-based masked top-K scoring for MI355X (gfx950, CDNA4).
//
// The serve hot path: the B x N x F score computation runs on the
// matrix cores (v_mfma_f32_16x16x32_bf16, bf16 inputs / fp32 accumulate)
// instead of the VALU fp32 dot loop of topk_score_kernel. Same
// reference semantics (recommendProductsWithFilter
// examples/.../ALSModel.scala:44-60, ecommerce predictKnownUser
// ECommAlgorithm.scala:471-506, similarproduct cosine top-N
// ALSAlgorithm.scala:168-242); the Python wrapper re-checks the bf16
// survivors against the fp32 factors so served scores stay exact.
//
// Geometry (per 256-thread workgroup, 4 waves):
//  - the block owns 64 queries; wave w owns queries [16w, 16w+16)
//  - item slices: grid = (ublocks, n_slices); blockIdx.x is the ublock
//    so concurrently-resident workgroups share one Y slice through L3
//  - per chunk of TM_CHUNK=64 items: Y rows are reg-staged into LDS as
//    bf16 with an XOR swizzle ((row & SWM) << 4 on the byte offset, the
//    bank-conflict fix for "different rows, same col-range" b128
//    reads), then each wave runs (TM_CHUNK/16) x (F/32) MFMAs:
//       A = Y tile   (lane holds Y[item = l&15][k = (l>>4)*8 + i])
//       B = X^T tile (lane holds X[query = l&15][k = (l>>4)*8 + i]),
//    accumulating D[item][query] in fp32 (D: col = l&15 = query,
//    row = (l>>4)*4 + reg = item) — operand maps per the CK xdlops
//    contract and the measured gfx950 C/D layout.
//
// Top-K epilogue:
//  - ONE top-K list per (query, workgroup) in LDS, with the running
//    K-th-best threshold also in LDS (th_lds[wave*16 + query]).
//  - common case per chunk: each lane max-reduces its 16 accumulator
//    values (15 v_max), reads the shared threshold (one broadcast
//    ds_read) and skips everything else — ~25 instructions per
//    64 items x 16 queries.
//  - rare case (some lane's max beats the threshold): the 4 lanes of a
//    query's quad take turns (serialized by lane group, exec-masked —
//    a single wave executes groups in program order, and within one
//    group every active lane owns a DIFFERENT query, so list writes
//    never contend) scanning their values and inserting; masks/bans are
//    only consulted here.
//  - inserts per query = K ln(items/K) per LIST, so one shared list per
//    query keeps both the insert count and the list LDS (64 lists) low
//    enough for 6-7 workgroups/CU.
//
// The X fragments live in registers for the whole kernel (loaded once);
// item staging is software-pipelined through registers, with the next
// chunk's loads issued AFTER the second barrier so they fly under the
// MFMA phase (a __syncthreads compiles to s_waitcnt vmcnt(0) — loads
// issued before it would be drained at the barrier).
//
// This is the one schedule that ships; the neighbouring schedules that
// were measured and rejected are recorded in NOTES.md.

#include <float.h>
#include <stdlib.h>
#include <type_traits>
#include <hip/hip_runtime.h>

#include "topk_common.h"

#define TM_CHUNK 64   // items staged per LDS pass
#define TM_WAVES 4
#define TM_QPW 16     // queries per wave
#define TM_UPB (TM_WAVES * TM_QPW)  // queries per block
#define TM_BS (TM_WAVES * 64)       // block size

// Row stride (words) of the staged category words, word-major
// [CW][stride]. TM_CHUNK + 32/CW for CW > 1: the drain's transpose store
// has lanes t..t+CW-1 writing the CW words of one item, and with a stride
// of TM_CHUNK (a multiple of the 32 write banks) they collided CW ways;
// the pad spreads a half-wave's CW rows over disjoint bank ranges and
// keeps every row 16 B aligned for the epilogue's ds_read_b128.
constexpr int tm_cats_stride(int cw) {
  return cw > 1 ? TM_CHUNK + 32 / cw : TM_CHUNK;
}

// Dynamic LDS layout, in order (KP = K + 1):
//   ys     [TM_CHUNK][F]          bf16  staged Y chunk (swizzled)
//   cats   [CW][tm_cats_stride]   u32   staged item category words
//   topv   [TM_UPB][KP]           f32   per-query top-K values
//   topi   [TM_UPB][KP]           i32   per-query top-K items
//   th     [TM_UPB]               f32   per-query K-th-best threshold
//   qc     [CW][TM_UPB]           u32   per-query accepted words
// At most 52 KB (F=128, K=64, CW=4). ops/topk.py sizes n_slices from the
// same sum.
constexpr size_t tm_lds_bytes(int f, int K, int cw) {
  return (size_t)TM_CHUNK * (f * 2) +
         (size_t)cw * tm_cats_stride(cw) * 4 +
         (sizeof(float) + sizeof(int)) * TM_UPB * (K + 1) +
         sizeof(float) * TM_UPB + sizeof(int) * TM_UPB * cw;
}

typedef __attribute__((ext_vector_type(8))) unsigned short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// Order-preserving float<->u32 map for atomicMax on scores (classic
// sign-flip transform: negative floats map to ~bits, non-negative to
// bits|0x80000000, making unsigned order == float order).
__device__ __forceinline__ unsigned tm_enc(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tm_dec(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// PROF=true compiles in wall_clock64() phase accumulators, summed per
// workgroup into prof[5] = {setup, stage, score, write, blocks}.
//
// CW = category words per item/query (0 = no category filter). With
// CW > 0 item j is a candidate for query b iff
//   OR_w (item_cats[j,w] & query_cats[b,w]) != 0.
// The filter runs BEFORE the threshold test (scores of filtered items
// become -FLT_MAX ahead of the max-reduce), not in the insert path where
// item_mask/bans are checked: under a selective filter the K-th-best
// threshold stays low relative to unfiltered scores, so an insert-time
// filter would send almost every chunk into the serialized lane-group
// slow path with a dependent global load per value. The chunk's
// TM_CHUNK x CW words ride the same register-staged pipeline as the Y
// tile, into a word-major LDS image so a lane's four D rows are one b128.
// Every CW > 0 line sits under `if constexpr`; CW == 0 is unchanged.
//
// ILV = true interleaves the slices at chunk granularity: slice s takes
// the TM_CHUNK-item chunks s, s + n_slices, s + 2 n_slices, ... of the
// whole item range instead of one contiguous run. The union path for
// K > 64 (ops/topk.py) needs it: item ids follow first appearance, so the
// popular, large-norm items cluster at low ids and a contiguous slice
// would hold far more than its share of a query's best items. A slice
// past the last chunk loads nothing and writes K empty slots. Every ILV
// line is a compile-time branch; ILV == false is unchanged.
template <int F, bool PROF, int CW = 0, bool ILV = false>
__global__ __launch_bounds__(TM_BS, 6)
void topk_mfma_kernel(
    const unsigned short* __restrict__ Xq,   // B x F bf16
    const unsigned short* __restrict__ Y,    // N x F bf16
    const uint8_t* __restrict__ item_mask,   // N or nullptr
    const long long* __restrict__ ban_indptr,
    const int* __restrict__ ban_indices,
    float* __restrict__ out_val,             // B x n_slices x K
    int* __restrict__ out_idx,
    int B, long long N, int K, int n_slices, int item_base,
    unsigned long long* prof,
    // optional [B] cross-slice threshold (tm_enc-coded, init 0): the
    // concurrently-running WGs of a query's OTHER slices publish their
    // K-th-best through L2, so each slice stops re-paying the full
    // insert ramp from -inf (insert volume was ~linear in n_slices)
    unsigned* __restrict__ th_g,
    int kflags,  // bit 0: disable the ban bloom (A/B hook)
    const int* __restrict__ item_cats,   // N x CW bit words (CW > 0)
    const int* __restrict__ query_cats)  // B x CW accepted-bit words
{
  static_assert(CW == 0 || CW == 1 || CW == 2 || CW == 4,
                "category words per item must be 1, 2 or 4");
  static_assert(CW == 0 || !PROF, "no phase probe with the category filter");
  static_assert(!ILV || !PROF, "no phase probe with interleaved slices");
  static_assert(TM_CHUNK * CW <= TM_BS,
                "one staged category word per thread");
  constexpr int ROWB = F * 2;            // bytes per staged Y row
  constexpr int SWM = (F >= 64) ? 7 : 3; // XOR-swizzle row mask
  constexpr int KS = F / 32;             // MFMA K-steps per dot product
  constexpr int IFR = TM_CHUNK / 16;     // item fragments per chunk
  constexpr int CSTR = tm_cats_stride(CW);
  // carve-up of the dynamic LDS: see tm_lds_bytes
  extern __shared__ char lds_raw[];
  unsigned short* ys = reinterpret_cast<unsigned short*>(lds_raw);
  unsigned* cats_lds = reinterpret_cast<unsigned*>(lds_raw + TM_CHUNK * ROWB);
  float* topv = reinterpret_cast<float*>(
      lds_raw + TM_CHUNK * ROWB + CW * CSTR * 4);
  const int KP = K + 1;  // stride coprime with the 32 banks
  int* topi = reinterpret_cast<int*>(topv + TM_UPB * KP);
  float* th_lds = reinterpret_cast<float*>(topi + TM_UPB * KP);
  unsigned* qc_lds = reinterpret_cast<unsigned*>(th_lds + TM_UPB);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int lg = lane >> 4;   // lane group: k-slice on input, item rows out
  const int lq = lane & 15;   // query column (B operand / D col)

  const bool probe = PROF && tid == 0;
  unsigned long long pt = 0, acc_setup = 0, acc_stage = 0, acc_score = 0;
  if (probe) pt = wall_clock64();

  const long long u0 = (long long)blockIdx.x * TM_UPB;
  const long long guser = u0 + wave * TM_QPW + lq;
  const bool has_user = guser < B;
  const int slice = blockIdx.y;
  const long long per = (N + n_slices - 1) / n_slices;
  const long long it0 =
      ILV ? (long long)slice * TM_CHUNK : (long long)slice * per;
  const long long it1 = ILV ? N : min(N, it0 + per);

  // ---- X fragments: one b128 per K-step, held for the whole kernel
  bf16x8 xf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    if (has_user) {
      xf[ks] = *reinterpret_cast<const bf16x8*>(
          &Xq[guser * F + ks * 32 + lg * 8]);
    } else {
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      xf[ks] = z;
    }
  }

  // ---- init the per-query top-K lists + shared thresholds
  for (int e = tid; e < TM_UPB * KP; e += TM_BS) {
    topv[e] = -FLT_MAX;
    topi[e] = -1;
  }
  if (tid < TM_UPB) th_lds[tid] = -FLT_MAX;
  __syncthreads();

  // this lane's query's banned list, and a 64-bit bloom over it: the
  // insert path's binary search is ~5 DEPENDENT global loads inside the
  // serialized lane-group loop, so a one-register membership pre-test
  // that skips it for definitely-unbanned items pays for itself after a
  // handful of inserts (~47% false-positive at 30 bans; saturates
  // harmlessly for huge lists). Built once at setup from the lane's own
  // list.
  const int* ban = nullptr;
  int bn = 0;
  unsigned long long bloom = 0ull;
  if (ban_indptr != nullptr && has_user) {
    const long long b0 = ban_indptr[guser];
    bn = (int)(ban_indptr[guser + 1] - b0);
    ban = ban_indices + b0;
    if ((kflags & 1) || bn > 512) {
      // disabled, or the list is big enough that the 64-bit bloom
      // would saturate anyway — skip the build, every check falls
      // through to the binary search (measured 0.998x at 300 bans)
      bloom = ~0ull;
    } else {
      for (int t = 0; t < bn; ++t)
        bloom |= 1ull << ((unsigned)((unsigned)ban[t] * 2654435761u) >> 26);
    }
  }
  // each query's accepted-category words, loaded once: word-major
  // [CW][TM_UPB] in LDS, not registers — under the 80-VGPR cap CW live
  // registers per lane spilled the hot loop (F=64, CW=4: 444 B/lane of
  // scratch against 196 B with the words in LDS). Queries past B hold
  // zero, which filters everything.
  if constexpr (CW > 0) {
    if (lg == 0) {
#pragma unroll
      for (int w = 0; w < CW; ++w)
        qc_lds[w * TM_UPB + wave * TM_QPW + lq] = has_user
            ? (unsigned)query_cats[guser * CW + w] : 0u;
    }
    // read back only by the writing wave's lanes, after the chunk
    // loop's barriers
  }
  if (probe) {
    const unsigned long long now = wall_clock64();
    acc_setup = now - pt;
    pt = now;
  }

  // ---- software-pipelined staging registers (granules of 16 B)
  constexpr int NG = (TM_CHUNK * ROWB) / 16 / TM_BS;  // granules per thread
  static_assert(NG >= 1, "chunk must cover one granule per thread");
  u32x4 stg[NG];
  // per-thread element offsets are chunk-invariant: loads use ONE
  // running base pointer advanced by a constant per chunk (the naive
  // form re-did ~20 64-bit address ops per chunk in the hot loop)
  int goff[NG];
  int grow[NG];
#pragma unroll
  for (int r = 0; r < NG; ++r) {
    const int lin = (tid + r * TM_BS) * 16;
    grow[r] = lin / ROWB;
    goff[r] = grow[r] * F + (lin % ROWB) / 2;
  }
  // category staging: the chunk's TM_CHUNK*CW words are contiguous in
  // global memory (item-major), so thread t < TM_CHUNK*CW carries word t
  // of the chunk — one coalesced dword per thread — and transposes it to
  // the word-major LDS image on drain. Rows at or past it1 stage 0 =
  // "filtered", which also covers the tail chunk.
  unsigned cstg = 0u;
  auto load_stg = [&](long long cbase) {
    if constexpr (CW > 0) {
      if (tid < TM_CHUNK * CW)
        cstg = (cbase + tid / CW < it1)
            ? (unsigned)item_cats[cbase * CW + tid] : 0u;
    }
    const unsigned short* yb_g = Y + cbase * F;
    const bool tail = cbase + TM_CHUNK > it1;
    if (!tail) {
#pragma unroll
      for (int r = 0; r < NG; ++r)
        stg[r] = *reinterpret_cast<const u32x4*>(&yb_g[goff[r]]);
    } else {
#pragma unroll
      for (int r = 0; r < NG; ++r)
        stg[r] = (cbase + grow[r] < it1)
            ? *reinterpret_cast<const u32x4*>(&yb_g[goff[r]])
            : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto drain = [&]() {
#pragma unroll
    for (int r = 0; r < NG; ++r) {
      const int lin = (tid + r * TM_BS) * 16;
      const int row = lin / ROWB;
      const int col = lin % ROWB;
      const int dst = row * ROWB + (col ^ ((row & SWM) << 4));
      *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(ys) + dst) = stg[r];
    }
    if constexpr (CW > 0) {
      if (tid < TM_CHUNK * CW) cats_lds[(tid % CW) * CSTR + tid / CW] = cstg;
    }
  };
  // pipelined cross-slice threshold: the register holds the value read
  // one fold period ago (tm_enc-coded; 0 decodes below every real
  // score, so the first fold is a no-op)
  unsigned gth_pipe =
      (th_g != nullptr && lg == 0 && has_user) ? th_g[guser] : 0u;
  int n_chunks;
  if constexpr (ILV) {
    const long long nch = (N + TM_CHUNK - 1) / TM_CHUNK;
    n_chunks =
        slice < nch ? (int)((nch - slice + n_slices - 1) / n_slices) : 0;
  } else {
    n_chunks = (int)((it1 - it0 + TM_CHUNK - 1) / TM_CHUNK);
  }
  // items between the starts of a slice's consecutive chunks
  const long long cstep = ILV ? (long long)n_slices * TM_CHUNK : TM_CHUNK;
  if (!ILV || n_chunks > 0) load_stg(it0);

  for (int ci = 0; ci < n_chunks; ++ci) {
    const long long base = it0 + (long long)ci * cstep;
    __syncthreads();  // all waves done reading the previous chunk
    drain();
    // fold the cross-slice global threshold into the local one every
    // 8 chunks; each wave's lg==0 lanes update only their own wave's
    // lists, and the barrier below orders the write before the
    // epilogue's reads. PIPELINED: consume the value LOADED 8 CHUNKS
    // AGO (a barrier since then already paid its vmcnt, so the fold
    // never stalls on the load) and issue the next one; thresholds
    // are monotonic so an 8-chunk-stale value only prunes less.
    if (th_g != nullptr && (ci & 7) == 0 && lg == 0) {
      if (has_user) {
        const int ml = wave * TM_QPW + lq;
        const float gv = tm_dec(gth_pipe);
        if (gv > th_lds[ml]) th_lds[ml] = gv;
        gth_pipe = th_g[guser];
      }
    }
    __syncthreads();
    // issue the NEXT chunk's global loads AFTER the barrier (a
    // __syncthreads compiles to s_waitcnt vmcnt(0)) so they fly
    // under the MFMA phase
    if constexpr (ILV) {
      if (ci + 1 < n_chunks) load_stg(base + cstep);
    } else {
      if (base + TM_CHUNK < it1) load_stg(base + TM_CHUNK);
    }
    if (probe) {
      const unsigned long long now = wall_clock64();
      acc_stage += now - pt;
      pt = now;
    }

    // ---- MFMA: every wave scores the whole chunk for its queries
    const int mylist = wave * TM_QPW + lq;
    float* tvu = topv + mylist * KP;
    int* tiu = topi + mylist * KP;
    f32x4 acc[IFR];
#pragma unroll
    for (int i = 0; i < IFR; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int i = 0; i < IFR; ++i) {
        const int row = i * 16 + lq;           // A operand row = item
        const int col = ks * 64 + lg * 16;     // byte offset of k-slice
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(
            reinterpret_cast<const char*>(ys) +
            row * ROWB + (col ^ ((row & SWM) << 4)));
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, xf[ks], acc[i], 0, 0, 0);
      }
    }

    // ---- category filter, ahead of the threshold test: a filtered
    // score becomes -FLT_MAX, which is never > th, so the max-reduce,
    // the serialized insert, the cross-slice publish/fold and the
    // write-out below need no change. One b128 per item fragment per
    // word: the lane's D rows i*16 + lg*4 + r are contiguous in
    // [w][CSTR].
    if constexpr (CW > 0) {
#pragma unroll
      for (int i = 0; i < IFR; ++i) {
        u32x4 hit = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int w = 0; w < CW; ++w) {
          const u32x4 c = *reinterpret_cast<const u32x4*>(
              &cats_lds[w * CSTR + i * 16 + lg * 4]);
          hit |= c & qc_lds[w * TM_UPB + mylist];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[i][r] = hit[r] != 0u ? acc[i][r] : -FLT_MAX;
      }
    }

    // ---- epilogue: common case is one max-reduce + one threshold read
    float mymax = -FLT_MAX;
#pragma unroll
    for (int i = 0; i < IFR; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) mymax = fmaxf(mymax, acc[i][r]);
    const float th_b = th_lds[mylist];
    if (has_user && mymax > th_b) {
      // serialize the query's 4 lane groups: exec-masked blocks of one
      // wave run in program order, and within a group the active lanes
      // all own different queries, so list writes never contend.
      // MUST be a runtime loop with an opaque barrier per iteration:
      // with `#pragma unroll` the four structurally-identical blocks
      // got tail-merged by the compiler into ONE exec-masked block
      // (it does not model cross-lane LDS aliasing), so all groups
      // read the threshold before any insert — losing inserts (a K=1
      // test failed: later groups overwrote the max).
#pragma unroll 1
      for (int g = 0; g < 4; ++g) {
        asm volatile("" ::: "memory");  // keep iterations distinct
        if (lg == g) {
          float th = th_lds[mylist];
          // 32-bit tail guard: li < lim replaces the former 64-bit
          // `item < it1` (16 hoisted v_cmp_gt_i64 in the fast loop)
          const int lim =
              (int)(it1 - base < TM_CHUNK ? it1 - base : TM_CHUNK);
#pragma unroll
          for (int i = 0; i < IFR; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int li = i * 16 + lg * 4 + r;      // D row
              const long long item = base + li;
              const float s = acc[i][r];
              if (s > th && li < lim) {
                const int gitem = (int)(item + item_base);
                const bool may_ban =
                    ban != nullptr &&
                    (bloom >>
                     ((unsigned)((unsigned)gitem * 2654435761u) >> 26)) & 1;
                if ((item_mask == nullptr || !item_mask[item]) &&
                    (!may_ban || !in_sorted(ban, bn, gitem))) {
                  int mi = 0;
                  float mv = tvu[0];
                  for (int q = 1; q < K; ++q)
                    if (tvu[q] < mv) { mv = tvu[q]; mi = q; }
                  tvu[mi] = s;
                  tiu[mi] = (int)(item + item_base);
                  float nm = tvu[0];
                  for (int q = 1; q < K; ++q) nm = fminf(nm, tvu[q]);
                  th = nm;
                  th_lds[mylist] = nm;
                  // publish to the other slices once the list is full;
                  // test-and-test-and-set: the plain read (L2-hot)
                  // filters publishes already beaten by another slice,
                  // keeping the atomic queue short
                  if (th_g != nullptr && nm > -FLT_MAX &&
                      tm_enc(nm) > th_g[guser])
                    atomicMax(&th_g[guser], tm_enc(nm));
                }
              }
            }
          }
        }
      }
    }
    if (probe) {
      const unsigned long long now = wall_clock64();
      acc_score += now - pt;
      pt = now;
    }
  }
  __syncthreads();
  if (probe) pt = wall_clock64();

  // ---- write out: one candidate group per slice per query
  for (int e = tid; e < TM_UPB * K; e += TM_BS) {
    const int list = e / K;
    const int q = e % K;
    const long long gu = u0 + list;
    if (gu < B) {
      const long long o = (gu * n_slices + slice) * (long long)K + q;
      out_val[o] = topv[list * KP + q];
      out_idx[o] = topi[list * KP + q];
    }
  }
  if (probe) {
    atomicAdd(&prof[0], acc_setup);
    atomicAdd(&prof[1], acc_stage);
    atomicAdd(&prof[2], acc_score);
    atomicAdd(&prof[3], wall_clock64() - pt);
    atomicAdd(&prof[4], 1ull);
  }
}

// args = the kernel's arguments, in order
template <int F, bool PROF, int CW, bool ILV, typename... Args>
static void launch(dim3 grid, int K, hipStream_t stream, Args... args) {
  launch_dyn_lds<topk_mfma_kernel<F, PROF, CW, ILV>>(
      grid, dim3(TM_BS), tm_lds_bytes(F, K, CW), stream, args...);
}

template <int F, int CW, typename... Args>
static void launch_cw(bool ilv, Args... args) {
  if (ilv) launch<F, false, CW, true>(args...);
  else launch<F, false, CW, false>(args...);
}

// the binding rejects prof together with a category filter or with
// interleaved slices
template <int F, typename... Args>
static void launch_rank(bool prof, int cw, bool ilv, Args... args) {
  switch (cw) {
    case 0:
      if (prof) launch<F, true, 0, false>(args...);
      else launch_cw<F, 0>(ilv, args...);
      break;
    case 1: launch_cw<F, 1>(ilv, args...); break;
    case 2: launch_cw<F, 2>(ilv, args...); break;
    case 4: launch_cw<F, 4>(ilv, args...); break;
    default: break;
  }
}

extern "C" void launch_topk_mfma(
    const unsigned short* Xq, const unsigned short* Y,
    const uint8_t* item_mask, const long long* ban_indptr,
    const int* ban_indices, float* out_val, int* out_idx,
    int B, long long N, int f, int K, int n_slices, int item_base,
    unsigned long long* prof, unsigned* th_g,
    const int* item_cats, const int* query_cats, int cw, int interleave,
    hipStream_t stream)
{
  const dim3 grid((B + TM_UPB - 1) / TM_UPB, n_slices);
  const char* e_bl = getenv("PIO_TOPK_BLOOM");
  const int kflags = (e_bl != nullptr && e_bl[0] == '0') ? 1 : 0;
  // the rank arrives as a compile-time tag so the argument list is
  // written once
  auto go = [&](auto rank) {
    launch_rank<decltype(rank)::value>(
        prof != nullptr, cw, interleave != 0, grid, K, stream, Xq, Y,
        item_mask, ban_indptr, ban_indices, out_val, out_idx, B, N, K,
        n_slices, item_base, prof, th_g, kflags, item_cats, query_cats);
  };
  switch (f) {
    case 32: go(std::integral_constant<int, 32>{}); break;
    case 64: go(std::integral_constant<int, 64>{}); break;
    case 128: go(std::integral_constant<int, 128>{}); break;
    default: break;
  }
}
