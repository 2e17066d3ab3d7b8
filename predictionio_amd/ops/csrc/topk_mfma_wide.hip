// MFMA masked top-K scoring for factor ranks 129..512 on MI355X (gfx950,
// CDNA4): the schedule of topk_mfma.hip with the rank streamed through LDS
// in 128-wide PANELS.
//
// topk_mfma_kernel<F> stages a whole 64-item x F bf16 chunk per pass; at
// F = 512 that is 64 KB of LDS for the tile alone. Here the padded rank is
// F = 128 * NP (NP = 2, 3, 4) and a chunk is staged one panel (64 items x
// 128 bf16 = 16 KB) at a time, double buffered, so the tile costs 32 KB at
// every NP and the chunk's accumulators simply stay in registers until its
// last panel has been multiplied in.
//
// Geometry (per 256-thread workgroup, 4 waves) — as topk_mfma.hip:
//  - the block owns 64 queries; wave w owns queries [16w, 16w+16)
//  - grid = (ublocks, n_slices); a slice is a contiguous item run, or
//    (ILV) every n_slices-th 64-item chunk
//  - v_mfma_f32_16x16x32_bf16 with the items as A and the queries as B:
//       A lane holds Y[item = l&15][k = (l>>4)*8 + i]
//       B lane holds X[query = l&15][k = (l>>4)*8 + i]
//       D: col = l&15 = query, row = (l>>4)*4 + reg = item
//  - the wave's X fragments for ALL panels are loaded once and held in
//    registers: xf[p*4 + ks] covers k = 128p + 32ks + [0, 32), one bf16x8
//    per lane per k-step, F/8 VGPRs (64 at F = 512).
//
// Panel pipeline. Step s = chunk * NP + p works on LDS buffer s & 1:
//     issue the global loads of panel s+1 into 4 staging b128 registers
//       (panel p+1 of this chunk, or panel 0 of the slice's next chunk)
//     16 MFMAs per wave on buffer s & 1: 4 item fragments x 4 k-steps,
//       A = ds_read_b128 with the XOR swizzle of the F = 128 kernel
//       (byte col ^ ((row & 7) << 4)), B = xf[p*4 + ks]
//     write the staging registers to buffer (s+1) & 1
//     if p == NP-1: the top-K epilogue on the 16 accumulators
//     ONE barrier
// The barrier that ends step s-1 is what makes buffer (s+1) & 1 free to
// overwrite (every wave has finished reading it) and what publishes buffer
// s & 1. The loads are issued after that barrier and consumed before the
// next one, so they fly under the MFMAs (a barrier drains vmcnt).
// The k-order is fixed in one place each: panel p of a Y row is its bf16
// elements [128p, 128p+128) (load_stg), k-step ks of a staged row is its
// bytes [64ks, 64ks+64) (the A read), and xf[p*4 + ks] is loaded from the
// same element range of the query row.
//
// The chunk's category words and item weights are loaded with panel 0 and
// used by the epilogue NP steps later — while panel 0 of the NEXT chunk is
// already being written. They are therefore double buffered too, by chunk
// parity (a few hundred bytes).
//
// Top-K epilogue, output layout and the empty-slot convention are those of
// topk_mfma_kernel: one shared list of length K per (query, workgroup) with
// its threshold in LDS, a max-reduce + one threshold read in the common
// case, the query's four lane groups serialized on the rare insert path,
// item_mask / ban lists checked at insert, category words and weights
// applied before the threshold test, the optional cross-slice threshold
// cell folded in every 8 chunks. See that file for the reasoning behind
// each of them; the comments here only mark what differs.

#include <float.h>
#include <stdlib.h>
#include <type_traits>
#include <hip/hip_runtime.h>

#include "topk_common.h"

#define TW_CHUNK 64    // items per chunk
#define TW_PANEL 128   // rank columns per panel
#define TW_WAVES 4
#define TW_QPW 16      // queries per wave
#define TW_UPB (TW_WAVES * TW_QPW)  // queries per block
#define TW_BS (TW_WAVES * 64)       // block size
#define TW_ROWB (TW_PANEL * 2)      // bytes per staged panel row
#define TW_PANEL_BYTES (TW_CHUNK * TW_ROWB)

// Row stride (words) of the staged category words, word-major
// [CW][stride]: padded for CW > 1 so the transpose store of the drain does
// not land CW-way on one bank, rows kept 16 B aligned for the b128 reads.
constexpr int tw_cats_stride(int cw) {
  return cw > 1 ? TW_CHUNK + 32 / cw : TW_CHUNK;
}

// Dynamic LDS layout, in order (KP = K + 1):
//   ys     [2][TW_CHUNK][TW_PANEL]    bf16  panel double buffer (swizzled)
//   cats   [2][CW][tw_cats_stride]    u32   item category words, by chunk
//                                           parity
//   wts    [2][TW_CHUNK]              f32   item weights, by chunk parity
//                                           (WT only)
//   topv   [TW_UPB][KP]               f32   per-query top-K values
//   topi   [TW_UPB][KP]               i32   per-query top-K items
//   th     [TW_UPB]                   f32   per-query K-th-best threshold
//   qc     [CW][TW_UPB]               u32   per-query accepted words
// The panel count does not enter: the panels of a chunk pass through the
// same two buffers. 32 KB + lists: 40.75 KB at K = 16 unfiltered, 68.5 KB
// at K = 64 with CW = 4 and WT. ops/topk.py sizes n_slices from the same sum.
constexpr size_t tw_lds_bytes(int np, int K, int cw, bool wt) {
  (void)np;
  return (size_t)2 * TW_PANEL_BYTES +
         (size_t)2 * cw * tw_cats_stride(cw) * 4 +
         (wt ? 2 * sizeof(float) * TW_CHUNK : 0) +
         (sizeof(float) + sizeof(int)) * TW_UPB * (K + 1) +
         sizeof(float) * TW_UPB + sizeof(int) * TW_UPB * cw;
}

typedef __attribute__((ext_vector_type(8))) unsigned short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// order-preserving float <-> u32 map of the cross-slice threshold cell
// (the coding of topk_mfma.hip: the binding zero-initializes the cell, and
// 0 decodes below every real score)
__device__ __forceinline__ unsigned tw_enc(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tw_dec(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// Workgroups per CU the register allocation is held to. The LDS admits 3
// (K <= 16) or fewer, so 3 (a cap of 168 VGPRs) is all NP = 2 and 3 need.
// NP = 4 holds 64 VGPRs of X fragments next to 16 staging and 16
// accumulators and, held to 168, four of its instantiations spilled 12 B
// per lane: it is bound to 2, under which none spills and those that still
// fit in 168 VGPRs (the unfiltered, unweighted ones among them) keep 3
// workgroups per CU. Figures per instantiation: NOTES.md.
constexpr int tw_min_blocks(int np) { return np >= 4 ? 2 : 3; }

template <int NP, int CW, bool ILV, bool WT>
__global__ __launch_bounds__(TW_BS, tw_min_blocks(NP))
void topk_mfma_wide_kernel(
    const unsigned short* __restrict__ Xq,   // B x F bf16, F = 128 NP
    const unsigned short* __restrict__ Y,    // N x F bf16
    const uint8_t* __restrict__ item_mask,   // N or nullptr
    const long long* __restrict__ ban_indptr,
    const int* __restrict__ ban_indices,
    float* __restrict__ out_val,             // B x n_slices x K
    int* __restrict__ out_idx,
    int B, long long N, int K, int n_slices, int item_base,
    unsigned* __restrict__ th_g,   // optional [B] cross-slice threshold
    int kflags,                    // bit 0: disable the ban bloom
    const int* __restrict__ item_cats,   // N x CW bit words (CW > 0)
    const int* __restrict__ query_cats,  // B x CW accepted-bit words
    const float* __restrict__ item_weights)  // N score weights (WT)
{
  static_assert(NP >= 2 && NP <= 4, "rank panels: 2, 3 or 4");
  static_assert(CW == 0 || CW == 1 || CW == 2 || CW == 4,
                "category words per item must be 1, 2 or 4");
  static_assert(TW_CHUNK * CW <= TW_BS,
                "one staged category word per thread");
  constexpr int F = NP * TW_PANEL;
  constexpr int KSP = TW_PANEL / 32;     // MFMA k-steps per panel
  constexpr int IFR = TW_CHUNK / 16;     // item fragments per chunk
  constexpr int CSTR = tw_cats_stride(CW);
  // carve-up of the dynamic LDS: see tw_lds_bytes
  extern __shared__ char lds_raw[];
  char* ys = lds_raw;
  unsigned* cats_lds = reinterpret_cast<unsigned*>(ys + 2 * TW_PANEL_BYTES);
  float* wts_lds = reinterpret_cast<float*>(cats_lds + 2 * CW * CSTR);
  float* topv = wts_lds + (WT ? 2 * TW_CHUNK : 0);
  const int KP = K + 1;  // stride coprime with the 32 banks
  int* topi = reinterpret_cast<int*>(topv + TW_UPB * KP);
  float* th_lds = reinterpret_cast<float*>(topi + TW_UPB * KP);
  unsigned* qc_lds = reinterpret_cast<unsigned*>(th_lds + TW_UPB);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int lg = lane >> 4;   // lane group: k-slice on input, item rows out
  const int lq = lane & 15;   // query column (B operand / D col)

  const long long u0 = (long long)blockIdx.x * TW_UPB;
  const long long guser = u0 + wave * TW_QPW + lq;
  const bool has_user = guser < B;
  const int slice = blockIdx.y;
  const long long per = (N + n_slices - 1) / n_slices;
  const long long it0 =
      ILV ? (long long)slice * TW_CHUNK : (long long)slice * per;
  const long long it1 = ILV ? N : min(N, it0 + per);

  // ---- X fragments of every panel, held for the whole kernel
  bf16x8 xf[NP * KSP];
#pragma unroll
  for (int k = 0; k < NP * KSP; ++k) {
    if (has_user) {
      xf[k] = *reinterpret_cast<const bf16x8*>(
          &Xq[guser * F + k * 32 + lg * 8]);
    } else {
      bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      xf[k] = z;
    }
  }

  // ---- init the per-query top-K lists + shared thresholds
  for (int e = tid; e < TW_UPB * KP; e += TW_BS) {
    topv[e] = -FLT_MAX;
    topi[e] = -1;
  }
  if (tid < TW_UPB) th_lds[tid] = -FLT_MAX;

  // this lane's query's banned list and the 64-bit bloom over it
  const int* ban = nullptr;
  int bn = 0;
  unsigned long long bloom = 0ull;
  if (ban_indptr != nullptr && has_user) {
    const long long b0 = ban_indptr[guser];
    bn = (int)(ban_indptr[guser + 1] - b0);
    ban = ban_indices + b0;
    if ((kflags & 1) || bn > 512) {
      bloom = ~0ull;
    } else {
      for (int t = 0; t < bn; ++t)
        bloom |= 1ull << ((unsigned)((unsigned)ban[t] * 2654435761u) >> 26);
    }
  }
  // each query's accepted-category words, word-major in LDS; queries past
  // B hold zero, which filters everything. Read back only by the writing
  // wave's lanes.
  if constexpr (CW > 0) {
    if (lg == 0) {
#pragma unroll
      for (int w = 0; w < CW; ++w)
        qc_lds[w * TW_UPB + wave * TW_QPW + lq] = has_user
            ? (unsigned)query_cats[guser * CW + w] : 0u;
    }
  }

  // ---- staging registers: a panel is 1024 granules of 16 B, 4 per
  // thread. Granule r of thread t is row t/16 + 16r, bytes (t%16)*16 of
  // the panel row: 16 consecutive threads read one row's 256 B.
  constexpr int NG = TW_PANEL_BYTES / 16 / TW_BS;
  static_assert(NG == 4, "four staging granules per thread");
  const int srow = tid >> 4;            // + 16 r
  const int scol = (tid & 15) * 16;     // byte column inside the panel row
  u32x4 stg[NG];
  unsigned cstg = 0u;   // thread t < TW_CHUNK*CW: category word t of the chunk
  float wstg = 0.f;     // thread t < TW_CHUNK: weight of the chunk's item t
  // panel p of the chunk whose first item is cbase (cbase < it1)
  auto load_stg = [&](long long cbase, int p) {
    if (p == 0) {
      if constexpr (WT) {
        if (tid < TW_CHUNK)
          wstg = (cbase + tid < it1) ? item_weights[cbase + tid] : 0.f;
      }
      if constexpr (CW > 0) {
        if (tid < TW_CHUNK * CW)
          cstg = (cbase + tid / CW < it1)
              ? (unsigned)item_cats[cbase * CW + tid] : 0u;
      }
    }
    // Rows at or past it1 re-read the slice's last row instead of
    // branching to a zero fill (a conditional load makes the compiler
    // wait for the whole panel ahead of the MFMAs): their scores are never
    // inserted (li < lim below) and their category word / weight is 0.
    // 64-bit row offset; the column part stays 32-bit.
    const int nrow = (int)(it1 - cbase < TW_CHUNK ? it1 - cbase : TW_CHUNK);
    const unsigned short* yb_g = Y + (p * TW_PANEL + (tid & 15) * 8);
#pragma unroll
    for (int r = 0; r < NG; ++r) {
      const int row = min(srow + 16 * r, nrow - 1);
      stg[r] = *reinterpret_cast<const u32x4*>(yb_g + (cbase + row) * F);
    }
  };
  // staging registers -> panel buffer `buf`; with p == 0 also the chunk's
  // category words / weights -> their buffer `cpar` (the chunk's parity)
  auto drain = [&](int buf, int p, int cpar) {
    char* yb = ys + buf * TW_PANEL_BYTES;
#pragma unroll
    for (int r = 0; r < NG; ++r) {
      const int row = srow + 16 * r;
      *reinterpret_cast<u32x4*>(
          yb + row * TW_ROWB + (scol ^ ((row & 7) << 4))) = stg[r];
    }
    if (p == 0) {
      if constexpr (CW > 0) {
        if (tid < TW_CHUNK * CW)
          cats_lds[cpar * CW * CSTR + (tid % CW) * CSTR + tid / CW] = cstg;
      }
      if constexpr (WT) {
        if (tid < TW_CHUNK) wts_lds[cpar * TW_CHUNK + tid] = wstg;
      }
    }
  };

  // cross-slice threshold, pipelined: the register holds the value read
  // one fold period ago
  unsigned gth_pipe =
      (th_g != nullptr && lg == 0 && has_user) ? th_g[guser] : 0u;
  int n_chunks;
  if constexpr (ILV) {
    const long long nch = (N + TW_CHUNK - 1) / TW_CHUNK;
    n_chunks =
        slice < nch ? (int)((nch - slice + n_slices - 1) / n_slices) : 0;
  } else {
    n_chunks = it1 > it0 ? (int)((it1 - it0 + TW_CHUNK - 1) / TW_CHUNK) : 0;
  }
  // items between the starts of a slice's consecutive chunks
  const long long cstep = ILV ? (long long)n_slices * TW_CHUNK : TW_CHUNK;

  // prologue: panel 0 of the first chunk into buffer 0
  if (n_chunks > 0) {
    load_stg(it0, 0);
    drain(0, 0, 0);
  }
  __syncthreads();  // lists, thresholds, qc words and buffer 0 are ready

  const int mylist = wave * TW_QPW + lq;
  float* tvu = topv + mylist * KP;
  int* tiu = topi + mylist * KP;
  int buf = 0;
  for (int ci = 0; ci < n_chunks; ++ci) {
    const long long base = it0 + (long long)ci * cstep;
    const bool more = ci + 1 < n_chunks;
    // fold the cross-slice threshold into the local one every 8 chunks.
    // th_lds[ml] is written and read by this wave alone, so program order
    // is all the ordering it needs.
    if (th_g != nullptr && (ci & 7) == 0 && lg == 0) {
      if (has_user) {
        const float gv = tw_dec(gth_pipe);
        if (gv > th_lds[mylist]) th_lds[mylist] = gv;
        gth_pipe = th_g[guser];
      }
    }

    f32x4 acc[IFR];
#pragma unroll
    for (int i = 0; i < IFR; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      constexpr int LASTP = NP - 1;
      // next panel's loads first, so they fly under this panel's MFMAs
      if (p < LASTP) load_stg(base, p + 1);
      else if (more) load_stg(base + cstep, 0);

      const char* yb = ys + buf * TW_PANEL_BYTES;
#pragma unroll
      for (int ks = 0; ks < KSP; ++ks) {
#pragma unroll
        for (int i = 0; i < IFR; ++i) {
          const int row = i * 16 + lq;           // A operand row = item
          const int col = ks * 64 + lg * 16;     // byte offset of k-slice
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(
              yb + row * TW_ROWB + (col ^ ((row & 7) << 4)));
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, xf[p * KSP + ks], acc[i], 0, 0, 0);
        }
      }

      if (p < LASTP) drain(buf ^ 1, p + 1, ci & 1);
      else if (more) drain(buf ^ 1, 0, (ci + 1) & 1);

      if (p == LASTP) {
        const unsigned* cats_c = cats_lds + (ci & 1) * CW * CSTR;
        const float* wts_c = wts_lds + (ci & 1) * TW_CHUNK;
        // ---- item weights, ahead of the category select: -FLT_MAX times
        // a negative weight would be a huge positive score
        if constexpr (WT) {
#pragma unroll
          for (int i = 0; i < IFR; ++i) {
            const f32x4 w =
                *reinterpret_cast<const f32x4*>(&wts_c[i * 16 + lg * 4]);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][r] = acc[i][r] * w[r] + 0.0f;
          }
        }
        // ---- category filter, ahead of the threshold test
        if constexpr (CW > 0) {
#pragma unroll
          for (int i = 0; i < IFR; ++i) {
            u32x4 hit = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int w = 0; w < CW; ++w) {
              const u32x4 c = *reinterpret_cast<const u32x4*>(
                  &cats_c[w * CSTR + i * 16 + lg * 4]);
              hit |= c & qc_lds[w * TW_UPB + mylist];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
              acc[i][r] = hit[r] != 0u ? acc[i][r] : -FLT_MAX;
          }
        }

        // ---- common case: one max-reduce + one threshold read
        float mymax = -FLT_MAX;
#pragma unroll
        for (int i = 0; i < IFR; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) mymax = fmaxf(mymax, acc[i][r]);
        const float th_b = th_lds[mylist];
        if (has_user && mymax > th_b) {
          // the query's 4 lane groups take turns. A runtime loop with an
          // opaque barrier per iteration: unrolled, the four identical
          // blocks are tail-merged into one exec-masked block and all
          // groups read the threshold before any insert.
#pragma unroll 1
          for (int g = 0; g < 4; ++g) {
            asm volatile("" ::: "memory");  // keep iterations distinct
            if (lg == g) {
              float th = th_lds[mylist];
              const int lim =
                  (int)(it1 - base < TW_CHUNK ? it1 - base : TW_CHUNK);
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
                         ((unsigned)((unsigned)gitem * 2654435761u) >> 26)) &
                            1;
                    if ((item_mask == nullptr || !item_mask[item]) &&
                        (!may_ban || !in_sorted(ban, bn, gitem))) {
                      int mi = 0;
                      float mv = tvu[0];
                      for (int q = 1; q < K; ++q)
                        if (tvu[q] < mv) { mv = tvu[q]; mi = q; }
                      tvu[mi] = s;
                      tiu[mi] = gitem;
                      float nm = tvu[0];
                      for (int q = 1; q < K; ++q) nm = fminf(nm, tvu[q]);
                      th = nm;
                      th_lds[mylist] = nm;
                      // publish to the other slices once the list is full
                      if (th_g != nullptr && nm > -FLT_MAX &&
                          tw_enc(nm) > th_g[guser])
                        atomicMax(&th_g[guser], tw_enc(nm));
                    }
                  }
                }
              }
            }
          }
        }
      }
      __syncthreads();  // the one barrier of the panel step
      buf ^= 1;
    }
  }

  // ---- write out: one candidate group per slice per query
  for (int e = tid; e < TW_UPB * K; e += TW_BS) {
    const int list = e / K;
    const int q = e % K;
    const long long gu = u0 + list;
    if (gu < B) {
      const long long o = (gu * n_slices + slice) * (long long)K + q;
      out_val[o] = topv[list * KP + q];
      out_idx[o] = topi[list * KP + q];
    }
  }
}

// args = the kernel's arguments, in order
template <int NP, int CW, bool ILV, bool WT, typename... Args>
static void launch(dim3 grid, int K, hipStream_t stream, Args... args) {
  launch_dyn_lds<topk_mfma_wide_kernel<NP, CW, ILV, WT>>(
      grid, dim3(TW_BS), tw_lds_bytes(NP, K, CW, WT), stream, args...);
}

template <int NP, int CW, typename... Args>
static void launch_cw(bool ilv, bool wt, Args... args) {
  if (ilv) {
    if (wt) launch<NP, CW, true, true>(args...);
    else launch<NP, CW, true, false>(args...);
  } else {
    if (wt) launch<NP, CW, false, true>(args...);
    else launch<NP, CW, false, false>(args...);
  }
}

template <int NP, typename... Args>
static void launch_np(int cw, Args... args) {
  switch (cw) {
    case 0: launch_cw<NP, 0>(args...); break;
    case 1: launch_cw<NP, 1>(args...); break;
    case 2: launch_cw<NP, 2>(args...); break;
    case 4: launch_cw<NP, 4>(args...); break;
    default: break;
  }
}

// f = 256, 384 or 512 (the binding checks); item_weights: nullptr =
// unweighted; th_g: nullptr = no cross-slice threshold
extern "C" void launch_topk_mfma_wide(
    const unsigned short* Xq, const unsigned short* Y,
    const uint8_t* item_mask, const long long* ban_indptr,
    const int* ban_indices, float* out_val, int* out_idx,
    int B, long long N, int f, int K, int n_slices, int item_base,
    unsigned* th_g, const int* item_cats, const int* query_cats, int cw,
    int interleave, const float* item_weights, hipStream_t stream)
{
  const dim3 grid((B + TW_UPB - 1) / TW_UPB, n_slices);
  const char* e_bl = getenv("PIO_TOPK_BLOOM");
  const int kflags = (e_bl != nullptr && e_bl[0] == '0') ? 1 : 0;
  auto go = [&](auto np) {
    launch_np<decltype(np)::value>(
        cw, interleave != 0, item_weights != nullptr, grid, K, stream, Xq, Y,
        item_mask, ban_indptr, ban_indices, out_val, out_idx, B, N, K,
        n_slices, item_base, th_g, kflags, item_cats, query_cats,
        item_weights);
  };
  switch (f) {
    case 256: go(std::integral_constant<int, 2>{}); break;
    case 384: go(std::integral_constant<int, 3>{}); break;
    case 512: go(std::integral_constant<int, 4>{}); break;
    default: break;
  }
}
