// Exact fp32 re-score of a top-K shortlist for MI355X (gfx950, CDNA4).
//
//   out[b, c] = dot(Xq[b, :], Y[idx[b, c], :])      idx [B, C] int32
//
// The union path for K > 64 (ops/topk.py) shortlists C = 2K candidates
// per query on their bf16 scores and needs their exact fp32 dots. Doing
// that as a gather Y[idx] plus an einsum materializes a B x C x f fp32
// intermediate (2 GB at B = 4096, K = 1024, f = 64); this kernel reads
// the rows where they lie.
//
// One 16-lane group per candidate, four candidates per wave. With VEC
// each lane loads float4s (a 64-float row is one 256 B request per
// group); otherwise lanes stride the row one float at a time — template
// ranks are arbitrary (the default is 10) and views need not be 16 B
// aligned. The partial sums meet in a 4-step cross-lane butterfly; no
// LDS. idx < 0 (an empty slot) gives -inf. The indices are trusted: the
// binding checks idx < N before the launch.

#include <hip/hip_runtime.h>
#include <math.h>

#define RS_BS 256   // threads per block
#define RS_GROUP 16 // lanes per candidate

template <bool VEC>
__global__ __launch_bounds__(RS_BS)
void topk_rescore_kernel(
    const float* __restrict__ Xq,   // B x f
    const float* __restrict__ Y,    // N x f
    const int* __restrict__ idx,    // B x C
    float* __restrict__ out,        // B x C
    long long total,                // B * C
    int C, int f)
{
  const long long cand =
      ((long long)blockIdx.x * RS_BS + threadIdx.x) / RS_GROUP;
  const int sub = threadIdx.x & (RS_GROUP - 1);
  const bool live = cand < total;
  const int j = live ? idx[cand] : -1;
  float acc = 0.f;
  if (j >= 0) {
    const float* x = Xq + (cand / C) * (long long)f;
    const float* y = Y + (long long)j * f;
    if constexpr (VEC) {
      for (int k = sub * 4; k < f; k += RS_GROUP * 4) {
        const float4 a = *reinterpret_cast<const float4*>(x + k);
        const float4 b = *reinterpret_cast<const float4*>(y + k);
        acc = fmaf(a.x, b.x, acc);
        acc = fmaf(a.y, b.y, acc);
        acc = fmaf(a.z, b.z, acc);
        acc = fmaf(a.w, b.w, acc);
      }
    } else {
      for (int k = sub; k < f; k += RS_GROUP) acc = fmaf(x[k], y[k], acc);
    }
  }
  // every lane of the wave takes part, live or not
#pragma unroll
  for (int o = RS_GROUP / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (live && sub == 0) out[cand] = j >= 0 ? acc : -INFINITY;
}

extern "C" void launch_topk_rescore(
    const float* Xq, const float* Y, const int* idx, float* out,
    long long B, int C, int f, hipStream_t stream)
{
  const long long total = B * C;
  if (total == 0) return;
  const long long blocks = (total * RS_GROUP + RS_BS - 1) / RS_BS;
  const bool vec = f % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(Xq) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(Y) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(topk_rescore_kernel<true>, dim3((unsigned)blocks),
                       dim3(RS_BS), 0, stream, Xq, Y, idx, out, total, C, f);
  else
    hipLaunchKernelGGL(topk_rescore_kernel<false>, dim3((unsigned)blocks),
                       dim3(RS_BS), 0, stream, Xq, Y, idx, out, total, C, f);
}
