// Residual sums of the ALS objective for MI355X (gfx950, CDNA4).
//
//   s_ui = dot(X[u, :], Y[indices[p], :])        for every stored rating p
//   A    = sum_p w_p (t_p - s_p)^2               B = sum_p s_p^2
//   explicit: (w, t) = (1, r)                    implicit: (1 + alpha r, 1)
//
// This is the one part of the training objective that touches every
// rating; the regulariser and Gramian terms are f x f or row-norm work
// and stay in torch (ops/als.py). Doing it as a gather Y[indices] plus a
// row-wise product materializes an nnz x f fp32 intermediate (512 GB at
// 2 G ratings, f = 64); this kernel reads the rows where they lie — the
// gather stream of a half-step with none of its arithmetic.
//
// One wave per CSR row at a time, persistent waves grid-striding over
// the rows. The wave keeps x_u in registers for the whole row, laid out
// identically in each of its four 16-lane groups; group g takes ratings
// start + 4 it + g, so one group handles one rating: it gathers the item
// row, runs an fma chain into one fp32 partial per lane and finishes
// with a 4-step cross-lane butterfly. No LDS in the row loop. With VEC a
// lane moves float4s (a 64-float row is one 256 B request per group);
// otherwise lanes stride the row one float at a time — template ranks
// are arbitrary (the default is 10) and views need not be 16 B aligned.
//
// A gather's address hangs on its column id, so the ids (and ratings) of
// the NEXT loop trip are loaded before this trip's gathers are issued:
// a trip is two iterations, 8 gathers per wave in flight, none of them
// waiting on its own index fetch.
//
// From s on everything is fp64: each group's leader lane carries the two
// accumulators through the wave's whole grid-stride loop. The wave, then
// the block's four waves (through 8 LDS doubles), reduce in a fixed
// order and thread 0 stores partials[blockIdx.x][0..1] — no atomics, so
// for a given grid the result is bit-reproducible. The caller sums the
// partials. Column ids are trusted: the Python wrapper range-checks them
// before the launch.

#include <hip/hip_runtime.h>

#define AL_BS 256       // threads per block
#define AL_WAVES 4      // waves per block = rows per block pass
#define AL_GROUP 16     // lanes per rating
#define AL_WG_PER_CU 8  // persistent grid: 32 waves per CU, the wave cap
#define AL_RL 8         // floats of a row a lane holds (f <= 128)

// A lane's share of one factor row. VEC: the float4s at k = 4 sub and
// k = 64 + 4 sub; otherwise the floats at k = sub + 16 i. Past f: zeros.
template <bool VEC>
__device__ __forceinline__ void al_load_row(
    const float* __restrict__ p, int f, int sub, float (&v)[AL_RL])
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
    for (int i = 0; i < AL_RL; ++i) {
      const int k = sub + AL_GROUP * i;
      v[i] = k < f ? p[k] : 0.f;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(AL_BS)
void als_loss_kernel(
    const long long* __restrict__ indptr,  // n_rows + 1
    const int* __restrict__ indices,       // nnz
    const float* __restrict__ values,      // nnz
    const float* __restrict__ X,           // n_rows x f
    const float* __restrict__ Y,           // n_cols x f
    float* __restrict__ pred,              // nnz, or null
    double* __restrict__ partials,         // gridDim.x x 2
    long long n_rows, int f, double alpha, int implicit_mode)
{
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int g = lane >> 4;
  const int sub = lane & (AL_GROUP - 1);

  double acc_a = 0.0, acc_b = 0.0;  // live in the group leaders only

  const long long stride = (long long)gridDim.x * AL_WAVES;
  for (long long row = (long long)blockIdx.x * AL_WAVES + wave; row < n_rows;
       row += stride) {
    const long long start = indptr[row];
    const long long end = indptr[row + 1];
    if (start >= end) continue;  // wave-uniform

    float x[AL_RL];
    al_load_row<VEC>(X + row * f, f, sub, x);

    // column id (-1 = no rating) and value of rating q. Past the end the
    // row's last rating is read instead: unconditional loads let the
    // compiler count them, so a trip's gathers wait for its own ids
    // only, not for the next trip's (a branch around the load made it
    // wait for all but one).
    auto fetch = [&](long long q, int& j, float& r) {
      const bool live = q < end;
      const long long qc = live ? q : end - 1;
      const int jq = indices[qc];
      r = values[qc];
      j = live ? jq : -1;
    };
    auto gather = [&](int j, float (&y)[AL_RL]) {
      if (j >= 0) {
        al_load_row<VEC>(Y + (long long)j * f, f, sub, y);
      } else {
#pragma unroll
        for (int i = 0; i < AL_RL; ++i) y[i] = 0.f;
      }
    };
    auto dot = [&](const float (&y)[AL_RL]) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < AL_RL; ++i) s = fmaf(x[i], y[i], s);
      return s;
    };
    auto tally = [&](long long q, int j, float r, float s) {
      if (j < 0) return;
      const double sd = (double)s;
      const double t = implicit_mode ? 1.0 : (double)r;
      const double w = implicit_mode ? 1.0 + alpha * (double)r : 1.0;
      const double d = t - sd;
      acc_a += w * d * d;
      acc_b += sd * sd;
      if (pred != nullptr) pred[q] = s;
    };

    int j0, j1;
    float r0, r1;
    fetch(start + g, j0, r0);
    fetch(start + 4 + g, j1, r1);
    for (long long base = start; base < end; base += 8) {
      const long long q = base + g;
      // the next trip's ids go out ahead of this trip's gathers
      int jn0, jn1;
      float rn0, rn1;
      fetch(q + 8, jn0, rn0);
      fetch(q + 12, jn1, rn1);
      float y0[AL_RL], y1[AL_RL];
      gather(j0, y0);
      gather(j1, y1);
      float s0 = dot(y0);
      float s1 = dot(y1);
      // every lane of the wave takes part, rating or not
#pragma unroll
      for (int o = AL_GROUP / 2; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
      }
      if (sub == 0) {
        tally(q, j0, r0, s0);
        tally(q + 4, j1, r1, s1);
      }
      j0 = jn0; r0 = rn0;
      j1 = jn1; r1 = rn1;
    }
  }

  // the four leaders of a wave (the other lanes hold zeros), then the
  // four waves, in a fixed order
#pragma unroll
  for (int o = AL_GROUP; o < 64; o <<= 1) {
    acc_a += __shfl_xor(acc_a, o);
    acc_b += __shfl_xor(acc_b, o);
  }
  __shared__ double sm[AL_WAVES][2];
  if (lane == 0) {
    sm[wave][0] = acc_a;
    sm[wave][1] = acc_b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x + 0] =
        ((sm[0][0] + sm[1][0]) + sm[2][0]) + sm[3][0];
    partials[2 * blockIdx.x + 1] =
        ((sm[0][1] + sm[1][1]) + sm[2][1]) + sm[3][1];
  }
}

// Blocks of the persistent grid for n_rows rows: AL_WG_PER_CU per CU, or
// fewer when there is less work. The caller sizes `partials` by it.
extern "C" int als_loss_grid(long long n_rows, int n_cu)
{
  const long long want = (n_rows + AL_WAVES - 1) / AL_WAVES;
  const long long cap = (long long)(n_cu > 0 ? n_cu : 1) * AL_WG_PER_CU;
  const long long grid = want < cap ? want : cap;
  return (int)(grid > 0 ? grid : 1);
}

extern "C" void launch_als_loss(
    const long long* indptr, const int* indices, const float* values,
    const float* X, const float* Y, float* pred, double* partials,
    long long n_rows, int f, double alpha, int implicit_mode, int grid,
    hipStream_t stream)
{
  if (n_rows <= 0 || grid <= 0) return;
  const bool vec = f % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(X) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(Y) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(als_loss_kernel<true>, dim3((unsigned)grid),
                       dim3(AL_BS), 0, stream, indptr, indices, values, X, Y,
                       pred, partials, n_rows, f, alpha, implicit_mode);
  else
    hipLaunchKernelGGL(als_loss_kernel<false>, dim3((unsigned)grid),
                       dim3(AL_BS), 0, stream, indptr, indices, values, X, Y,
                       pred, partials, n_rows, f, alpha, implicit_mode);
}
