// PyTorch bindings for the MI355X HIP kernel library.
//
// Compiled natively with hipcc against libtorch's ROCm build (no hipify,
// no CUDA shims — the kernels are written directly for gfx950).

#include <torch/extension.h>

#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

extern "C" void launch_als_solve(
    const long long* indptr, const int* indices, const float* values,
    const float* Y, const float* YtY, const float* V, float* X,
    int n_rows, int f, float lambda, float alpha,
    int implicit_mode, int wr_scale, int which,
    unsigned long long* prof, hipStream_t stream);

extern "C" void launch_als_row_transform(
    const float* in, const float* W, float* out, long long n_rows, int f,
    int n_cu, hipStream_t stream);

extern "C" void launch_topk_score(
    const float* Xq, const float* Y, const uint8_t* item_mask,
    const long long* ban_indptr, const int* ban_indices,
    float* out_val, int* out_idx,
    int B, long long N, int f, int K, int n_slices, int item_base,
    unsigned long long* prof,
    const int* item_cats, const int* query_cats, int cw,
    hipStream_t stream);

extern "C" void launch_topk_mfma(
    const unsigned short* Xq, const unsigned short* Y,
    const uint8_t* item_mask, const long long* ban_indptr,
    const int* ban_indices, float* out_val, int* out_idx,
    int B, long long N, int f, int K, int n_slices, int item_base,
    unsigned long long* prof, unsigned* th_g,
    const int* item_cats, const int* query_cats, int cw, int interleave,
    hipStream_t stream);

extern "C" void launch_topk_rescore(
    const float* Xq, const float* Y, const int* idx, float* out,
    long long B, int C, int f, hipStream_t stream);

extern "C" int als_loss_grid(long long n_rows, int n_cu);

extern "C" void launch_als_loss(
    const long long* indptr, const int* indices, const float* values,
    const float* X, const float* Y, float* pred, double* partials,
    long long n_rows, int f, double alpha, int implicit_mode, int grid,
    hipStream_t stream);

extern "C" void launch_cooc_topn(
    const long long* u_indptr, const int* u_items, const long long* i_indptr,
    const int* i_users, const int* rows, int n_rows, int n, int tier,
    int* pool, long long n_items, int* top_ids, int* top_cnt, int grid,
    hipStream_t stream);

extern "C" int cooc_dense_lds_max();

namespace {

void check_cuda_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
}

bool supported_rank(int64_t f) {
  return f == 16 || f == 32 || f == 64 || f == 128;
}

// Optional per-query category filter: item_cats [N, W] and query_cats
// [B, W] int32 bit words, W in {1, 2, 4}, given together or not at all.
// Returns W (0 = no filter); any mismatch raises.
int check_cats(const c10::optional<torch::Tensor>& item_cats,
               const c10::optional<torch::Tensor>& query_cats,
               int64_t B, int64_t N, bool has_prof) {
  TORCH_CHECK(item_cats.has_value() == query_cats.has_value(),
              "item_cats and query_cats must be given together");
  if (!item_cats.has_value()) return 0;
  TORCH_CHECK(!has_prof, "prof cannot be combined with category filters");
  TORCH_CHECK(item_cats->is_cuda() && item_cats->is_contiguous() &&
                  item_cats->scalar_type() == torch::kInt32 &&
                  item_cats->dim() == 2,
              "item_cats must be a contiguous [N, W] i32 GPU tensor");
  TORCH_CHECK(query_cats->is_cuda() && query_cats->is_contiguous() &&
                  query_cats->scalar_type() == torch::kInt32 &&
                  query_cats->dim() == 2,
              "query_cats must be a contiguous [B, W] i32 GPU tensor");
  const int64_t W = item_cats->size(1);
  TORCH_CHECK(W == 1 || W == 2 || W == 4,
              "category words W must be 1, 2 or 4, got ", W);
  TORCH_CHECK(item_cats->size(0) == N, "item_cats must have N rows");
  TORCH_CHECK(query_cats->size(0) == B && query_cats->size(1) == W,
              "query_cats must be [B, W] with item_cats' W");
  return (int)W;
}

// The arguments topk_score and topk_score_mfma share, validated against
// the batch B and item count N and reduced to the raw pointers the
// launchers take (nullptr = not given; cw = 0 = no category filter).
struct TopkArgs {
  const uint8_t* mask = nullptr;
  const long long* ban_indptr = nullptr;
  const int* ban_indices = nullptr;
  unsigned long long* prof = nullptr;
  const int* item_cats = nullptr;
  const int* query_cats = nullptr;
  int cw = 0;
};

TopkArgs check_topk_args(const c10::optional<torch::Tensor>& item_mask,
                         const c10::optional<torch::Tensor>& ban_indptr,
                         const c10::optional<torch::Tensor>& ban_indices,
                         const c10::optional<torch::Tensor>& prof,
                         const c10::optional<torch::Tensor>& item_cats,
                         const c10::optional<torch::Tensor>& query_cats,
                         int64_t B, int64_t N) {
  TopkArgs a;
  a.cw = check_cats(item_cats, query_cats, B, N, prof.has_value());
  if (a.cw) {
    a.item_cats = item_cats->data_ptr<int>();
    a.query_cats = query_cats->data_ptr<int>();
  }
  if (item_mask.has_value()) {
    TORCH_CHECK(item_mask->is_cuda() && item_mask->is_contiguous() &&
                    item_mask->scalar_type() == torch::kUInt8,
                "item_mask must be contiguous u8 GPU");
    TORCH_CHECK(item_mask->size(0) == N, "item_mask size mismatch");
    a.mask = item_mask->data_ptr<uint8_t>();
  }
  if (ban_indptr.has_value()) {
    TORCH_CHECK(ban_indices.has_value(), "ban_indices required with ban_indptr");
    TORCH_CHECK(ban_indptr->is_cuda() && ban_indptr->is_contiguous() &&
                ban_indptr->scalar_type() == torch::kInt64);
    TORCH_CHECK(ban_indices->is_cuda() && ban_indices->is_contiguous() &&
                ban_indices->scalar_type() == torch::kInt32);
    TORCH_CHECK(ban_indptr->size(0) == B + 1, "ban_indptr must be B+1");
    a.ban_indptr = reinterpret_cast<const long long*>(
        ban_indptr->data_ptr<int64_t>());
    a.ban_indices = ban_indices->data_ptr<int>();
  }
  if (prof.has_value()) {
    TORCH_CHECK(prof->is_cuda() && prof->is_contiguous() &&
                    prof->scalar_type() == torch::kUInt64 &&
                    prof->numel() >= 5,
                "prof must be a contiguous u64[5] GPU tensor");
    a.prof = reinterpret_cast<unsigned long long*>(
        prof->data_ptr<uint64_t>());
  }
  return a;
}

// Solve one ALS half-iteration: for every CSR row r,
//   explicit: (sum_i y_i y_i^T + lambda*nnz_r*I) x_r = sum_i r_i y_i
//   implicit: (YtY + sum_i alpha*r * y_i y_i^T + lambda*I) x_r
//               = sum_i (1+alpha*r) y_i
// V = Y L^-T (L = chol(YtY + lambda I)) precomputed on the host per
// half-iteration enables the per-row Woodbury fast path in implicit mode
// (see als_woodbury_kernel). which: 0 = both passes, 1 = Woodbury rows
// only (emits Z), 2 = dense rows only (writes into `out`).
torch::Tensor als_solve(torch::Tensor indptr, torch::Tensor indices,
                        torch::Tensor values, torch::Tensor Y,
                        c10::optional<torch::Tensor> YtY,
                        c10::optional<torch::Tensor> V,
                        double lambda, double alpha,
                        bool implicit_mode, bool wr_scale,
                        int64_t which, c10::optional<torch::Tensor> out,
                        c10::optional<torch::Tensor> prof) {
  TORCH_CHECK(indptr.is_cuda() && indptr.scalar_type() == torch::kInt64 &&
                  indptr.is_contiguous(), "indptr must be contiguous i64 GPU");
  TORCH_CHECK(indices.is_cuda() && indices.scalar_type() == torch::kInt32 &&
                  indices.is_contiguous(), "indices must be contiguous i32 GPU");
  check_cuda_f32(values, "values");
  check_cuda_f32(Y, "Y");
  const int64_t f = Y.size(1);
  TORCH_CHECK(supported_rank(f), "rank must be one of 16/32/64/128, got ", f);
  const int64_t n_rows = indptr.size(0) - 1;
  TORCH_CHECK(indices.size(0) == values.size(0), "indices/values mismatch");
  const float* yty_ptr = nullptr;
  if (YtY.has_value()) {
    check_cuda_f32(*YtY, "YtY");
    TORCH_CHECK(YtY->size(0) == f && YtY->size(1) == f, "YtY must be f x f");
    yty_ptr = YtY->data_ptr<float>();
  }
  const float* v_ptr = nullptr;
  if (V.has_value()) {
    // V may be bf16 when PIO_ALS_STAGE_BF16 is set (the kernel stages
    // it as bf16; the pointer is reinterpreted device-side)
    TORCH_CHECK(V->is_cuda() && V->is_contiguous() &&
                    (V->scalar_type() == torch::kFloat32 ||
                     V->scalar_type() == torch::kBFloat16),
                "V must be contiguous fp32/bf16 GPU");
    TORCH_CHECK(V->sizes() == Y.sizes(), "V must match Y shape");
    const bool env_bf16 = [] {
      const char* e = getenv("PIO_ALS_STAGE_BF16");
      return e != nullptr && e[0] == '1';
    }();
    TORCH_CHECK((V->scalar_type() == torch::kBFloat16) == env_bf16,
                "V dtype must match PIO_ALS_STAGE_BF16");
    v_ptr = reinterpret_cast<const float*>(V->data_ptr());
  }
  unsigned long long* prof_ptr = nullptr;
  if (prof.has_value()) {
    TORCH_CHECK(prof->is_cuda() && prof->is_contiguous() &&
                prof->scalar_type() == torch::kUInt64 &&
                prof->numel() >= 5,
                "prof must be a contiguous u64 GPU tensor of >= 5");
    prof_ptr = reinterpret_cast<unsigned long long*>(
        prof->data_ptr());
  }
  torch::Tensor X;
  if (out.has_value()) {
    check_cuda_f32(*out, "out");
    TORCH_CHECK(out->size(0) == n_rows && out->size(1) == f,
                "out must be n_rows x f");
    X = *out;
  } else {
    X = torch::empty({n_rows, f}, Y.options());
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Y.device());
  hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_als_solve(reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>()), indices.data_ptr<int>(),
                   values.data_ptr<float>(), Y.data_ptr<float>(), yty_ptr,
                   v_ptr, X.data_ptr<float>(), (int)n_rows, (int)f, (float)lambda,
                   (float)alpha, implicit_mode ? 1 : 0, wr_scale ? 1 : 0,
                   (int)which, prof_ptr, stream);
  C10_HIP_CHECK(hipGetLastError());
  return X;
}

// out[N, f] = in[N, f] . W[f, f] in exact fp32 on the matrix pipe (see
// als_xform.hip): the whitening V = Y L^-T and the map back X = Z L^-1.
// `out` may be a row slice of a larger buffer, or `in` itself.
torch::Tensor als_row_transform(torch::Tensor in, torch::Tensor W,
                                c10::optional<torch::Tensor> out) {
  check_cuda_f32(in, "in");
  check_cuda_f32(W, "W");
  TORCH_CHECK(in.dim() == 2 && W.dim() == 2, "in and W must be 2-D");
  const int64_t n_rows = in.size(0);
  const int64_t f = in.size(1);
  TORCH_CHECK(supported_rank(f), "rank must be one of 16/32/64/128, got ", f);
  TORCH_CHECK(W.size(0) == f && W.size(1) == f, "W must be f x f");
  TORCH_CHECK(W.device() == in.device(), "W must be on in's device");
  torch::Tensor X;
  if (out.has_value()) {
    check_cuda_f32(*out, "out");
    TORCH_CHECK(out->dim() == 2 && out->size(0) == n_rows &&
                    out->size(1) == f, "out must be n_rows x f");
    TORCH_CHECK(out->device() == in.device(), "out must be on in's device");
    X = *out;
  } else {
    X = torch::empty({n_rows, f}, in.options());
  }
  if (n_rows == 0) return X;
  // the kernel moves rows in 16-byte quads
  TORCH_CHECK(reinterpret_cast<uintptr_t>(in.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(X.data_ptr()) % 16 == 0,
              "in/out must be 16-byte aligned");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(in.device());
  hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int n_cu = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  launch_als_row_transform(in.data_ptr<float>(), W.data_ptr<float>(),
                           X.data_ptr<float>(), (long long)n_rows, (int)f,
                           n_cu, stream);
  C10_HIP_CHECK(hipGetLastError());
  return X;
}

// The two sums over stored ratings that the ALS objective needs (see
// als_loss.hip): with s = dot(X[u], Y[indices[p]]),
//   [A, B] = [sum w (t - s)^2, sum s^2]
//   explicit: (w, t) = (1, r)      implicit: (w, t) = (1 + alpha r, 1)
// as a float64 [2] device tensor; no host sync. X holds the CSR's rows,
// Y the columns' factors; any rank 1 <= f <= 128, unpadded. pred, if
// given, receives s per rating. Column ids are trusted (ops/als.py
// range-checks them first).
torch::Tensor als_residual_sums(torch::Tensor indptr, torch::Tensor indices,
                                torch::Tensor values, torch::Tensor X,
                                torch::Tensor Y, double alpha,
                                bool implicit_mode,
                                c10::optional<torch::Tensor> pred) {
  TORCH_CHECK(indptr.is_cuda() && indptr.scalar_type() == torch::kInt64 &&
                  indptr.is_contiguous() && indptr.dim() == 1 &&
                  indptr.size(0) >= 1,
              "indptr must be a contiguous 1-D i64 GPU tensor");
  TORCH_CHECK(indices.is_cuda() && indices.scalar_type() == torch::kInt32 &&
                  indices.is_contiguous() && indices.dim() == 1,
              "indices must be a contiguous 1-D i32 GPU tensor");
  check_cuda_f32(values, "values");
  check_cuda_f32(X, "X");
  check_cuda_f32(Y, "Y");
  TORCH_CHECK(values.dim() == 1 && X.dim() == 2 && Y.dim() == 2,
              "values must be 1-D, X and Y 2-D");
  TORCH_CHECK(indices.device() == X.device() && indptr.device() == X.device() &&
                  values.device() == X.device() && Y.device() == X.device(),
              "all tensors must be on one device");
  const int64_t n_rows = indptr.size(0) - 1;
  const int64_t nnz = indices.size(0);
  const int64_t f = X.size(1);
  TORCH_CHECK(X.size(0) == n_rows, "X must have one row per CSR row");
  TORCH_CHECK(Y.size(1) == f, "X/Y rank mismatch");
  TORCH_CHECK(f >= 1 && f <= 128, "rank must be in [1, 128], got ", f);
  TORCH_CHECK(values.size(0) == nnz, "indices/values mismatch");
  float* pred_ptr = nullptr;
  if (pred.has_value()) {
    check_cuda_f32(*pred, "pred");
    TORCH_CHECK(pred->dim() == 1 && pred->size(0) == nnz &&
                    pred->device() == X.device(),
                "pred must be [nnz] on X's device");
    pred_ptr = pred->data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  const auto f64 = X.options().dtype(torch::kFloat64);
  if (n_rows == 0 || nnz == 0) return torch::zeros({2}, f64);
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int n_cu = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int grid = als_loss_grid((long long)n_rows, n_cu);
  auto partials = torch::empty({grid, 2}, f64);  // every block writes its row
  launch_als_loss(
      reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>()),
      indices.data_ptr<int>(), values.data_ptr<float>(), X.data_ptr<float>(),
      Y.data_ptr<float>(), pred_ptr, partials.data_ptr<double>(),
      (long long)n_rows, (int)f, alpha, implicit_mode ? 1 : 0, grid, stream);
  C10_HIP_CHECK(hipGetLastError());
  return partials.sum(0);
}

// Fused masked top-K scoring: per-slice candidate groups; caller merges
// with a small torch.topk. Returns (vals [B, n_slices*4*K], idx i32).
std::tuple<torch::Tensor, torch::Tensor> topk_score(
    torch::Tensor Xq, torch::Tensor Y, int64_t K, int64_t n_slices,
    c10::optional<torch::Tensor> item_mask,
    c10::optional<torch::Tensor> ban_indptr,
    c10::optional<torch::Tensor> ban_indices, int64_t item_base,
    c10::optional<torch::Tensor> prof,
    c10::optional<torch::Tensor> item_cats,
    c10::optional<torch::Tensor> query_cats) {
  check_cuda_f32(Xq, "Xq");
  check_cuda_f32(Y, "Y");
  const int64_t f = Y.size(1);
  TORCH_CHECK(supported_rank(f), "rank must be one of 16/32/64/128, got ", f);
  TORCH_CHECK(Xq.size(1) == f, "Xq/Y rank mismatch");
  TORCH_CHECK(K >= 1 && K <= 64, "K must be in [1, 64]");
  const int64_t B = Xq.size(0);
  const int64_t N = Y.size(0);
  TORCH_CHECK(n_slices >= 1);
  const TopkArgs a = check_topk_args(item_mask, ban_indptr, ban_indices, prof,
                                     item_cats, query_cats, B, N);
  // the kernel emits TK_WAVES=4 independent candidate groups per slice
  auto out_val = torch::empty({B, n_slices * 4 * K}, Xq.options());
  auto out_idx = torch::empty({B, n_slices * 4 * K},
                              Xq.options().dtype(torch::kInt32));
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Y.device());
  hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_topk_score(Xq.data_ptr<float>(), Y.data_ptr<float>(), a.mask,
                    a.ban_indptr, a.ban_indices, out_val.data_ptr<float>(),
                    out_idx.data_ptr<int>(), (int)B, (long long)N, (int)f,
                    (int)K, (int)n_slices, (int)item_base, a.prof,
                    a.item_cats, a.query_cats, a.cw, stream);
  C10_HIP_CHECK(hipGetLastError());
  return {out_val, out_idx};
}

// MFMA variant of topk_score: bf16 query/item factors (fp32 accumulate on
// the matrix cores). Output is n_slices candidate groups of K per query
// (topk_score emits n_slices*4); the Python wrapper merges and
// fp32-rescores. K is the per-slice list length. interleave = true deals
// the 64-item chunks round-robin to the slices (slice s takes chunks s,
// s + n_slices, ...) instead of one contiguous run each. gth: None keeps
// the PIO_TOPK_GTH default, false launches without the cross-slice
// threshold — it prunes to the top K overall, so a caller that wants
// every slice's own top K (the union path) must turn it off.
std::tuple<torch::Tensor, torch::Tensor> topk_score_mfma(
    torch::Tensor Xq, torch::Tensor Y, int64_t K, int64_t n_slices,
    c10::optional<torch::Tensor> item_mask,
    c10::optional<torch::Tensor> ban_indptr,
    c10::optional<torch::Tensor> ban_indices, int64_t item_base,
    c10::optional<torch::Tensor> prof,
    c10::optional<torch::Tensor> item_cats,
    c10::optional<torch::Tensor> query_cats, bool interleave,
    c10::optional<bool> gth_opt) {
  TORCH_CHECK(Xq.is_cuda() && Xq.is_contiguous() &&
                  Xq.scalar_type() == torch::kBFloat16,
              "Xq must be contiguous bf16 GPU");
  TORCH_CHECK(Y.is_cuda() && Y.is_contiguous() &&
                  Y.scalar_type() == torch::kBFloat16,
              "Y must be contiguous bf16 GPU");
  const int64_t f = Y.size(1);
  TORCH_CHECK(f == 32 || f == 64 || f == 128,
              "mfma rank must be one of 32/64/128, got ", f);
  TORCH_CHECK(Xq.size(1) == f, "Xq/Y rank mismatch");
  TORCH_CHECK(K >= 1 && K <= 64, "K must be in [1, 64]");
  const int64_t B = Xq.size(0);
  const int64_t N = Y.size(0);
  TORCH_CHECK(n_slices >= 1);
  TORCH_CHECK(!(interleave && prof.has_value()),
              "prof cannot be combined with interleave");
  const TopkArgs a = check_topk_args(item_mask, ban_indptr, ban_indices, prof,
                                     item_cats, query_cats, B, N);
  // one candidate group per slice per query (the kernel keeps a single
  // shared top-K list per query per workgroup)
  auto out_val = torch::empty({B, n_slices * K},
                              Xq.options().dtype(torch::kFloat32));
  auto out_idx = torch::empty({B, n_slices * K},
                              Xq.options().dtype(torch::kInt32));
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Y.device());
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  // cross-slice threshold exchange (default ON; PIO_TOPK_GTH=0
  // disables): a [B] tm_enc-coded atomicMax cell per query, zero-init
  // (= below every real score), shared by all of a query's slice WGs
  // through L2. +17-29% for B in [64, 4096]; the kernel's
  // test-and-test-and-set read keeps the atomic queue short (the
  // unfiltered version serialized at small B —
  // profiles/serve_gth_ab_r2.log).
  torch::Tensor th_g;
  unsigned* th_g_ptr = nullptr;
  const char* e_gth = getenv("PIO_TOPK_GTH");
  const bool gth = gth_opt.has_value()
      ? *gth_opt : !(e_gth != nullptr && e_gth[0] == '0');
  if (gth) {
    th_g = torch::zeros({B}, Xq.options().dtype(torch::kInt32));
    th_g_ptr = reinterpret_cast<unsigned*>(th_g.data_ptr<int>());
  }
  launch_topk_mfma(
      reinterpret_cast<const unsigned short*>(Xq.data_ptr()),
      reinterpret_cast<const unsigned short*>(Y.data_ptr()), a.mask,
      a.ban_indptr, a.ban_indices, out_val.data_ptr<float>(),
      out_idx.data_ptr<int>(), (int)B, (long long)N, (int)f, (int)K,
      (int)n_slices, (int)item_base, a.prof, th_g_ptr, a.item_cats,
      a.query_cats, a.cw, interleave ? 1 : 0, stream);
  C10_HIP_CHECK(hipGetLastError());
  return {out_val, out_idx};
}

// out[b, c] = dot(Xq[b, :], Y[idx[b, c], :]) in fp32; idx < 0 gives -inf.
// Any rank: rows move as float4 when f % 4 == 0 and both base pointers
// are 16-byte aligned, as single floats otherwise. The kernel trusts
// idx, so the upper bound is checked here (one small reduction).
torch::Tensor topk_rescore(torch::Tensor Xq, torch::Tensor Y,
                           torch::Tensor idx) {
  check_cuda_f32(Xq, "Xq");
  check_cuda_f32(Y, "Y");
  TORCH_CHECK(Xq.dim() == 2 && Y.dim() == 2 && idx.dim() == 2,
              "Xq, Y and idx must be 2-D");
  TORCH_CHECK(Xq.size(1) == Y.size(1), "Xq/Y rank mismatch");
  TORCH_CHECK(idx.is_cuda() && idx.is_contiguous() &&
                  idx.scalar_type() == torch::kInt32,
              "idx must be a contiguous i32 GPU tensor");
  TORCH_CHECK(Y.device() == Xq.device() && idx.device() == Xq.device(),
              "Xq, Y and idx must be on one device");
  const int64_t B = Xq.size(0);
  const int64_t C = idx.size(1);
  TORCH_CHECK(idx.size(0) == B, "idx must have one row per query");
  TORCH_CHECK(C < (1LL << 31) && B * C <= (1LL << 34),
              "too many candidates for one launch");
  auto out = torch::empty({B, C}, Xq.options());
  if (B * C == 0) return out;
  TORCH_CHECK(idx.max().item<int>() < Y.size(0),
              "idx holds an index >= the number of items");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Y.device());
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_topk_rescore(Xq.data_ptr<float>(), Y.data_ptr<float>(),
                      idx.data_ptr<int>(), out.data_ptr<float>(),
                      (long long)B, (int)C, (int)Xq.size(1), stream);
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

// One tier of co-occurrence top-N (see cooc_topn.hip): the item rows
// listed in `rows` are counted, selected and written to top_ids/top_cnt
// [N, n] in place; rows not listed are left alone. tier 0 / 1: the
// 1024- / 8192-slot LDS hash tables; tier 2: dense counters in `pool`,
// a zero [G, N] i32 tensor that is all zero again afterwards, one
// persistent workgroup per counter row; tier 3: dense counters in LDS,
// N <= cooc_dense_lds_max(). Ids are trusted
// (ops/cooccurrence.py range-checks both CSRs first).
void cooc_topn(torch::Tensor u_indptr, torch::Tensor u_items,
               torch::Tensor i_indptr, torch::Tensor i_users,
               torch::Tensor rows, int64_t n, int64_t tier,
               c10::optional<torch::Tensor> pool, torch::Tensor top_ids,
               torch::Tensor top_cnt) {
  auto check = [](const torch::Tensor& t, torch::ScalarType st, int64_t dim,
                  const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == st &&
                    t.dim() == dim,
                name, " must be a contiguous ", dim, "-D ",
                st == torch::kInt64 ? "i64" : "i32", " GPU tensor");
  };
  check(u_indptr, torch::kInt64, 1, "u_indptr");
  check(i_indptr, torch::kInt64, 1, "i_indptr");
  check(u_items, torch::kInt32, 1, "u_items");
  check(i_users, torch::kInt32, 1, "i_users");
  check(rows, torch::kInt32, 1, "rows");
  check(top_ids, torch::kInt32, 2, "top_ids");
  check(top_cnt, torch::kInt32, 2, "top_cnt");
  TORCH_CHECK(u_indptr.size(0) >= 1 && i_indptr.size(0) >= 1,
              "indptr tensors must not be empty");
  TORCH_CHECK(u_items.size(0) == i_users.size(0),
              "the two CSRs must hold the same pairs");
  TORCH_CHECK(n >= 1 && n <= 64, "n must be in [1, 64], got ", n);
  TORCH_CHECK(tier >= 0 && tier <= 3, "tier must be 0, 1, 2 or 3");
  const int64_t N = i_indptr.size(0) - 1;
  TORCH_CHECK(N < (1LL << 31) && u_indptr.size(0) - 1 < (1LL << 31),
              "item and user counts must be below 2^31");
  TORCH_CHECK(top_ids.size(0) == N && top_ids.size(1) == n &&
                  top_cnt.size(0) == N && top_cnt.size(1) == n,
              "top_ids and top_cnt must be [N, n]");
  const auto dev = u_indptr.device();
  TORCH_CHECK(u_items.device() == dev && i_indptr.device() == dev &&
                  i_users.device() == dev && rows.device() == dev &&
                  top_ids.device() == dev && top_cnt.device() == dev,
              "all tensors must be on one device");
  const int64_t n_rows = rows.size(0);
  TORCH_CHECK(n_rows < (1LL << 31), "too many rows for one launch");
  if (n_rows == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  const int n_cu = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  int64_t grid;
  int* pool_ptr = nullptr;
  if (tier == 2) {
    TORCH_CHECK(pool.has_value(), "the dense tier needs a counter pool");
    check(*pool, torch::kInt32, 2, "pool");
    TORCH_CHECK(pool->device() == dev && pool->size(0) >= 1 &&
                    pool->size(1) == N,
                "pool must be [G >= 1, N] on the inputs' device");
    grid = std::min<int64_t>(pool->size(0), n_rows);
    pool_ptr = pool->data_ptr<int>();
  } else if (tier == 3) {
    TORCH_CHECK(N <= cooc_dense_lds_max(), "the LDS dense tier holds at most ",
                cooc_dense_lds_max(), " items, got ", N);
    grid = std::min<int64_t>(n_rows, n_cu);  // 120 KB of LDS: one per CU
  } else {
    // LDS admits ten 16 KB / two 72 KB workgroups per CU
    grid = std::min<int64_t>(n_rows, (int64_t)n_cu * (tier == 0 ? 8 : 2));
  }
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_cooc_topn(
      reinterpret_cast<const long long*>(u_indptr.data_ptr<int64_t>()),
      u_items.data_ptr<int>(),
      reinterpret_cast<const long long*>(i_indptr.data_ptr<int64_t>()),
      i_users.data_ptr<int>(), rows.data_ptr<int>(), (int)n_rows, (int)n,
      (int)tier, pool_ptr, (long long)N, top_ids.data_ptr<int>(),
      top_cnt.data_ptr<int>(), (int)grid, stream);
  C10_HIP_CHECK(hipGetLastError());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X (gfx950) HIP kernels for predictionio_amd";
  m.def("als_solve", &als_solve, "Fused ALS Gramian+Cholesky half-iteration",
        py::arg("indptr"), py::arg("indices"), py::arg("values"),
        py::arg("Y"), py::arg("YtY") = py::none(), py::arg("V") = py::none(),
        py::arg("lambda_") = 0.01,
        py::arg("alpha") = 1.0, py::arg("implicit_mode") = false,
        py::arg("wr_scale") = true, py::arg("which") = 0,
        py::arg("out") = py::none(), py::arg("prof") = py::none());
  m.def("als_row_transform", &als_row_transform,
        "out[N, f] = in[N, f] . W[f, f], fp32 MFMA row transform",
        py::arg("in_"), py::arg("W"), py::arg("out") = py::none());
  m.def("als_residual_sums", &als_residual_sums,
        "[sum w (t - s)^2, sum s^2] over the stored ratings, float64",
        py::arg("indptr"), py::arg("indices"), py::arg("values"),
        py::arg("X"), py::arg("Y"), py::arg("alpha") = 1.0,
        py::arg("implicit_mode") = false, py::arg("pred") = py::none());
  m.def("topk_score", &topk_score, "Fused masked top-K scoring",
        py::arg("Xq"), py::arg("Y"), py::arg("K"), py::arg("n_slices") = 64,
        py::arg("item_mask") = py::none(), py::arg("ban_indptr") = py::none(),
        py::arg("ban_indices") = py::none(), py::arg("item_base") = 0,
        py::arg("prof") = py::none(), py::arg("item_cats") = py::none(),
        py::arg("query_cats") = py::none());
  m.def("topk_score_mfma", &topk_score_mfma,
        "Fused masked top-K scoring on MFMA (bf16 in, fp32 accumulate)",
        py::arg("Xq"), py::arg("Y"), py::arg("K"), py::arg("n_slices") = 64,
        py::arg("item_mask") = py::none(), py::arg("ban_indptr") = py::none(),
        py::arg("ban_indices") = py::none(), py::arg("item_base") = 0,
        py::arg("prof") = py::none(), py::arg("item_cats") = py::none(),
        py::arg("query_cats") = py::none(), py::arg("interleave") = false,
        py::arg("gth") = py::none());
  m.def("topk_rescore", &topk_rescore,
        "Exact fp32 dots of each query with its shortlisted items",
        py::arg("Xq"), py::arg("Y"), py::arg("idx"));
  m.def("cooc_topn", &cooc_topn,
        "Co-occurrence top-N of the listed item rows, one tier",
        py::arg("u_indptr"), py::arg("u_items"), py::arg("i_indptr"),
        py::arg("i_users"), py::arg("rows"), py::arg("n"), py::arg("tier"),
        py::arg("pool"), py::arg("top_ids"), py::arg("top_cnt"));
  m.def("cooc_dense_lds_max", &cooc_dense_lds_max,
        "Largest item count of the LDS dense tier");
}
