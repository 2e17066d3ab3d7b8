// PyTorch bindings for the MI355X HIP kernel library.
//
// Compiled natively with hipcc against libtorch's ROCm build (no hipify,
// no CUDA shims — the kernels are written directly for gfx950).

#include <torch/extension.h>

#include <climits>

#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

extern "C" void launch_als_solve(
    const long long* indptr, const int* indices, const float* values,
    const float* Y, const float* YtY, const float* V, float* X,
    int n_rows, int f, float lambda, float alpha,
    int implicit_mode, int wr_scale, int which,
    unsigned long long* prof, int heavy_min, hipStream_t stream);

extern "C" int als_wide_lds_bytes(int f);

extern "C" void launch_als_solve_wide(
    const long long* indptr, const int* indices, const float* values,
    const float* Y, const float* YtY, float* X, int n_rows, int f,
    float lambda, float alpha, int implicit_mode, int wr_scale,
    int skip_below, int skip_above, int grid, hipStream_t stream);

extern "C" long long als_heavy_slot_floats(int f);

extern "C" void launch_als_heavy(
    const long long* chunks, const long long* chunk_ptr,
    const long long* rows, const long long* chunk_ptr_host, int n_heavy,
    const int* indices, const float* values, const float* Y,
    const float* YtY, float* X, float* ws, long long ws_slots, float* carry,
    int f, float lambda, float alpha, int implicit_mode, int wr_scale,
    hipStream_t stream);

extern "C" int als_nnls_max_it();

extern "C" void launch_als_nnls(
    const long long* indptr, const int* indices, const float* values,
    const float* Y, const float* YtY, float* X, int* iters, int n_rows,
    int f, float lambda, float alpha, int implicit_mode, int wr_scale,
    int skip_above, hipStream_t stream);

extern "C" void launch_als_heavy_nnls(
    const long long* chunks, const long long* chunk_ptr,
    const long long* rows, const long long* chunk_ptr_host, int n_heavy,
    const int* indices, const float* values, const float* Y,
    const float* YtY, float* X, int* iters, float* ws, long long ws_slots,
    float* carry, int f, float lambda, float alpha, int implicit_mode,
    int wr_scale, hipStream_t stream);

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
    const float* item_weights, hipStream_t stream);

extern "C" void launch_topk_mfma(
    const unsigned short* Xq, const unsigned short* Y,
    const uint8_t* item_mask, const long long* ban_indptr,
    const int* ban_indices, float* out_val, int* out_idx,
    int B, long long N, int f, int K, int n_slices, int item_base,
    unsigned long long* prof, unsigned* th_g,
    const int* item_cats, const int* query_cats, int cw, int interleave,
    const float* item_weights, hipStream_t stream);

extern "C" void launch_topk_mfma_wide(
    const unsigned short* Xq, const unsigned short* Y,
    const uint8_t* item_mask, const long long* ban_indptr,
    const int* ban_indices, float* out_val, int* out_idx,
    int B, long long N, int f, int K, int n_slices, int item_base,
    unsigned* th_g, const int* item_cats, const int* query_cats, int cw,
    int interleave, const float* item_weights, hipStream_t stream);

extern "C" void launch_topk_rescore(
    const float* Xq, const float* Y, const int* idx, const float* w,
    float* out, long long B, int C, int f, hipStream_t stream);

extern "C" int als_loss_grid(long long n_rows, int n_cu);

extern "C" void launch_als_loss(
    const long long* indptr, const int* indices, const float* values,
    const float* X, const float* Y, float* pred, double* partials,
    long long n_rows, int f, double alpha, int implicit_mode, int grid,
    hipStream_t stream);

extern "C" void launch_cooc_topn(
    const long long* u_indptr, const int* u_items, const long long* i_indptr,
    const int* i_users, const int* rows, int n_rows, int n, int tier,
    int* pool, long long n_items, int* top_ids, void* top_val, int llr,
    int cross, const int* col_deg, const double* col_h, int n_users, int grid,
    hipStream_t stream);

extern "C" int cooc_dense_lds_max();

extern "C" void launch_topk_cand(
    const float* Xq, const float* Y, const int* cand, const long long* segs,
    int n_segs, const uint8_t* item_mask, const long long* ban_indptr,
    const int* ban_indices, const int* item_cats, const int* query_cats,
    const float* item_weights, int cw, int f, int K, int threads,
    float* out_val, int* out_idx, float* scores, int grid,
    hipStream_t stream);

extern "C" int indicator_topk_cap(int threads);

extern "C" void launch_indicator_topk(
    const int* top_ids, const void* top_sc, int n, const long long* q_indptr,
    const int* q_items, const int* work, int n_work, int max_items,
    const long long* ban_indptr, const int* ban_indices,
    const long long* allow_indptr, const int* allow_indices,
    const int* item_cats, const int* query_cats, int cw, int is_float,
    int exclude_own, int K, int threads, int n_cu, int* out_ids, void* out_sc,
    hipStream_t stream);

extern "C" int rank_count_tmax();
extern "C" int rank_count_group();
extern "C" int rank_stream_lds_bytes(int f);

extern "C" void launch_rank_list(
    const float* X, const float* Y, const int* slot_user, const int* slot_tgt,
    const long long* seen_indptr, const int* seen_indices, float* tscore,
    int* corr, int n_slots, int f, hipStream_t stream);

extern "C" void launch_rank_stream(
    const float* X, const float* Y, long long N, const int* slot_user,
    const float* tscore, int n_slots, int n_slices, int ties, int* partial,
    int f, hipStream_t stream);

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

// Per-item score weights of the top-K entries: a contiguous fp32 [N]
// tensor on the factors' device, or not given (nullptr). A mismatch
// raises ValueError; there is no fallback. With the phase probe the
// kernels have no weighted instantiation.
const float* check_item_weights(const c10::optional<torch::Tensor>& w,
                                const torch::Tensor& Y, bool prof) {
  if (!w.has_value()) return nullptr;
  TORCH_CHECK_VALUE(!prof, "prof cannot be combined with item_weights");
  TORCH_CHECK_VALUE(w->scalar_type() == torch::kFloat32,
                    "item_weights must be fp32");
  TORCH_CHECK_VALUE(w->dim() == 1 && w->size(0) == Y.size(0),
                    "item_weights must have shape [N]");
  TORCH_CHECK_VALUE(w->is_contiguous(), "item_weights must be contiguous");
  TORCH_CHECK_VALUE(w->is_cuda() && w->device() == Y.device(),
                    "item_weights must be on the device of Y");
  return w->data_ptr<float>();
}

// Solve one ALS half-iteration: for every CSR row r,
//   explicit: (sum_i y_i y_i^T + lambda*nnz_r*I) x_r = sum_i r_i y_i
//   implicit: (YtY + sum_i alpha*r * y_i y_i^T + lambda*I) x_r
//               = sum_i (1+alpha*r) y_i
// V = Y L^-T (L = chol(YtY + lambda I)) precomputed on the host per
// half-iteration enables the per-row Woodbury fast path in implicit mode
// (see als_woodbury_kernel). which: 0 = both passes, 1 = Woodbury rows
// only (emits Z), 2 = dense rows only (writes into `out`). Rows of degree
// > heavy_min are left to als_heavy_solve (INT_MAX: there are none).
torch::Tensor als_solve(torch::Tensor indptr, torch::Tensor indices,
                        torch::Tensor values, torch::Tensor Y,
                        c10::optional<torch::Tensor> YtY,
                        c10::optional<torch::Tensor> V,
                        double lambda, double alpha,
                        bool implicit_mode, bool wr_scale,
                        int64_t which, c10::optional<torch::Tensor> out,
                        c10::optional<torch::Tensor> prof,
                        int64_t heavy_min) {
  TORCH_CHECK(heavy_min > 0 && heavy_min <= INT_MAX,
              "heavy_min must be in [1, INT_MAX]");
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
                   (int)which, prof_ptr, (int)heavy_min, stream);
  C10_HIP_CHECK(hipGetLastError());
  return X;
}

// The dense solve at the padded ranks 192 and 256 (als_wide.hip): every row
// of the CSR in one pass, one 512-thread workgroup per row on `grid`
// persistent workgroups (0: one per CU, which is what the LDS admits).
// Same systems as als_solve; there is no Woodbury pass and no heavy-row
// split at these ranks.
torch::Tensor als_solve_wide(torch::Tensor indptr, torch::Tensor indices,
                             torch::Tensor values, torch::Tensor Y,
                             c10::optional<torch::Tensor> YtY,
                             double lambda, double alpha, bool implicit_mode,
                             bool wr_scale, c10::optional<torch::Tensor> out,
                             int64_t grid) {
  TORCH_CHECK(indptr.is_cuda() && indptr.scalar_type() == torch::kInt64 &&
                  indptr.is_contiguous(), "indptr must be contiguous i64 GPU");
  TORCH_CHECK(indices.is_cuda() && indices.scalar_type() == torch::kInt32 &&
                  indices.is_contiguous(), "indices must be contiguous i32 GPU");
  check_cuda_f32(values, "values");
  check_cuda_f32(Y, "Y");
  const int64_t f = Y.size(1);
  TORCH_CHECK_VALUE(f == 192 || f == 256,
                    "rank must be padded to 192 or 256, got ", f);
  TORCH_CHECK(indptr.size(0) >= 1, "indptr must hold n_rows + 1 entries");
  const int64_t n_rows = indptr.size(0) - 1;
  TORCH_CHECK(n_rows <= INT_MAX, "row counts must be below 2^31");
  TORCH_CHECK(indices.size(0) == values.size(0), "indices/values mismatch");
  TORCH_CHECK_VALUE(!implicit_mode || YtY.has_value(),
                    "implicit mode needs YtY");
  TORCH_CHECK(grid >= 0 && grid <= (1 << 20), "grid must be in [0, 2^20]");
  const float* yty_ptr = nullptr;
  if (YtY.has_value()) {
    check_cuda_f32(*YtY, "YtY");
    TORCH_CHECK(YtY->size(0) == f && YtY->size(1) == f, "YtY must be f x f");
    yty_ptr = YtY->data_ptr<float>();
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
  if (n_rows == 0) return X;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Y.device());
  hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (grid == 0)
    grid = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  grid = std::min<int64_t>(grid, n_rows);
  launch_als_solve_wide(
      reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>()),
      indices.data_ptr<int>(), values.data_ptr<float>(), Y.data_ptr<float>(),
      yty_ptr, X.data_ptr<float>(), (int)n_rows, (int)f, (float)lambda,
      (float)alpha, implicit_mode ? 1 : 0, wr_scale ? 1 : 0, -1, INT_MAX,
      (int)grid, stream);
  C10_HIP_CHECK(hipGetLastError());
  return X;
}

// The split-row pass for heavy rows (als_heavy.hip): per chunk of
// consecutive CSR entries a partial normal matrix and right-hand side on
// fp32 MFMA, then one solve per row over its partials in chunk order.
// rows [H], chunk_ptr [H + 1] and chunks [C, 2] (entry start, end) are
// i64 GPU tensors; chunk_ptr_host is chunk_ptr on the CPU. The caller has
// checked them against X and the CSR. The partial workspace takes at most
// ws_bytes; longer chunk tables are walked in batches.
// nonnegative: the partials go to the block-pivoting solver of
// als_nnls.hip instead of the Cholesky solve; iters, if given, receives
// that solver's trip count per row of X.
int* check_iters(const c10::optional<torch::Tensor>& iters,
                 const torch::Tensor& X);

void als_heavy_solve(torch::Tensor indices, torch::Tensor values,
                     torch::Tensor Y, c10::optional<torch::Tensor> YtY,
                     torch::Tensor X, torch::Tensor rows,
                     torch::Tensor chunk_ptr, torch::Tensor chunks,
                     torch::Tensor chunk_ptr_host, double lambda,
                     double alpha, bool implicit_mode, bool wr_scale,
                     int64_t ws_bytes, bool nonnegative,
                     c10::optional<torch::Tensor> iters) {
  TORCH_CHECK(nonnegative || !iters.has_value(),
              "iters is an output of the nonnegative solver");
  int* iters_ptr = check_iters(iters, X);
  TORCH_CHECK(indices.is_cuda() && indices.scalar_type() == torch::kInt32 &&
                  indices.is_contiguous(), "indices must be contiguous i32 GPU");
  check_cuda_f32(values, "values");
  check_cuda_f32(Y, "Y");
  check_cuda_f32(X, "X");
  const int64_t f = Y.size(1);
  TORCH_CHECK(supported_rank(f), "rank must be one of 16/32/64/128, got ", f);
  TORCH_CHECK(X.dim() == 2 && X.size(1) == f, "X must be n_rows x f");
  TORCH_CHECK(indices.size(0) == values.size(0), "indices/values mismatch");
  // factor rows are gathered in 16-byte quads
  TORCH_CHECK(reinterpret_cast<uintptr_t>(Y.data_ptr()) % 16 == 0,
              "Y must be 16-byte aligned");
  const float* yty_ptr = nullptr;
  if (YtY.has_value()) {
    check_cuda_f32(*YtY, "YtY");
    TORCH_CHECK(YtY->size(0) == f && YtY->size(1) == f, "YtY must be f x f");
    yty_ptr = YtY->data_ptr<float>();
  }
  auto i64_gpu = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                    t.scalar_type() == torch::kInt64 &&
                    t.device() == Y.device(),
                name, " must be a contiguous i64 tensor on Y's device");
  };
  i64_gpu(rows, "rows");
  i64_gpu(chunk_ptr, "chunk_ptr");
  i64_gpu(chunks, "chunks");
  const int64_t H = rows.numel();
  TORCH_CHECK(H < INT_MAX, "too many heavy rows");
  TORCH_CHECK(!chunk_ptr_host.is_cuda() && chunk_ptr_host.is_contiguous() &&
                  chunk_ptr_host.scalar_type() == torch::kInt64 &&
                  chunk_ptr_host.numel() == H + 1 && chunk_ptr.numel() == H + 1,
              "chunk_ptr / chunk_ptr_host must hold rows + 1 i64 entries");
  if (H == 0) return;
  const int64_t* cp = chunk_ptr_host.data_ptr<int64_t>();
  TORCH_CHECK(cp[0] == 0, "chunk_ptr must start at 0");
  for (int64_t h = 0; h < H; ++h)
    TORCH_CHECK(cp[h + 1] > cp[h], "every heavy row needs a chunk");
  const int64_t C = cp[H];
  TORCH_CHECK(chunks.dim() == 2 && chunks.size(0) == C && chunks.size(1) == 2,
              "chunks must be [chunk_ptr[-1], 2]");
  const int64_t slot = als_heavy_slot_floats((int)f);
  int64_t slots = ws_bytes / (slot * (int64_t)sizeof(float));
  slots = slots < 1 ? 1 : (slots > C ? C : slots);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Y.device());
  hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  torch::Tensor ws = torch::empty({slots * slot}, Y.options());
  torch::Tensor carry = torch::empty({2 * slot}, Y.options());
  if (nonnegative)
    launch_als_heavy_nnls(
        reinterpret_cast<const long long*>(chunks.data_ptr<int64_t>()),
        reinterpret_cast<const long long*>(chunk_ptr.data_ptr<int64_t>()),
        reinterpret_cast<const long long*>(rows.data_ptr<int64_t>()),
        reinterpret_cast<const long long*>(cp), (int)H,
        indices.data_ptr<int>(), values.data_ptr<float>(),
        Y.data_ptr<float>(), yty_ptr, X.data_ptr<float>(), iters_ptr,
        ws.data_ptr<float>(), (long long)slots, carry.data_ptr<float>(),
        (int)f, (float)lambda, (float)alpha, implicit_mode ? 1 : 0,
        wr_scale ? 1 : 0, stream);
  else
  launch_als_heavy(
      reinterpret_cast<const long long*>(chunks.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(chunk_ptr.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(rows.data_ptr<int64_t>()),
      reinterpret_cast<const long long*>(cp), (int)H,
      indices.data_ptr<int>(), values.data_ptr<float>(), Y.data_ptr<float>(),
      yty_ptr, X.data_ptr<float>(), ws.data_ptr<float>(), (long long)slots,
      carry.data_ptr<float>(), (int)f, (float)lambda, (float)alpha,
      implicit_mode ? 1 : 0, wr_scale ? 1 : 0, stream);
  C10_HIP_CHECK(hipGetLastError());
}

int* check_iters(const c10::optional<torch::Tensor>& iters,
                 const torch::Tensor& X) {
  if (!iters.has_value()) return nullptr;
  TORCH_CHECK(iters->is_cuda() && iters->is_contiguous() &&
                  iters->scalar_type() == torch::kInt32 &&
                  iters->device() == X.device() &&
                  iters->numel() == X.size(0),
              "iters must be a contiguous i32 GPU tensor, one per row");
  return iters->data_ptr<int>();
}

// The nonnegative half-step (als_nnls.hip): per row the minimiser of
// 1/2 x^T A x - b^T x over x >= 0, A and b those of als_solve, by block
// principal pivoting. Every row of degree <= skip_above is solved; rows
// above it are left to als_heavy_solve(nonnegative = true). iters, if
// given ([n_rows] i32), receives the solver's trip count per row.
torch::Tensor als_nnls_solve(torch::Tensor indptr, torch::Tensor indices,
                             torch::Tensor values, torch::Tensor Y,
                             c10::optional<torch::Tensor> YtY,
                             double lambda, double alpha,
                             bool implicit_mode, bool wr_scale,
                             c10::optional<torch::Tensor> out,
                             int64_t skip_above,
                             c10::optional<torch::Tensor> iters) {
  TORCH_CHECK(skip_above > 0 && skip_above <= INT_MAX,
              "skip_above must be in [1, INT_MAX]");
  TORCH_CHECK(indptr.is_cuda() && indptr.scalar_type() == torch::kInt64 &&
                  indptr.is_contiguous(), "indptr must be contiguous i64 GPU");
  TORCH_CHECK(indices.is_cuda() && indices.scalar_type() == torch::kInt32 &&
                  indices.is_contiguous(), "indices must be contiguous i32 GPU");
  check_cuda_f32(values, "values");
  check_cuda_f32(Y, "Y");
  const int64_t f = Y.size(1);
  TORCH_CHECK(supported_rank(f), "rank must be one of 16/32/64/128, got ", f);
  const int64_t n_rows = indptr.size(0) - 1;
  TORCH_CHECK(n_rows >= 0 && n_rows < INT_MAX, "row count must be below 2^31");
  TORCH_CHECK(indices.size(0) == values.size(0), "indices/values mismatch");
  // factor rows and YtY rows are read in 16-byte quads
  TORCH_CHECK(reinterpret_cast<uintptr_t>(Y.data_ptr()) % 16 == 0,
              "Y must be 16-byte aligned");
  const float* yty_ptr = nullptr;
  if (YtY.has_value()) {
    check_cuda_f32(*YtY, "YtY");
    TORCH_CHECK(YtY->size(0) == f && YtY->size(1) == f, "YtY must be f x f");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(YtY->data_ptr()) % 16 == 0,
                "YtY must be 16-byte aligned");
    yty_ptr = YtY->data_ptr<float>();
  }
  TORCH_CHECK(!implicit_mode || yty_ptr != nullptr,
              "implicit mode needs YtY");
  torch::Tensor X;
  if (out.has_value()) {
    check_cuda_f32(*out, "out");
    TORCH_CHECK(out->size(0) == n_rows && out->size(1) == f,
                "out must be n_rows x f");
    X = *out;
  } else {
    X = torch::empty({n_rows, f}, Y.options());
  }
  int* iters_ptr = check_iters(iters, X);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Y.device());
  hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_als_nnls(
      reinterpret_cast<const long long*>(indptr.data_ptr<int64_t>()),
      indices.data_ptr<int>(), values.data_ptr<float>(), Y.data_ptr<float>(),
      yty_ptr, X.data_ptr<float>(), iters_ptr, (int)n_rows, (int)f,
      (float)lambda, (float)alpha, implicit_mode ? 1 : 0, wr_scale ? 1 : 0,
      (int)skip_above, stream);
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
    c10::optional<torch::Tensor> query_cats,
    c10::optional<torch::Tensor> item_weights) {
  check_cuda_f32(Xq, "Xq");
  check_cuda_f32(Y, "Y");
  const float* wts = check_item_weights(item_weights, Y, prof.has_value());
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
                    a.item_cats, a.query_cats, a.cw, wts, stream);
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
    c10::optional<bool> gth_opt,
    c10::optional<torch::Tensor> item_weights) {
  TORCH_CHECK(Xq.is_cuda() && Xq.is_contiguous() &&
                  Xq.scalar_type() == torch::kBFloat16,
              "Xq must be contiguous bf16 GPU");
  TORCH_CHECK(Y.is_cuda() && Y.is_contiguous() &&
                  Y.scalar_type() == torch::kBFloat16,
              "Y must be contiguous bf16 GPU");
  const float* wts = check_item_weights(item_weights, Y, prof.has_value());
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
      a.query_cats, a.cw, interleave ? 1 : 0, wts, stream);
  C10_HIP_CHECK(hipGetLastError());
  return {out_val, out_idx};
}

// topk_score_mfma for padded ranks 256 / 384 / 512 (topk_mfma_wide.hip:
// the rank streamed through LDS in 128-wide panels). Same arguments, same
// validation, same output layout; the wide kernel has no phase probe, so
// a prof tensor raises.
std::tuple<torch::Tensor, torch::Tensor> topk_score_mfma_wide(
    torch::Tensor Xq, torch::Tensor Y, int64_t K, int64_t n_slices,
    c10::optional<torch::Tensor> item_mask,
    c10::optional<torch::Tensor> ban_indptr,
    c10::optional<torch::Tensor> ban_indices, int64_t item_base,
    c10::optional<torch::Tensor> prof,
    c10::optional<torch::Tensor> item_cats,
    c10::optional<torch::Tensor> query_cats, bool interleave,
    c10::optional<bool> gth_opt,
    c10::optional<torch::Tensor> item_weights) {
  TORCH_CHECK(Xq.is_cuda() && Xq.is_contiguous() &&
                  Xq.scalar_type() == torch::kBFloat16,
              "Xq must be contiguous bf16 GPU");
  TORCH_CHECK(Y.is_cuda() && Y.is_contiguous() &&
                  Y.scalar_type() == torch::kBFloat16,
              "Y must be contiguous bf16 GPU");
  TORCH_CHECK(!prof.has_value(), "the wide-rank kernel has no phase probe");
  const float* wts = check_item_weights(item_weights, Y, false);
  TORCH_CHECK(Xq.dim() == 2 && Y.dim() == 2, "Xq and Y must be 2-D");
  const int64_t f = Y.size(1);
  TORCH_CHECK(f == 256 || f == 384 || f == 512,
              "wide mfma rank must be one of 256/384/512, got ", f);
  TORCH_CHECK(Xq.size(1) == f, "Xq/Y rank mismatch");
  TORCH_CHECK(K >= 1 && K <= 64, "K must be in [1, 64]");
  const int64_t B = Xq.size(0);
  const int64_t N = Y.size(0);
  TORCH_CHECK(n_slices >= 1);
  const TopkArgs a = check_topk_args(item_mask, ban_indptr, ban_indices, prof,
                                     item_cats, query_cats, B, N);
  auto out_val = torch::empty({B, n_slices * K},
                              Xq.options().dtype(torch::kFloat32));
  auto out_idx = torch::empty({B, n_slices * K},
                              Xq.options().dtype(torch::kInt32));
  if (B == 0) return {out_val, out_idx};
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Y.device());
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  // the cross-slice threshold cell, as in topk_score_mfma
  torch::Tensor th_g;
  unsigned* th_g_ptr = nullptr;
  const char* e_gth = getenv("PIO_TOPK_GTH");
  const bool gth = gth_opt.has_value()
      ? *gth_opt : !(e_gth != nullptr && e_gth[0] == '0');
  if (gth) {
    th_g = torch::zeros({B}, Xq.options().dtype(torch::kInt32));
    th_g_ptr = reinterpret_cast<unsigned*>(th_g.data_ptr<int>());
  }
  launch_topk_mfma_wide(
      reinterpret_cast<const unsigned short*>(Xq.data_ptr()),
      reinterpret_cast<const unsigned short*>(Y.data_ptr()), a.mask,
      a.ban_indptr, a.ban_indices, out_val.data_ptr<float>(),
      out_idx.data_ptr<int>(), (int)B, (long long)N, (int)f, (int)K,
      (int)n_slices, (int)item_base, th_g_ptr, a.item_cats, a.query_cats,
      a.cw, interleave ? 1 : 0, wts, stream);
  C10_HIP_CHECK(hipGetLastError());
  return {out_val, out_idx};
}

// out[b, c] = dot(Xq[b, :], Y[idx[b, c], :]) in fp32, times
// item_weights[idx[b, c]] when weights are given; idx < 0 gives -inf.
// Any rank: rows move as float4 when f % 4 == 0 and both base pointers
// are 16-byte aligned, as single floats otherwise. The kernel trusts
// idx, so the upper bound is checked here (one small reduction).
torch::Tensor topk_rescore(torch::Tensor Xq, torch::Tensor Y,
                           torch::Tensor idx,
                           c10::optional<torch::Tensor> item_weights) {
  // idx is int32: checked first, before anything looks at the data
  TORCH_CHECK_VALUE(Y.dim() == 2 && Y.size(0) < (1LL << 31),
                    "the item count N must be below 2^31");
  check_cuda_f32(Xq, "Xq");
  check_cuda_f32(Y, "Y");
  const float* wts = check_item_weights(item_weights, Y, false);
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
                      idx.data_ptr<int>(), wts, out.data_ptr<float>(),
                      (long long)B, (int)C, (int)Xq.size(1), stream);
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

// One tier of co-occurrence top-N (see cooc_topn.hip): the item rows
// listed in `rows` are counted, selected and written to top_ids/top_cnt
// [Na, n] in place; rows not listed are left alone. tier 0 / 1: the
// 1024- / 8192-slot LDS hash tables; tier 2: dense counters in `pool`,
// a zero [G, Nb] i32 tensor that is all zero again afterwards, one
// persistent workgroup per counter row; tier 3: dense counters in LDS,
// Nb <= cooc_dense_lds_max(). (i_indptr, i_users) is the item-major CSR
// of the row side A, (u_indptr, u_items) the user-major CSR of the
// column side B over Nb = n_cols items; n_cols < 0 says that they hold
// the same pairs (Nb = Na). exclude_self drops the pair (i, i) and needs
// Na == Nb. With llr set the rows are ranked by the log-likelihood
// ratio, top_cnt is fp32 and col_deg i32 [Nb] / col_h f64 [Nb] carry the
// column totals. Ids are trusted (ops/cooccurrence.py range-checks the
// CSRs first).
void cooc_topn(torch::Tensor u_indptr, torch::Tensor u_items,
               torch::Tensor i_indptr, torch::Tensor i_users,
               torch::Tensor rows, int64_t n, int64_t tier,
               c10::optional<torch::Tensor> pool, torch::Tensor top_ids,
               torch::Tensor top_cnt, bool llr, bool exclude_self,
               int64_t n_cols, c10::optional<torch::Tensor> col_deg,
               c10::optional<torch::Tensor> col_h) {
  auto check = [](const torch::Tensor& t, torch::ScalarType st, int64_t dim,
                  const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == st &&
                    t.dim() == dim,
                name, " must be a contiguous ", dim, "-D ", c10::toString(st),
                " GPU tensor");
  };
  check(u_indptr, torch::kInt64, 1, "u_indptr");
  check(i_indptr, torch::kInt64, 1, "i_indptr");
  check(u_items, torch::kInt32, 1, "u_items");
  check(i_users, torch::kInt32, 1, "i_users");
  check(rows, torch::kInt32, 1, "rows");
  check(top_ids, torch::kInt32, 2, "top_ids");
  check(top_cnt, llr ? torch::kFloat32 : torch::kInt32, 2, "top_cnt");
  TORCH_CHECK(u_indptr.size(0) >= 1 && i_indptr.size(0) >= 1,
              "indptr tensors must not be empty");
  TORCH_CHECK(n_cols >= 0 || u_items.size(0) == i_users.size(0),
              "the two CSRs must hold the same pairs");
  TORCH_CHECK(n >= 1 && n <= 64, "n must be in [1, 64], got ", n);
  TORCH_CHECK(tier >= 0 && tier <= 3, "tier must be 0, 1, 2 or 3");
  const int64_t Na = i_indptr.size(0) - 1;
  const int64_t N = n_cols < 0 ? Na : n_cols;  // the counters' size
  const int64_t U = u_indptr.size(0) - 1;
  TORCH_CHECK(N < (1LL << 31) && Na < (1LL << 31) && U < (1LL << 31),
              "item and user counts must be below 2^31");
  TORCH_CHECK(!exclude_self || N == Na,
              "exclude_self needs the same item count on both sides");
  TORCH_CHECK(top_ids.size(0) == Na && top_ids.size(1) == n &&
                  top_cnt.size(0) == Na && top_cnt.size(1) == n,
              "top_ids and top_cnt must be [N, n]");
  const auto dev = u_indptr.device();
  TORCH_CHECK(u_items.device() == dev && i_indptr.device() == dev &&
                  i_users.device() == dev && rows.device() == dev &&
                  top_ids.device() == dev && top_cnt.device() == dev,
              "all tensors must be on one device");
  const int* deg_ptr = nullptr;
  const double* h_ptr = nullptr;
  if (llr) {
    TORCH_CHECK(col_deg.has_value() && col_h.has_value(),
                "llr needs col_deg and col_h");
    check(*col_deg, torch::kInt32, 1, "col_deg");
    check(*col_h, torch::kFloat64, 1, "col_h");
    TORCH_CHECK(col_deg->size(0) == N && col_h->size(0) == N &&
                    col_deg->device() == dev && col_h->device() == dev,
                "col_deg and col_h must be [Nb] on the inputs' device");
    deg_ptr = col_deg->data_ptr<int>();
    h_ptr = col_h->data_ptr<double>();
  }
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
      top_cnt.data_ptr(), (int)llr, (int)!exclude_self, deg_ptr, h_ptr,
      (int)U, (int)grid, stream);
  C10_HIP_CHECK(hipGetLastError());
}

// Candidate-list top-K over a list of segments (see topk_cand.hip): each
// row (query, lo, hi) of `segs` ranks cand_indices[lo..hi) for its query.
// K in [1, 64] returns the segments' K best as (vals [n_segs, K] fp32,
// idx [n_segs, K] i32), score descending then id ascending, empty slots
// -inf / -1; threads (64 or 256) picks the instantiation. K = 0 is scores
// mode: `scores` [nnz] receives every listed candidate's fp32 score, -inf
// where it is filtered, and the returned tensors are empty. Xq and Y are
// read where they lie, any rank 1 <= f <= 128. The candidate ids and the
// segments are trusted: ops/topk.py range-checks the ids and builds the
// segments from the checked CSR.
std::tuple<torch::Tensor, torch::Tensor> topk_cand(
    torch::Tensor Xq, torch::Tensor Y, torch::Tensor cand_indices,
    torch::Tensor segs, int64_t K, int64_t threads,
    c10::optional<torch::Tensor> item_mask,
    c10::optional<torch::Tensor> ban_indptr,
    c10::optional<torch::Tensor> ban_indices,
    c10::optional<torch::Tensor> item_cats,
    c10::optional<torch::Tensor> query_cats,
    c10::optional<torch::Tensor> scores,
    c10::optional<torch::Tensor> item_weights) {
  check_cuda_f32(Xq, "Xq");
  check_cuda_f32(Y, "Y");
  TORCH_CHECK(Xq.dim() == 2 && Y.dim() == 2, "Xq and Y must be 2-D");
  const float* wts = check_item_weights(item_weights, Y, false);
  const int64_t B = Xq.size(0);
  const int64_t N = Y.size(0);
  const int64_t f = Y.size(1);
  TORCH_CHECK(Xq.size(1) == f, "Xq/Y rank mismatch");
  TORCH_CHECK(f >= 1 && f <= 128, "rank must be in [1, 128], got ", f);
  TORCH_CHECK(N < (1LL << 31), "item count must be below 2^31");
  TORCH_CHECK(cand_indices.is_cuda() && cand_indices.is_contiguous() &&
                  cand_indices.scalar_type() == torch::kInt32 &&
                  cand_indices.dim() == 1,
              "cand_indices must be a contiguous 1-D i32 GPU tensor");
  TORCH_CHECK(segs.is_cuda() && segs.is_contiguous() &&
                  segs.scalar_type() == torch::kInt64 && segs.dim() == 2 &&
                  segs.size(1) == 3,
              "segs must be a contiguous [n, 3] i64 GPU tensor");
  TORCH_CHECK(threads == 64 || threads == 256, "threads must be 64 or 256");
  TORCH_CHECK(K >= 0 && K <= 64, "K must be in [0, 64]");
  TORCH_CHECK((K == 0) == scores.has_value(),
              "scores goes with K = 0 and only with it");
  const auto dev = Xq.device();
  TORCH_CHECK(Y.device() == dev && cand_indices.device() == dev &&
                  segs.device() == dev,
              "all tensors must be on one device");
  const TopkArgs a = check_topk_args(item_mask, ban_indptr, ban_indices,
                                     c10::nullopt, item_cats, query_cats, B,
                                     N);
  const int64_t n_segs = segs.size(0);
  TORCH_CHECK(n_segs < (1LL << 31), "too many segments for one launch");
  float* scores_ptr = nullptr;
  if (scores.has_value()) {
    check_cuda_f32(*scores, "scores");
    TORCH_CHECK(scores->dim() == 1 &&
                    scores->size(0) == cand_indices.size(0) &&
                    scores->device() == dev,
                "scores must be [nnz] on Xq's device");
    scores_ptr = scores->data_ptr<float>();
  }
  auto out_val = torch::empty({K == 0 ? 0 : n_segs, K}, Xq.options());
  auto out_idx = torch::empty({K == 0 ? 0 : n_segs, K},
                              Xq.options().dtype(torch::kInt32));
  if (n_segs == 0) return {out_val, out_idx};
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  const int n_cu = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const int thr = K == 0 ? 256 : (int)threads;
  // 32 waves per CU either way: 32 one-wave or 8 four-wave workgroups
  const int64_t grid =
      std::min<int64_t>(n_segs, (int64_t)n_cu * (thr == 64 ? 32 : 8));
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_topk_cand(
      Xq.data_ptr<float>(), Y.data_ptr<float>(), cand_indices.data_ptr<int>(),
      reinterpret_cast<const long long*>(segs.data_ptr<int64_t>()),
      (int)n_segs, a.mask, a.ban_indptr, a.ban_indices, a.item_cats,
      a.query_cats, wts, a.cw, (int)f, (int)K, thr, out_val.data_ptr<float>(),
      out_idx.data_ptr<int>(), scores_ptr, (int)grid, stream);
  C10_HIP_CHECK(hipGetLastError());
  return {out_val, out_idx};
}

// One tier of indicator top-K (see indicator_topk.hip): the queries
// listed in `work` (sorted by entry count descending; max_items = the row
// count of work[0]) sum the rows of the indicator table that their CSR
// segment names, filter and rank, and write their rows of out_ids /
// out_scores [B, K] in place; rows not listed are left alone. threads 64
// takes queries of at most indicator_topk_cap(64) entries (rows x n),
// threads 256 of at most indicator_topk_cap(256). top_scores / out_scores
// are int32 (counts) or fp32. The ban and allow CSRs are optional, each
// given whole or not at all; exclude_query drops a query's own rows and
// needs n_cols == Nr. All ids are trusted: ops/cooccurrence.py
// range-checks the table, the query CSR and the lists first.
void indicator_topk(torch::Tensor top_ids, torch::Tensor top_scores,
                    torch::Tensor q_indptr, torch::Tensor q_items,
                    torch::Tensor work, int64_t max_items, int64_t threads,
                    int64_t K, int64_t n_cols,
                    c10::optional<torch::Tensor> ban_indptr,
                    c10::optional<torch::Tensor> ban_indices,
                    c10::optional<torch::Tensor> allow_indptr,
                    c10::optional<torch::Tensor> allow_indices,
                    c10::optional<torch::Tensor> item_cats,
                    c10::optional<torch::Tensor> query_cats,
                    bool exclude_query, torch::Tensor out_ids,
                    torch::Tensor out_scores) {
  const auto dev = top_ids.device();
  auto check = [&dev](const torch::Tensor& t, torch::ScalarType st,
                      int64_t dim, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == st &&
                    t.dim() == dim && t.device() == dev,
                name, " must be a contiguous ", dim, "-D ", c10::toString(st),
                " tensor on the table's GPU");
  };
  const auto st = top_scores.scalar_type();
  TORCH_CHECK(st == torch::kInt32 || st == torch::kFloat32,
              "top_scores must be int32 or float32");
  check(top_ids, torch::kInt32, 2, "top_ids");
  check(top_scores, st, 2, "top_scores");
  check(q_indptr, torch::kInt64, 1, "q_indptr");
  check(q_items, torch::kInt32, 1, "q_items");
  check(work, torch::kInt32, 1, "work");
  check(out_ids, torch::kInt32, 2, "out_ids");
  check(out_scores, st, 2, "out_scores");
  TORCH_CHECK(top_scores.sizes() == top_ids.sizes(),
              "top_ids and top_scores must have one shape");
  const int64_t Nr = top_ids.size(0);
  const int64_t n = top_ids.size(1);
  const int64_t B = q_indptr.size(0) - 1;
  TORCH_CHECK(B >= 0, "q_indptr must not be empty");
  TORCH_CHECK(Nr < (1LL << 31) && n_cols >= 1 && n_cols < (1LL << 31) &&
                  B < (1LL << 31) && n < (1LL << 31),
              "row, column and query counts must be below 2^31");
  TORCH_CHECK(K >= 1 && K <= 1024, "K must be in [1, 1024], got ", K);
  TORCH_CHECK(out_ids.size(0) == B && out_ids.size(1) == K &&
                  out_scores.size(0) == B && out_scores.size(1) == K,
              "out_ids and out_scores must be [B, K]");
  TORCH_CHECK(threads == 64 || threads == 256, "threads must be 64 or 256");
  TORCH_CHECK(!exclude_query || n_cols == Nr,
              "exclude_query needs n_cols == the table's row count");
  TORCH_CHECK(max_items >= 0 &&
                  max_items * n <= indicator_topk_cap((int)threads),
              "a query of ", max_items, " rows x ", n,
              " entries exceeds this instantiation's cap");
  auto opt_csr = [&](const c10::optional<torch::Tensor>& ip,
                     const c10::optional<torch::Tensor>& ix, const char* name,
                     const long long*& ip_ptr, const int*& ix_ptr) {
    TORCH_CHECK(ip.has_value() == ix.has_value(), name,
                ": indptr and indices must be given together");
    if (!ip.has_value()) return;
    check(*ip, torch::kInt64, 1, name);
    check(*ix, torch::kInt32, 1, name);
    TORCH_CHECK(ip->size(0) == B + 1, name, ": indptr must be B + 1");
    ip_ptr = reinterpret_cast<const long long*>(ip->data_ptr<int64_t>());
    ix_ptr = ix->data_ptr<int>();
  };
  const long long* ban_p = nullptr;
  const long long* allow_p = nullptr;
  const int* ban_x = nullptr;
  const int* allow_x = nullptr;
  opt_csr(ban_indptr, ban_indices, "ban list", ban_p, ban_x);
  opt_csr(allow_indptr, allow_indices, "allow list", allow_p, allow_x);
  const int cw = check_cats(item_cats, query_cats, B, n_cols, false);
  TORCH_CHECK(cw == 0 || (item_cats->device() == dev &&
                          query_cats->device() == dev),
              "category words must be on the table's GPU");
  const int64_t n_work = work.size(0);
  if (n_work == 0 || max_items == 0 || n == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
  const int n_cu = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_indicator_topk(
      top_ids.data_ptr<int>(), top_scores.data_ptr(), (int)n,
      reinterpret_cast<const long long*>(q_indptr.data_ptr<int64_t>()),
      q_items.data_ptr<int>(), work.data_ptr<int>(), (int)n_work,
      (int)max_items, ban_p, ban_x, allow_p, allow_x,
      cw ? item_cats->data_ptr<int>() : nullptr,
      cw ? query_cats->data_ptr<int>() : nullptr, cw,
      st == torch::kFloat32 ? 1 : 0, exclude_query ? 1 : 0, (int)K,
      (int)threads, n_cu, out_ids.data_ptr<int>(), out_scores.data_ptr(),
      stream);
  C10_HIP_CHECK(hipGetLastError());
}

// Held-out rank counts (see rank_count.hip). The slot arrays come from
// ops/ranking.py: slot_user [S] names the X row of each slot, slot_tgt
// [S, TMAX] its target item ids (-1 = none), S a multiple of the slot
// group. Ids are trusted: the wrapper validates the CSRs first.
void check_rank_common(const torch::Tensor& X, const torch::Tensor& Y,
                       const torch::Tensor& slot_user) {
  check_cuda_f32(X, "X");
  check_cuda_f32(Y, "Y");
  TORCH_CHECK(X.dim() == 2 && Y.dim() == 2 && X.size(1) == Y.size(1) &&
                  supported_rank(X.size(1)),
              "X and Y must be 2-D with one rank in {16, 32, 64, 128}");
  TORCH_CHECK(X.size(0) >= 1 && Y.size(0) >= 1 &&
                  Y.size(0) < (1LL << 31) && X.size(0) < (1LL << 31),
              "X and Y need between 1 and 2^31 - 1 rows");
  TORCH_CHECK(slot_user.is_cuda() && slot_user.is_contiguous() &&
                  slot_user.scalar_type() == torch::kInt32 &&
                  slot_user.dim() == 1 &&
                  slot_user.size(0) % rank_count_group() == 0 &&
                  slot_user.size(0) < (1LL << 31),
              "slot_user must be a contiguous 1-D int32 GPU tensor, its "
              "length a multiple of ", rank_count_group());
  TORCH_CHECK(Y.device() == X.device() && slot_user.device() == X.device(),
              "all tensors must be on one GPU");
}

// Target scores and seen-list corrections: (tscore [S, TMAX] fp32,
// corr [S, 2, TMAX] int32 = seen items scoring > / >= each target).
std::vector<torch::Tensor> rank_list(
    torch::Tensor X, torch::Tensor Y, torch::Tensor slot_user,
    torch::Tensor slot_tgt, c10::optional<torch::Tensor> seen_indptr,
    c10::optional<torch::Tensor> seen_indices) {
  check_rank_common(X, Y, slot_user);
  const int64_t S = slot_user.size(0);
  const int T = rank_count_tmax();
  TORCH_CHECK(slot_tgt.is_cuda() && slot_tgt.is_contiguous() &&
                  slot_tgt.scalar_type() == torch::kInt32 &&
                  slot_tgt.dim() == 2 && slot_tgt.size(0) == S &&
                  slot_tgt.size(1) == T && slot_tgt.device() == X.device(),
              "slot_tgt must be a contiguous [S, ", T, "] int32 GPU tensor");
  TORCH_CHECK(seen_indptr.has_value() == seen_indices.has_value(),
              "seen_indptr and seen_indices must be given together");
  const long long* sp = nullptr;
  const int* sx = nullptr;
  if (seen_indptr.has_value()) {
    TORCH_CHECK(seen_indptr->is_cuda() && seen_indptr->is_contiguous() &&
                    seen_indptr->scalar_type() == torch::kInt64 &&
                    seen_indptr->dim() == 1 &&
                    seen_indptr->size(0) == X.size(0) + 1 &&
                    seen_indptr->device() == X.device(),
                "seen_indptr must be a contiguous int64 GPU tensor of "
                "X's rows + 1");
    TORCH_CHECK(seen_indices->is_cuda() && seen_indices->is_contiguous() &&
                    seen_indices->scalar_type() == torch::kInt32 &&
                    seen_indices->dim() == 1 &&
                    seen_indices->device() == X.device(),
                "seen_indices must be a contiguous 1-D int32 GPU tensor");
    sp = reinterpret_cast<const long long*>(seen_indptr->data_ptr<int64_t>());
    sx = seen_indices->data_ptr<int>();
  }
  auto tscore = torch::empty({S, T}, X.options());
  auto corr = torch::empty({S, 2, T}, slot_user.options());
  if (S == 0) return {tscore, corr};
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_rank_list(X.data_ptr<float>(), Y.data_ptr<float>(),
                   slot_user.data_ptr<int>(), slot_tgt.data_ptr<int>(), sp, sx,
                   tscore.data_ptr<float>(), corr.data_ptr<int>(), (int)S,
                   (int)X.size(1), stream);
  C10_HIP_CHECK(hipGetLastError());
  return {tscore, corr};
}

// partial [n_slices, S, 2, TMAX] int32: per item slice, how many of its
// items score > (row 0) and, with ties, >= (row 1) each target score.
// Without ties row 1 is not written.
torch::Tensor rank_stream(torch::Tensor X, torch::Tensor Y,
                          torch::Tensor slot_user, torch::Tensor tscore,
                          int64_t n_slices, bool ties) {
  check_rank_common(X, Y, slot_user);
  const int64_t S = slot_user.size(0);
  const int T = rank_count_tmax();
  check_cuda_f32(tscore, "tscore");
  TORCH_CHECK(tscore.dim() == 2 && tscore.size(0) == S &&
                  tscore.size(1) == T && tscore.device() == X.device(),
              "tscore must be [S, ", T, "]");
  TORCH_CHECK(n_slices >= 1 && n_slices <= 65535,
              "n_slices must be in [1, 65535], got ", n_slices);
  auto partial = torch::empty({n_slices, S, 2, T}, slot_user.options());
  if (S == 0) return partial;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  hipStream_t stream =
      c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  launch_rank_stream(X.data_ptr<float>(), Y.data_ptr<float>(),
                     (long long)Y.size(0), slot_user.data_ptr<int>(),
                     tscore.data_ptr<float>(), (int)S, (int)n_slices,
                     ties ? 1 : 0, partial.data_ptr<int>(), (int)X.size(1),
                     stream);
  C10_HIP_CHECK(hipGetLastError());
  return partial;
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
        py::arg("out") = py::none(), py::arg("prof") = py::none(),
        py::arg("heavy_min") = (int64_t)INT_MAX);
  m.def("als_solve_wide", &als_solve_wide,
        "Dense ALS half-iteration at padded ranks 192 / 256 (MFMA solver)",
        py::arg("indptr"), py::arg("indices"), py::arg("values"),
        py::arg("Y"), py::arg("YtY") = py::none(), py::arg("lambda_") = 0.01,
        py::arg("alpha") = 1.0, py::arg("implicit_mode") = false,
        py::arg("wr_scale") = true, py::arg("out") = py::none(),
        py::arg("grid") = (int64_t)0);
  m.def("als_wide_lds_bytes", &als_wide_lds_bytes,
        "LDS bytes per workgroup of the rank-192 / 256 solver");
  m.def("als_heavy_solve", &als_heavy_solve,
        "Split-row ALS solve of heavy rows: MFMA partial Gramians per chunk",
        py::arg("indices"), py::arg("values"), py::arg("Y"),
        py::arg("YtY"), py::arg("X"), py::arg("rows"), py::arg("chunk_ptr"),
        py::arg("chunks"), py::arg("chunk_ptr_host"), py::arg("lambda_"),
        py::arg("alpha"), py::arg("implicit_mode"), py::arg("wr_scale"),
        py::arg("ws_bytes") = (int64_t)256 << 20,
        py::arg("nonnegative") = false, py::arg("iters") = py::none());
  m.def("als_nnls_solve", &als_nnls_solve,
        "Nonnegative ALS half-iteration: fused block-pivoting NNLS solve",
        py::arg("indptr"), py::arg("indices"), py::arg("values"),
        py::arg("Y"), py::arg("YtY") = py::none(),
        py::arg("lambda_") = 0.01, py::arg("alpha") = 1.0,
        py::arg("implicit_mode") = false, py::arg("wr_scale") = true,
        py::arg("out") = py::none(),
        py::arg("skip_above") = (int64_t)INT_MAX,
        py::arg("iters") = py::none());
  m.def("als_nnls_max_it", &als_nnls_max_it,
        "Trip bound of the nonnegative solver");
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
        py::arg("query_cats") = py::none(),
        py::arg("item_weights") = py::none());
  m.def("topk_score_mfma", &topk_score_mfma,
        "Fused masked top-K scoring on MFMA (bf16 in, fp32 accumulate)",
        py::arg("Xq"), py::arg("Y"), py::arg("K"), py::arg("n_slices") = 64,
        py::arg("item_mask") = py::none(), py::arg("ban_indptr") = py::none(),
        py::arg("ban_indices") = py::none(), py::arg("item_base") = 0,
        py::arg("prof") = py::none(), py::arg("item_cats") = py::none(),
        py::arg("query_cats") = py::none(), py::arg("interleave") = false,
        py::arg("gth") = py::none(), py::arg("item_weights") = py::none());
  // the argument list of topk_score_mfma, position for position, so the
  // Python call sites are shared; prof is accepted only to be refused
  m.def("topk_score_mfma_wide", &topk_score_mfma_wide,
        "topk_score_mfma for padded ranks 256 / 384 / 512 (rank panels)",
        py::arg("Xq"), py::arg("Y"), py::arg("K"), py::arg("n_slices") = 64,
        py::arg("item_mask") = py::none(), py::arg("ban_indptr") = py::none(),
        py::arg("ban_indices") = py::none(), py::arg("item_base") = 0,
        py::arg("prof") = py::none(), py::arg("item_cats") = py::none(),
        py::arg("query_cats") = py::none(), py::arg("interleave") = false,
        py::arg("gth") = py::none(), py::arg("item_weights") = py::none());
  m.def("topk_rescore", &topk_rescore,
        "Exact fp32 dots of each query with its shortlisted items",
        py::arg("Xq"), py::arg("Y"), py::arg("idx"),
        py::arg("item_weights") = py::none());
  m.def("cooc_topn", &cooc_topn,
        "Co-occurrence top-N of the listed item rows, one tier",
        py::arg("u_indptr"), py::arg("u_items"), py::arg("i_indptr"),
        py::arg("i_users"), py::arg("rows"), py::arg("n"), py::arg("tier"),
        py::arg("pool"), py::arg("top_ids"), py::arg("top_cnt"),
        py::arg("llr") = false, py::arg("exclude_self") = true,
        py::arg("n_cols") = -1, py::arg("col_deg") = py::none(),
        py::arg("col_h") = py::none());
  m.def("topk_cand", &topk_cand,
        "Candidate-list top-K (or scores) over a list of segments",
        py::arg("Xq"), py::arg("Y"), py::arg("cand_indices"),
        py::arg("segs"), py::arg("K"), py::arg("threads"),
        py::arg("item_mask") = py::none(), py::arg("ban_indptr") = py::none(),
        py::arg("ban_indices") = py::none(),
        py::arg("item_cats") = py::none(), py::arg("query_cats") = py::none(),
        py::arg("scores") = py::none(),
        py::arg("item_weights") = py::none());
  m.def("cooc_dense_lds_max", &cooc_dense_lds_max,
        "Largest item count of the LDS dense tier");
  m.def("indicator_topk", &indicator_topk,
        "Indicator top-K of the listed queries, one tier",
        py::arg("top_ids"), py::arg("top_scores"), py::arg("q_indptr"),
        py::arg("q_items"), py::arg("work"), py::arg("max_items"),
        py::arg("threads"), py::arg("K"), py::arg("n_cols"),
        py::arg("ban_indptr"), py::arg("ban_indices"),
        py::arg("allow_indptr"), py::arg("allow_indices"),
        py::arg("item_cats"), py::arg("query_cats"),
        py::arg("exclude_query"), py::arg("out_ids"), py::arg("out_scores"));
  m.def("indicator_topk_cap", &indicator_topk_cap,
        "Largest entry count per query of the 64- / 256-thread kernel",
        py::arg("threads"));
  m.def("rank_list", &rank_list,
        "Held-out ranks: target scores and seen-list corrections per slot",
        py::arg("X"), py::arg("Y"), py::arg("slot_user"), py::arg("slot_tgt"),
        py::arg("seen_indptr") = py::none(),
        py::arg("seen_indices") = py::none());
  m.def("rank_stream", &rank_stream,
        "Held-out ranks: per-slice counts of items beating each target",
        py::arg("X"), py::arg("Y"), py::arg("slot_user"), py::arg("tscore"),
        py::arg("n_slices"), py::arg("ties") = true);
  m.def("rank_count_tmax", &rank_count_tmax, "Targets per slot");
  m.def("rank_count_group", &rank_count_group, "Slots per workgroup");
  m.def("rank_stream_lds_bytes", &rank_stream_lds_bytes,
        "Dynamic LDS of the stream kernel at rank f", py::arg("f"));
}
