// Shared by the fused top-K kernels (topk_kernels.hip, topk_mfma.hip).
#pragma once

#include <hip/hip_runtime.h>

// membership test in a sorted int list (a query's banned items)
__device__ __forceinline__ bool in_sorted(const int* arr, int n, int x) {
  int lo = 0, hi = n - 1;
  while (lo <= hi) {
    int mid = (lo + hi) >> 1;
    int v = arr[mid];
    if (v == x) return true;
    if (v < x) lo = mid + 1; else hi = mid - 1;
  }
  return false;
}

// Launch Kernel with lds_bytes of dynamic LDS. A request above the 64 KB
// default limit first raises the kernel's own limit (once per kernel:
// the flag is per template instantiation) to the CU's 160 KB.
template <auto Kernel, typename... Args>
static void launch_dyn_lds(dim3 grid, dim3 block, size_t lds_bytes,
                           hipStream_t stream, Args... args) {
  static bool raised = false;
  if (!raised && lds_bytes > 64 * 1024) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    raised = true;
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, args...);
}
