// The WT = true (per-item score weights) instantiations of
// topk_mfma_kernel and their entry point launch_topk_mfma_wt, in a
// translation unit of their own: built with packed fp32 VALU ops off
// (ops/build.py), and the unweighted instantiations' build is untouched.
#define TM_WT true
#include "topk_mfma.hip"
