// The WT = true (per-item score weights) instantiations of
// topk_score_kernel and their entry point launch_topk_score_wt, in a
// translation unit of their own: built with packed fp32 VALU ops off
// (ops/build.py), and the unweighted instantiations' build is untouched.
#define TK_WT true
#include "topk_kernels.hip"
