"""Build the _pio_hip extension in-tree with hipcc for gfx950.

No hipify, no CUDA path: the .hip sources are native CDNA4 code; hipcc
compiles host + device and links against libtorch's ROCm build. The .so is
written next to this file so it travels with the repo snapshot to GPU boxes.
"""

from __future__ import annotations

import os
import subprocess
import sys
import sysconfig
import tempfile

OPS_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(OPS_DIR, "csrc")
SO_PATH = os.path.join(OPS_DIR, "_pio_hip.so")
SOURCES = ["bindings.cpp", "als_kernels.hip", "als_xform.hip",
           "als_loss.hip", "topk_kernels.hip", "topk_mfma.hip", "topk_rescore.hip",
           "cooc_topn.hip", "topk_cand.hip", "indicator_topk.hip",
           "rank_count.hip", "topk_kernels_wt.hip", "topk_mfma_wt.hip",
           "als_heavy.hip", "als_nnls.hip", "topk_mfma_wide.hip",
           "als_wide.hip"]
# compiled on their own with packed fp32 VALU ops off (the vectorizer may
# otherwise pair independent fp32 chains), then linked with the rest.
# cooc_topn.hip is here since its LLR score stage: today it holds no
# fp32 arithmetic (fp64 sum, one cvt) and the ISA is the same with or
# without the flag, count kernels included; the flag keeps a later score
# functor's fp32 code (cosine, Jaccard) from being packed unnoticed. The
# file includes only the HIP runtime, so it needs none of the torch -D's.
# indicator_topk.hip: its fp32 segment sums are an ordered chain of adds
# (the canonical sum) and must stay one.
# rank_count.hip: its scores live on the matrix pipe and its epilogue is
# compares and integer adds, so the flag changes nothing today; it keeps
# fp32 VALU code added to it later from being packed unnoticed.
# topk_kernels_wt.hip, topk_mfma_wt.hip: the weighted (WT = true)
# instantiations of topk_kernels.hip / topk_mfma.hip, which they include;
# the unweighted ones stay in their own files, built as before.
# als_heavy.hip: the weight products that feed its MFMAs and its ordered
# partial sums are independent fp32 chains the vectorizer could pair.
# als_nnls.hip: the same Gramian tile loop, and the ordered fma chains of
# its Cholesky, substitutions and gradient must not be re-associated.
# topk_mfma_wide.hip: holds its weighted (WT = true) instantiations too,
# whose weight products must stay single fp32 ops like topk_mfma_wt.hip's.
# als_wide.hip: als_heavy.hip's reasons (weight products feeding MFMAs),
# and the ordered fma chains of its panel solve and substitutions.
NO_PACKED_FP32 = ["topk_cand.hip", "cooc_topn.hip", "indicator_topk.hip",
                  "rank_count.hip", "topk_kernels_wt.hip",
                  "topk_mfma_wt.hip", "als_heavy.hip", "als_nnls.hip",
                  "topk_mfma_wide.hip", "als_wide.hip"]
HEADERS = ["topk_common.h"]  # included by SOURCES: rebuild when they change
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def _torch_paths():
    import torch
    root = os.path.dirname(torch.__file__)
    return {
        "includes": [
            os.path.join(root, "include"),
            os.path.join(root, "include", "torch", "csrc", "api", "include"),
        ],
        "libdir": os.path.join(root, "lib"),
        "abi": int(torch._C._GLIBCXX_USE_CXX11_ABI),
    }


def needs_build() -> bool:
    if not os.path.exists(SO_PATH):
        return True
    so_mtime = os.path.getmtime(SO_PATH)
    for s in SOURCES + HEADERS:
        if os.path.getmtime(os.path.join(CSRC, s)) > so_mtime:
            return True
    return False


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not needs_build():
        return SO_PATH
    tp = _torch_paths()
    py_include = sysconfig.get_paths()["include"]
    hipcc = os.environ.get("HIPCC", "hipcc")
    cmd = [
        hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC",
        "-shared",
        "-DTORCH_EXTENSION_NAME=_pio_hip",
        "-DTORCH_API_INCLUDE_EXTENSION_H",
        f"-D_GLIBCXX_USE_CXX11_ABI={tp['abi']}",
        "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
        "-Wno-deprecated-declarations", "-Wno-unused-result",
        f"-I{py_include}",
    ]
    for inc in tp["includes"]:
        cmd.append(f"-I{inc}")
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        for s in NO_PACKED_FP32:
            obj = os.path.join(tmp, os.path.splitext(s)[0] + ".o")
            oc = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17",
                  "-fPIC", "-D__HIP_PLATFORM_AMD__=1",
                  "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
                  "-c", os.path.join(CSRC, s), "-o", obj]
            if verbose:
                print("[ops.build]", " ".join(oc), file=sys.stderr)
            subprocess.run(oc, check=True)
            objs.append(obj)
        # objects first: hipcc puts `-x hip` before the first .cpp and
        # would read anything after it as HIP source
        cmd += objs
        cmd += [os.path.join(CSRC, s) for s in SOURCES
                if s not in NO_PACKED_FP32]
        cmd += [
            f"-L{tp['libdir']}", f"-Wl,-rpath,{tp['libdir']}",
            "-ltorch", "-ltorch_cpu", "-ltorch_python", "-ltorch_hip",
            "-lc10", "-lc10_hip", "-lamdhip64",
            "-o", SO_PATH,
        ]
        if verbose:
            print("[ops.build]", " ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
    return SO_PATH


if __name__ == "__main__":
    build(force="--force" in sys.argv)
