"""Build libkgan_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libkgan_hip.so")
SOURCES = ["kg_conv.hip", "kg_wgrad.hip", "kg_agg.hip", "kg_aggconv.hip", "kg_gen.hip", "kg_genblock.hip", "kg_disc.hip", "kg_map.hip", "kg_comm.hip", "kg_misc.hip", "kg_mmd.hip", "kg_input.hip", "kg_sample.hip", "kg_eval.hip", "kg_prdc.hip", "kg_frechet.hip", "kg_cls.hip", "kg_nn.hip", "kg_nn_gram.hip", "kg_kin.hip", "kg_proj.hip"]


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(ROOT, "include", "kgan_hip.h")]
    return any(os.path.getmtime(d) > t for d in deps)


LIB_ASAN = os.path.join(PKG, "libkgan_hip_asan.so")
# the persistent LDS-ring form of kg_conv (round 5; never selected by the plan): out of the default build, compiled in by
# `python kinetic-gan_amd/build.py --with-ring` or KG_WITH_RING=1 for its tests (tests/test_kernels_gpu.py, KG_TEST_RING=1)
RING_SOURCE = os.path.join(ROOT, "tools", "probe", "kg_conv_ring.hip")


def _with_ring() -> bool:
    return os.environ.get("KG_WITH_RING", "0") == "1" or "--with-ring" in sys.argv


def build_asan() -> str:
    """Host-side AddressSanitizer build: the library's host code - argument validation, launch plans,
    workspace sizing, job tables - instrumented with -fsanitize=address; device code is compiled as usual (GPU ASAN
    needs xnack+ targets, which this pool does not run).  Used by tests/test_abi_cpu.py through a small C driver
    (tests/asan_host_check.c) that exercises every entry point that does not launch; never shipped or benchmarked."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address", "-shared-libsan",
           "-Wno-option-ignored", "-std=c++17", "-fPIC", "-shared", "-mllvm", "-amdgpu-mfma-vgpr-form",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", LIB_ASAN] + [os.path.join(CSRC, s) for s in SOURCES] + ["-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc (asan) failed:\n" + r.stdout + r.stderr)
    return LIB_ASAN


last_action = None      # "compiled" / "reused" - what the last build() call did (reported by __graft_entry__.build)


def build(force: bool = False, verbose: bool = False) -> str:
    global last_action
    if not force and not _stale():
        last_action = "reused"      # an up-to-date prebuilt libkgan_hip.so (e.g. pushed to the GPU box with the tree)
        return LIB
    last_action = "compiled"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -amdgpu-mfma-vgpr-form: keep MFMA accumulators in VGPRs (gfx950 has one unified register file).  With
    # the default AGPR form hipcc copied every accumulator AGPR->VGPR->AGPR around each K-slice of the GEMM
    # loops (480 v_accvgpr_read/write in kg_conv), which also forces each slice to wait for its MFMAs.
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-mllvm", "-amdgpu-mfma-vgpr-form",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "-o", LIB] + [os.path.join(CSRC, s) for s in SOURCES] + ["-ldl"]
    if _with_ring():
        cmd += ["-DKG_WITH_RING", RING_SOURCE]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stdout + r.stderr)
    if verbose:
        sys.stderr.write(r.stderr)
    return LIB


if __name__ == "__main__":
    if "--asan" in sys.argv:
        print(build_asan())
    else:
        print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
