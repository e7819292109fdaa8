"""Sequence scoring (biogpt_hip_score / biogpt_hip_score_batch) without a GPU: the C-ABI is exported and bound, argument checks come
before any HIP call, and the log-softmax kernel holds everything in registers and LDS (no scratch)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("biogpt_hip_score", "biogpt_hip_score_batch"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int


def test_score_null_context_fails_without_a_device(pkg):
    L = pkg.lib()
    toks = np.array([2, 5, 7], dtype=np.int32)
    lens = np.array([3], dtype=np.int32)
    out = np.zeros(3, dtype=np.float32)
    assert L.biogpt_hip_score(None, toks.ctypes.data, 3, 0, None, out.ctypes.data, None, None) == -1
    assert "null context" in pkg._err()
    assert L.biogpt_hip_score_batch(None, toks.ctypes.data, lens.ctypes.data, 1, None, out.ctypes.data, None, None) == -1
    assert "null context" in pkg._err()


def test_logprob_kernel_uses_no_scratch(pkg, tmp_path):
    """logprob_rows_kernel: the kernel descriptor in obj/engine.o, read as test_pass_kernels_use_no_scratch reads the pass kernels'."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(llvm + "/clang-offload-bundler") and shutil.which("objcopy")):
        pytest.skip("no clang-offload-bundler / objcopy in this image")
    pkg.build()
    path = os.path.join(ROOT, "biogpt.cpp_amd", "csrc", "obj", "engine.o")
    assert os.path.exists(path), path
    fat, co = str(tmp_path / "engine.fatbin"), str(tmp_path / "engine.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([llvm + "/llvm-readelf", "--notes", co], text=True)
    name, seen = None, 0
    for line in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name and "logprob_rows_kernel" in name:
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen += 1
    assert seen == 1
