"""Beam search (biogpt_hip_generate_beam) without a GPU: the C-ABI is exported and bound, argument checks come before any HIP call,
and the beam kernels hold everything in registers and LDS (no scratch)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_beam_symbol_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    assert re.search(r"\bbiogpt_hip_generate_beam\s*\(", hdr)
    assert "biogpt_hip_generate_beam" in bound
    assert getattr(raw, "biogpt_hip_generate_beam") is not None
    assert pkg.lib().biogpt_hip_generate_beam.restype is ctypes.c_int
    assert hasattr(pkg.BiogptModel, "generate_beam")


def test_beam_null_context_fails_without_a_device(pkg):
    L = pkg.lib()
    prompt = np.array([2, 5, 7], dtype=np.int32)
    ids = np.zeros((4, 8), dtype=np.int32)
    lens = np.zeros(4, dtype=np.int32)
    sc = np.zeros(4, dtype=np.float32)
    secs = ctypes.c_double(0.0)
    assert L.biogpt_hip_generate_beam(None, prompt.ctypes.data, 3, 8, 4, 8, 2, 1.0, 1, ids.ctypes.data, lens.ctypes.data, sc.ctypes.data,
                                      ctypes.byref(secs)) == -1
    assert "null context" in pkg._err()


def test_beam_kernels_use_no_scratch(pkg, tmp_path):
    """beam_group_rows_kernel (every instantiation), beam_group_select_kernel and kv_group_fork_kernel: the kernel descriptors in obj/engine.o,
    read as test_score_capi.py reads logprob_rows_kernel's."""
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
    name, seen = None, set()
    for line in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name and re.search(r"beam_group_rows_kernel|beam_group_select_kernel|kv_group_fork_kernel", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 8, seen      # beam_group_rows_kernel<8 / 16 / 32, false / true>, beam_group_select_kernel, kv_group_fork_kernel
