"""Beam search over a batch of prompts (biogpt_hip_generate_beam_batch) without a GPU: the C-ABI is exported and bound, argument checks
come before any HIP call, the beam kernels hold everything in registers and LDS (no scratch), and the kernels the other suites count
are still the ones they count."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_beam_batch_symbol_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    assert re.search(r"\bbiogpt_hip_generate_beam_batch\s*\(", hdr)
    assert "biogpt_hip_generate_beam_batch" in bound
    assert getattr(raw, "biogpt_hip_generate_beam_batch") is not None
    assert pkg.lib().biogpt_hip_generate_beam_batch.restype is ctypes.c_int
    assert hasattr(pkg.BiogptModel, "generate_beam_batch")


def test_beam_batch_null_context_fails_without_a_device(pkg):
    """No device on this machine: a call that reached HIP would return -2, not -1."""
    L = pkg.lib()
    prompts = np.array([2, 5, 7, 2, 9], dtype=np.int32)
    lens = np.array([3, 2], dtype=np.int32)
    ids = np.zeros((2, 4, 8), dtype=np.int32)
    ol = np.zeros((2, 4), dtype=np.int32)
    sc = np.zeros((2, 4), dtype=np.float32)
    counts = np.zeros(2, dtype=np.int32)
    secs = ctypes.c_double(0.0)
    assert L.biogpt_hip_generate_beam_batch(None, prompts.ctypes.data, lens.ctypes.data, 2, 8, 4, 8, 2, 1.0, 1, None, ids.ctypes.data, ol.ctypes.data,
                                            sc.ctypes.data, counts.ctypes.data, ctypes.byref(secs)) == -1
    assert "null context" in pkg._err()


def kernel_scratch(pkg, tmp_path):
    """{kernel name: private_segment_fixed_size} of obj/engine.o, read as test_beam_capi.py reads it."""
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
    name, out = None, {}
    for line in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name:
            out[name] = int(m.group(1))
    return out


def test_beam_batch_kernels_use_no_scratch(pkg, tmp_path):
    """beam_group_rows_kernel<8 / 16 / 32> over logits and over processed log-probabilities, beam_group_select_kernel, kv_group_fork_kernel."""
    ks = {n: v for n, v in kernel_scratch(pkg, tmp_path).items() if re.search(r"beam_group_rows_kernel|beam_group_select_kernel|kv_group_fork_kernel", n)}
    for n, v in ks.items():
        assert v == 0, "%s uses %d bytes of scratch per lane" % (n, v)
    assert len(ks) == 8, sorted(ks)


def test_existing_kernel_counts_are_unchanged(pkg, tmp_path):
    """What test_beam_capi.py, test_rules_capi.py and test_sample_capi.py count by name: no other kernel's name adds to any of them."""
    names = list(kernel_scratch(pkg, tmp_path))
    count = lambda pat: len({n for n in names if re.search(pat, n)})
    assert count(r"beam_group_rows_kernel|beam_group_select_kernel|kv_group_fork_kernel") == 8
    assert count(r"rules_rows_kernel|beam_group_rows_kernelILi\d+ELb1E") == 4
    assert count(r"sample_rows_kernel|kv_share_kernel") == 2
