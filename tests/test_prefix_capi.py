"""Shared-prefix scoring (biogpt_hip_score_continuations) without a GPU: the C-ABI is exported and bound, the argument checks that need no
model come before any HIP call, the Python wrappers exist, and every instantiation of attn_fast_kernel -- the three that were there and the
three that read a column's first rows from a shared slot -- holds everything in registers and LDS (no scratch)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "biogpt_hip_score_continuations"


def test_prefix_symbol_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    assert re.search(r"\b%s\s*\(" % NAME, hdr)
    assert NAME in bound
    assert getattr(raw, NAME) is not None
    assert getattr(pkg.lib(), NAME).restype is ctypes.c_int


def test_prefix_python_wrappers_exist(pkg):
    p = inspect.signature(pkg.BiogptModel.score_continuations).parameters
    assert list(p) == ["self", "prefix", "continuations"]
    p = inspect.signature(pkg.BiogptModel.rank_continuations).parameters
    assert list(p) == ["self", "prefix", "continuations", "normalize"] and p["normalize"].default is False


def test_prefix_null_context_fails_without_a_device(pkg):
    """No device on this machine and no context: a call that reached HIP would not return -1 with this message."""
    pre = np.array([2, 5, 7], dtype=np.int32)
    conts = np.array([9, 11, 4], dtype=np.int32)
    lens = np.array([2, 1], dtype=np.int32)
    out = np.zeros(3, dtype=np.float32)
    secs = ctypes.c_double(-1.0)
    rc = pkg.lib().biogpt_hip_score_continuations(None, pre.ctypes.data, 3, conts.ctypes.data, lens.ctypes.data, 2, out.ctypes.data, None, None,
                                                  ctypes.byref(secs))
    assert rc == -1
    assert "null context" in pkg._err()
    assert secs.value == -1.0 and (out == 0).all()
    assert pkg.lib().biogpt_hip_score_continuations(None, None, 0, None, None, 0, None, None, None, None) == -1
    assert "null context" in pkg._err()


def test_attention_instantiations_use_no_scratch(pkg, tmp_path):
    """attn_fast_kernel<1,true> / <2,false> / <4,false>, each plain and SHARED: the kernel descriptors in obj/engine.o, read as
    test_score_capi.py reads the log-softmax kernel's.  Six instantiations, none with a private segment."""
    llvm = "/opt/rocm/lib/llvm/bin"
    # the build itself needs ROCm: without its tools this check must fail, not vanish
    assert os.path.exists(llvm + "/clang-offload-bundler") and os.path.exists(llvm + "/llvm-readelf"), "no ROCm LLVM tools under " + llvm
    assert shutil.which("objcopy"), "no objcopy on PATH"
    pkg.build()
    path = os.path.join(ROOT, "biogpt.cpp_amd", "csrc", "obj", "engine.o")
    assert os.path.exists(path), path
    fat, co = str(tmp_path / "engine.fatbin"), str(tmp_path / "engine.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    notes = subprocess.check_output([llvm + "/llvm-readelf", "--notes", co], text=True)
    name, seen = None, {}
    for line in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name and "attn_fast_kernel" in name:
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen[name] = True
    # Itanium mangling of the template arguments <int KP, bool VPRE, bool SHARED>: ILi<KP>ELb<VPRE>ELb<SHARED>EE
    args = sorted(re.search(r"attn_fast_kernelILi(\d)ELb([01])ELb([01])EE", n).groups() for n in seen)
    plain = [a[:2] for a in args if a[2] == "0"]
    shared = [a[:2] for a in args if a[2] == "1"]
    assert plain == [("1", "1"), ("2", "0"), ("4", "0")], args
    assert shared == plain, args
    assert len(seen) == 6, sorted(seen)
