"""Generation rules (biogpt_hip_generate_beam_rules, biogpt_hip_generate_sample_rules, biogpt_hip_rules_rows_device) without a GPU: the C-ABI is
exported and bound, the struct has the documented layout, argument checks come before any HIP call and name the field, and the new kernels hold
everything in registers and LDS (no scratch)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("biogpt_hip_generate_beam_rules", "biogpt_hip_generate_sample_rules", "biogpt_hip_rules_rows_device")


def test_rules_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    assert hasattr(pkg, "rules_rows")
    import inspect
    for fn in (pkg.BiogptModel.generate_beam, pkg.BiogptModel.generate_sample):
        p = inspect.signature(fn).parameters
        assert p["repetition_penalty"].default == 1.0 and p["no_repeat_ngram_size"].default == 0
        assert p["min_new_tokens"].default == 0 and tuple(p["suppress_tokens"].default) == ()


def test_rules_struct_layout(pkg):
    """typedef struct { float; int32_t; int32_t; int32_t; const int32_t *; } biogpt_hip_gen_rules -- as the header spells it."""
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    m = re.search(r"typedef struct biogpt_hip_gen_rules \{(.*?)\} biogpt_hip_gen_rules;", hdr, re.S)
    assert m
    fields = re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(\w+);", m.group(1), re.M)
    assert [(t.replace(" ", ""), n) for t, n in fields] == [("float", "repetition_penalty"), ("int32_t", "no_repeat_ngram_size"), ("int32_t", "min_new_tokens"),
                                                            ("int32_t", "n_suppress"), ("constint32_t*", "suppress")]
    R = pkg.GenRules
    assert [n for n, _ in R._fields_] == [n for _, n in fields]
    assert (R.repetition_penalty.offset, R.no_repeat_ngram_size.offset, R.min_new_tokens.offset, R.n_suppress.offset, R.suppress.offset) == (0, 4, 8, 12, 16)
    assert ctypes.sizeof(R) == 24
    r, keep = pkg.gen_rules(1.25, 3, 7, [5, 9])
    assert (r.repetition_penalty, r.no_repeat_ngram_size, r.min_new_tokens, r.n_suppress, r.suppress[0], r.suppress[1]) == (1.25, 3, 7, 2, 5, 9)
    r, keep = pkg.gen_rules()
    assert (r.repetition_penalty, r.no_repeat_ngram_size, r.min_new_tokens, r.n_suppress) == (1.0, 0, 0, 0) and not r.suppress


def test_rules_generation_null_context_fails_without_a_device(pkg):
    L = pkg.lib()
    prompt = np.array([2, 5, 7], dtype=np.int32)
    ids = np.zeros((4, 8), dtype=np.int32)
    lens = np.zeros(4, dtype=np.int32)
    sc = np.zeros(4, dtype=np.float32)
    secs = ctypes.c_double(0.0)
    r, keep = pkg.gen_rules(1.2, 3, 4, [9])
    assert L.biogpt_hip_generate_beam_rules(None, prompt.ctypes.data, 3, 8, 4, 8, 2, 1.0, 1, ids.ctypes.data, lens.ctypes.data, sc.ctypes.data,
                                            ctypes.byref(secs), ctypes.byref(r)) == -1
    assert "null context" in pkg._err()
    pl = np.array([3], dtype=np.int32)
    seeds = np.array([1, 2], dtype=np.uint32)
    assert L.biogpt_hip_generate_sample_rules(None, prompt.ctypes.data, pl.ctypes.data, 1, 2, 8, 8, 40, 0.9, 0.9, seeds.ctypes.data, -1, ids.ctypes.data,
                                              lens.ctypes.data, ctypes.byref(secs), ctypes.byref(r)) == -1
    assert "null context" in pkg._err()
    assert L.biogpt_hip_generate_beam_rules(None, prompt.ctypes.data, 3, 8, 4, 8, 2, 1.0, 1, ids.ctypes.data, lens.ctypes.data, sc.ctypes.data,
                                            ctypes.byref(secs), None) == -1


# (keyword arguments of gen_rules / the raw struct, the field the message must name) -- shared with test_gpu_rules.py
BAD_RULES = [
    (dict(repetition_penalty=0.0), "repetition_penalty"),
    (dict(repetition_penalty=-1.5), "repetition_penalty"),
    (dict(repetition_penalty=math.nan), "repetition_penalty"),
    (dict(repetition_penalty=math.inf), "repetition_penalty"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
    (dict(min_new_tokens=-1), "min_new_tokens"),
    (dict(suppress_tokens=list(range(257))), "n_suppress"),
    (dict(suppress_tokens=[3, 96]), "suppress"),
    (dict(suppress_tokens=[-1]), "suppress"),
]


def rows_device(pkg, r, mode=0):
    rows = np.zeros((2, 96), dtype=np.float32)
    hist = np.array([2, 5, 7, 2, 9], dtype=np.int32)
    hl, pl = np.array([3, 2], dtype=np.int32), np.array([2, 2], dtype=np.int32)
    out = np.zeros_like(rows)
    return pkg.lib().biogpt_hip_rules_rows_device(0, mode, rows.ctypes.data, 2, 96, hist.ctypes.data, hl.ctypes.data, pl.ctypes.data, 4,
                                                  ctypes.byref(r) if r is not None else None, out.ctypes.data)


@pytest.mark.parametrize("kw,field", BAD_RULES, ids=[f + "_%d" % i for i, (_, f) in enumerate(BAD_RULES)])
def test_rules_argument_errors_come_before_any_hip_call(pkg, kw, field):
    """No device on this machine: a call that reached HIP would return -2, not -1."""
    r, keep = pkg.gen_rules(**kw)
    assert rows_device(pkg, r) == -1
    assert field in pkg._err(), pkg._err()


def test_rules_struct_errors_the_python_helper_cannot_build(pkg):
    r, keep = pkg.gen_rules()
    r.n_suppress = -1
    assert rows_device(pkg, r) == -1 and "n_suppress" in pkg._err()
    r.n_suppress = 3      # NULL suppress with n_suppress > 0
    assert rows_device(pkg, r) == -1 and "suppress" in pkg._err() and "NULL" in pkg._err()
    r, keep = pkg.gen_rules(1.2)
    for mode in (-1, 2):
        assert rows_device(pkg, r, mode) == -1 and "mode" in pkg._err()
    assert rows_device(pkg, None) == -1 and "null argument" in pkg._err()


def test_rules_kernels_use_no_scratch(pkg, tmp_path):
    """rules_rows_kernel and beam_group_rows_kernel over processed log-probabilities (<8 / 16 / 32, true>): the kernel descriptors in obj/engine.o, read as test_beam_capi.py reads
    the beam kernels'."""
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
        if m and name and re.search(r"rules_rows_kernel|beam_group_rows_kernelILi\d+ELb1E", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 4, seen      # rules_rows_kernel, beam_group_rows_kernel<8 / 16 / 32, true>
