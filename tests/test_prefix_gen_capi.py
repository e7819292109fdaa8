"""Generation behind a shared prefix (biogpt_hip_generate_greedy_prefix / biogpt_hip_generate_sample_prefix / biogpt_hip_prefix_stats) without a
GPU: the C-ABI is exported and bound, `prefix` is the last argument of the two Python wrappers and changes nothing where it is not given, the
checks that need no model come before any HIP call, the new kernels hold everything in registers and LDS, and the host restatement of the call's
layout (prefix_gen_ref.py) keeps every chunk of a concatenation on one side of the shared rows."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import prefix_gen_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["biogpt_hip_generate_greedy_prefix", "biogpt_hip_generate_sample_prefix", "biogpt_hip_prefix_stats", "biogpt_hip_attn_prefix_device",
         "biogpt_hip_attn_prefix_bench"]


@pytest.mark.parametrize("name", NAMES)
def test_prefix_gen_symbols_exported_and_bound(pkg, name):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {n for n, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in bound
    assert getattr(raw, name) is not None
    assert getattr(pkg.lib(), name).restype is ctypes.c_int


def test_prefix_is_the_last_python_argument(pkg):
    p = inspect.signature(pkg.BiogptModel.generate_greedy_batch).parameters
    assert list(p) == ["self", "prompts", "n_predict", "n_batch", "prefix"] and p["prefix"].default is None
    p = inspect.signature(pkg.BiogptModel.generate_sample).parameters
    assert list(p) == ["self", "prompts", "n_predict", "n_samples", "top_k", "top_p", "temp", "seed", "seeds", "eos_id", "n_batch", "repetition_penalty",
                       "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens", "trie", "prefix"]
    assert p["prefix"].default is None
    assert list(inspect.signature(pkg.BiogptModel.prefix_stats).parameters) == ["self"]


def test_prefix_gen_null_context_fails_without_a_device(pkg):
    """No device on this machine and no context: a call that reached HIP would not return -1 with this message."""
    pre = np.array([2, 5, 7], dtype=np.int32)
    suf = np.array([9, 11, 4], dtype=np.int32)
    lens = np.array([2, 1], dtype=np.int32)
    seeds = np.array([1, 2], dtype=np.uint32)
    out = np.full((2, 4), 77, dtype=np.int32)
    ol = np.full(2, 77, dtype=np.int32)
    secs = ctypes.c_double(-1.0)
    L = pkg.lib()
    assert L.biogpt_hip_generate_greedy_prefix(None, pre.ctypes.data, 3, suf.ctypes.data, lens.ctypes.data, 2, 8, 4, out.ctypes.data, ctypes.byref(secs)) == -1
    assert "null context" in pkg._err()
    assert L.biogpt_hip_generate_sample_prefix(None, pre.ctypes.data, 3, suf.ctypes.data, lens.ctypes.data, 2, 1, 8, 4, 40, 0.9, 0.9, seeds.ctypes.data, -1,
                                               out.ctypes.data, ol.ctypes.data, ctypes.byref(secs)) == -1
    assert "null context" in pkg._err()
    assert secs.value == -1.0 and (out == 77).all() and (ol == 77).all()
    st = np.full(4, 77, dtype=np.int32)
    assert L.biogpt_hip_prefix_stats(None, st.ctypes.data) == -1
    assert "null context" in pkg._err() and (st == 77).all()
    assert L.biogpt_hip_generate_greedy_prefix(None, None, 0, None, None, 0, 0, 0, None, None) == -1
    assert "null context" in pkg._err()


def test_prefix_with_trie_or_rules_raises_without_a_model(pkg):
    """The check needs neither a model nor the library: `self` is never looked at."""
    f = pkg.BiogptModel.generate_sample
    with pytest.raises(ValueError, match="trie"):
        f(None, [[5]], 4, trie=object(), prefix=[2, 7], eos_id=2)
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=3), dict(suppress_tokens=[5])):
        with pytest.raises(ValueError, match="rules"):
            f(None, [[5]], 4, prefix=[2, 7], **kw)


def test_prefix_kernels_use_no_scratch(pkg, tmp_path):
    """The descriptors of attn_prefix_kernel<8>, kv_prefix_copy_kernel and kv_share_kernel in obj/engine.o, read as test_prefix_capi.py reads those of
    attn_fast_kernel (whose six instantiations that test still counts: the new kernel's name does not contain theirs)."""
    llvm = "/opt/rocm/lib/llvm/bin"
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
        if m and name and ("kv_prefix_copy_kernel" in name or "kv_share_kernel" in name or "attn_prefix_kernel" in name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen[name] = True
    assert len(seen) == 3 and all(any(k in n for n in seen) for k in ("kv_prefix_copy_kernel", "kv_share_kernel", "attn_prefix_kernelILi8EE")), sorted(seen)


# ---- the host restatement of the layout ----

@pytest.mark.parametrize("n_batch", range(1, 10))
@pytest.mark.parametrize("n_prefix", range(1, 21))
def test_chunks_of_the_concatenation_never_straddle_the_shared_rows(n_prefix, n_batch):
    lens = [0, 1, 2, 7, 40]
    lay = ref.layout(n_prefix, n_batch, lens)
    k = lay["n_shared"]
    assert k % n_batch == 0 and 0 <= k <= n_prefix - 1 and k + n_batch > n_prefix - 1
    assert lay["columns"] == len(lens)
    assert lay["prompt_columns"] == k + sum(n_prefix - k + n for n in lens)
    prefix = list(range(100, 100 + n_prefix))
    eff = ref.effective_prompts(prefix, [[7] * n for n in lens], n_batch)
    for s, n in enumerate(lens):
        assert len(eff[s]) >= 1 and prefix[:k] + eff[s] == prefix + [7] * n
        whole = ref.chunks(n_prefix + n, n_batch)
        assert all(e <= k or b >= k for b, e in whole), (whole, k)
        # the shared chunks, then the sequence's own, are the concatenation's chunks one for one
        assert lay["shared_chunks"] + lay["own_chunks"][s] == whole
