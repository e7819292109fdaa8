"""Sampled generation (biogpt_hip_generate_sample) without a GPU: the C-ABI is exported and bound, argument checks come before any HIP call, the
generator and the sampler's tail -- the text the kernel runs, through its host entry point -- equal oracle/sampler.py, and the kernels hold
everything in registers and LDS (no scratch)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("biogpt_hip_generate_sample", "biogpt_hip_sample_candidates_host", "biogpt_hip_mt19937_seed")


def test_sample_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES + ("biogpt_hip_sample_rows_device",):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    assert hasattr(pkg.BiogptModel, "generate_sample")


def test_sample_null_context_fails_without_a_device(pkg):
    L = pkg.lib()
    prompt = np.array([2, 5, 7], dtype=np.int32)
    lens = np.array([3], dtype=np.int32)
    seeds = np.array([1, 2], dtype=np.uint32)
    ids = np.zeros((2, 8), dtype=np.int32)
    ol = np.zeros(2, dtype=np.int32)
    secs = ctypes.c_double(0.0)
    assert L.biogpt_hip_generate_sample(None, prompt.ctypes.data, lens.ctypes.data, 1, 2, 8, 8, 40, 0.9, 0.9, seeds.ctypes.data, -1, ids.ctypes.data,
                                        ol.ctypes.data, ctypes.byref(secs)) == -1
    assert "null context" in pkg._err()


def seeded(pkg, seed):
    st = np.zeros(625, dtype=np.uint32)
    assert pkg.lib().biogpt_hip_mt19937_seed(seed, st.ctypes.data) == 0
    return st


def host_pick(pkg, vals, ids, top_p, temp, st):
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    out = ctypes.c_int32(-1)
    assert pkg.lib().biogpt_hip_sample_candidates_host(vals.ctypes.data, ids.ctypes.data, vals.size, top_p, temp, st.ctypes.data, ctypes.byref(out)) == 0, pkg._err()
    return int(out.value)


def temper(y):
    y ^= y >> 11
    y ^= (y << 7) & 0x9D2C5680
    y ^= (y << 15) & 0xEFC60000
    y ^= y >> 18
    return y & 0xFFFFFFFF


def test_mt19937_known_answer_through_the_hook(pkg):
    """std::mt19937(5489): the state after seeding is init_genrand's, and 4999 draws (two outputs each) through the host hook leave the state in front
    of the 9999th output -- the 10000th is 4123659995 (ISO C++ [rand.predef]); the draws themselves are the oracle's."""
    st = seeded(pkg, 5489)
    ref = sampler.Mt19937(5489)
    assert int(st[624]) == 624
    vals, ids = [0.0, 0.0], [0, 1]      # two equal candidates: partial sums {0.5, 1.0}, the pick is u > 0.5
    for _ in range(4999):
        u = sampler.generate_canonical_53(ref)
        assert host_pick(pkg, vals, ids, 1.0, 1.0, st) == (1 if u > 0.5 else 0)
    pos = int(st[624])
    assert pos == 9998 % 624
    assert temper(int(st[pos])) == ref()
    assert temper(int(st[pos + 1])) == 4123659995 == ref()


SETS = [(40, 0.9, 0.9), (40, 1.0, 1.0), (5, 0.5, 0.7), (1, 0.9, 0.9), (320, 0.95, 1.3), (64, 0.3, 0.5), (2, 0.9999, 1.0)]


@pytest.mark.parametrize("top_k,top_p,temp", SETS)
def test_host_tail_equals_restatement_on_random_logits(pkg, top_k, top_p, temp):
    """64 rows x 320 random logits (the recipe of test_host_sampler_equals_restatement_on_random_logits), candidates by stable arg-sort, ONE state
    carried across the rows: the ids and the final state are the oracle's (a draw consumed with one candidate left would shift the state)."""
    rng = np.random.default_rng(top_k * 131 + int(temp * 10))
    rows, nv = 64, 320
    lg = (rng.standard_normal((rows, nv)) * 2.5).astype(np.float32)
    fp, ft = float(np.float32(top_p)), float(np.float32(temp))
    k = top_k
    st = seeded(pkg, 7)
    ref = sampler.Mt19937(7)
    got, want = [], []
    for row in lg:
        order = np.argsort(-row.astype(np.float64), kind="stable")[:k]
        got.append(host_pick(pkg, row[order], order, fp, ft, st))
        want.append(sampler.sample_top_k_top_p(row, k, fp, ft, ref))
    assert got == want
    if k > 1:
        assert len(set(got)) > 4
    # the state: bring the oracle's generator to the same place by drawing what is left of the hook's block
    pos = int(st[624])
    assert all(temper(int(st[i])) == ref() for i in range(pos, 624))


def test_hook_rejects_bad_arguments(pkg):
    st = seeded(pkg, 1)
    vals, ids, out = np.zeros(4, np.float32), np.arange(4, dtype=np.int32), ctypes.c_int32(0)
    L = pkg.lib()
    for k, top_p, temp in ((0, 0.9, 0.9), (-1, 0.9, 0.9), (2, 0.9, 0.0), (2, 0.9, float("nan")), (2, float("inf"), 1.0)):
        assert L.biogpt_hip_sample_candidates_host(vals.ctypes.data, ids.ctypes.data, k, top_p, temp, st.ctypes.data, ctypes.byref(out)) == -1
    assert L.biogpt_hip_sample_candidates_host(None, ids.ctypes.data, 2, 0.9, 0.9, st.ctypes.data, ctypes.byref(out)) == -1


def test_sample_kernels_use_no_scratch(pkg, tmp_path):
    """sample_rows_kernel and kv_share_kernel: the kernel descriptors in obj/engine.o, read as test_beam_capi.py reads the beam kernels'."""
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
        if m and name and re.search(r"sample_rows_kernel|kv_share_kernel", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 2, seen
