"""Trie-constrained generation (biogpt_hip_trie_*, biogpt_hip_generate_beam_trie, biogpt_hip_generate_sample_trie, biogpt_hip_trie_rows_device) without a
GPU: the C-ABI is exported and bound, the host trie equals trie_ref on the shapes a build and a walk can go wrong on, argument errors come before any
HIP call and name the field, trie_rows_kernel uses no scratch, and the host code runs clean under the address and undefined-behaviour sanitizers as a
stand-alone program."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import trie_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "biogpt.cpp_amd", "csrc")
NAMES = ("biogpt_hip_trie_build", "biogpt_hip_trie_free", "biogpt_hip_trie_info", "biogpt_hip_trie_allowed_host", "biogpt_hip_generate_beam_trie",
         "biogpt_hip_generate_sample_trie", "biogpt_hip_trie_rows_device", "biogpt_hip_beam_rows_masked_device")


def test_trie_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
        getattr(pkg.lib(), name)
    assert hasattr(pkg, "Trie") and hasattr(pkg, "trie_rows")
    for fn in (pkg.BiogptModel.generate_beam, pkg.BiogptModel.generate_beam_batch, pkg.BiogptModel.generate_sample):
        assert inspect.signature(fn).parameters["trie"].default is None
    assert inspect.signature(pkg.beam_rows).parameters["masked"].default is False


def test_host_trie_is_no_hip_code():
    """csrc/trie_host.{h,cpp} include no HIP header and are part of the library."""
    for f in ("trie_host.h", "trie_host.cpp"):
        assert not re.search(r"#include\s*[<\"]hip", open(os.path.join(CSRC, f)).read()), f
    assert re.search(r"^SRCS\s*=.*\btrie_host\.cpp\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)


@pytest.mark.parametrize("V", [42384, 42383, 1001, 96, 33])
def test_build_info_allowed_equal_the_restatement(pkg, V):
    rng = np.random.default_rng(V)
    for name, entries in trie_ref.shape_tries(V).items():
        ref = trie_ref.RefTrie(entries)
        t = pkg.Trie.build(entries, V)
        assert t.info() == ref.info(), name
        for which in ("first", "last", "mid"):
            eos = trie_ref.unused_token(entries, V, which)
            for h in trie_ref.probe_histories(entries, V, rng):
                got = t.allowed(h, eos)
                assert list(got) == ref.allowed(h, eos), (name, which, h)
                assert len(got) >= 1
        t.close()
    fans = {n: trie_ref.RefTrie(e).info()["max_fanout"] for n, e in trie_ref.shape_tries(V).items() if n.startswith("fan")}
    assert all(f == int(n[3:]) for n, f in fans.items()), fans
    if V >= 42383:
        assert sorted(fans.values()) == [1, 255, 256, 257, 4097]


def test_random_tries_equal_the_restatement(pkg):
    """Random entries over a small pool: many shared prefixes, duplicates and entries that are prefixes of others; EOS inside the pool's range."""
    rng = np.random.default_rng(5)
    for V, pool, n in ((96, 6, 300), (1001, 50, 200), (42384, 3, 500)):
        toks = rng.choice(np.arange(1, V), pool, replace=False)
        entries = [[int(t) for t in rng.choice(toks, int(rng.integers(1, 7)))] for _ in range(n)]
        ref = trie_ref.RefTrie(entries)
        t = pkg.Trie.build(entries, V)
        assert t.info() == ref.info()
        assert t.info()["entries"] < n      # duplicates merged
        assert any(tuple(e[:k]) in ref.entries for e in ref.entries for k in range(1, len(e)))      # prefix entries
        eos = trie_ref.unused_token(entries, V, "mid")
        for h in trie_ref.probe_histories(entries, V, rng, n=40):
            assert list(t.allowed(h, eos)) == ref.allowed(h, eos), h
        t.close()


# ---- argument errors: -1 and the field, without a device (a call that reached HIP would return -2 on this machine) ----

def _build_raw(pkg, seqs, lens, n, V, null_seqs=False, null_lens=False):
    s, l = np.asarray(seqs, dtype=np.int32), np.asarray(lens, dtype=np.int32)
    return pkg.lib().biogpt_hip_trie_build(None if null_seqs else s.ctypes.data, None if null_lens else l.ctypes.data, n, V)


@pytest.mark.parametrize("kw,field", [(dict(n=0), "n_seqs"), (dict(lens=[2, 0]), "lens"), (dict(lens=[2, -1]), "lens"), (dict(seqs=[1, 2, 10]), "seqs"),
                                      (dict(seqs=[1, -1, 3]), "seqs"), (dict(null_seqs=True), "seqs"), (dict(null_lens=True), "lens"), (dict(V=0), "n_vocab")])
def test_build_errors_name_the_argument(pkg, kw, field):
    args = dict(seqs=[1, 2, 3], lens=[2, 1], n=2, V=10)
    args.update(kw)
    assert not _build_raw(pkg, **args)
    assert field in pkg._err(), pkg._err()
    with pytest.raises(pkg.BiogptError):
        pkg.Trie.build([[1], []], 10)
    with pytest.raises(pkg.BiogptError):
        pkg.Trie.build([], 10)


def test_info_and_allowed_errors(pkg):
    L = pkg.lib()
    t = pkg.Trie.build([[1, 2], [3]], 10)
    g = np.array([1], dtype=np.int32)
    out = np.zeros(4, dtype=np.int32)
    info = (ctypes.c_int64 * 5)()
    assert L.biogpt_hip_trie_info(None, info) == -1 and "trie" in pkg._err()
    assert L.biogpt_hip_trie_info(t._h, None) == -1 and "out" in pkg._err()
    for args, field in (((None, g.ctypes.data, 1, 9, out.ctypes.data, 4), "trie"), ((t._h, None, 1, 9, out.ctypes.data, 4), "gen"),
                        ((t._h, g.ctypes.data, -1, 9, out.ctypes.data, 4), "n_gen"), ((t._h, g.ctypes.data, 1, 10, out.ctypes.data, 4), "eos_id"),
                        ((t._h, g.ctypes.data, 1, -1, out.ctypes.data, 4), "eos_id"), ((t._h, g.ctypes.data, 1, 9, None, 4), "out_ids"),
                        ((t._h, g.ctypes.data, 1, 9, out.ctypes.data, -1), "cap")):
        assert L.biogpt_hip_trie_allowed_host(*args) == -1, field
        assert field in pkg._err(), (field, pkg._err())
    assert L.biogpt_hip_trie_allowed_host(t._h, g.ctypes.data, 1, 9, out.ctypes.data, 0) == 1      # the size alone
    t.close()
    t.close()      # twice is harmless
    with pytest.raises(pkg.BiogptError, match="open Trie"):
        pkg.trie_rows(np.zeros((1, 10), np.float32), t, [[]])


def call_generate(pkg, which, trie, eos, ctx=None):
    L = pkg.lib()
    prompt = np.array([2, 5, 7], dtype=np.int32)
    pl = np.array([3], dtype=np.int32)
    ids, lens, sc, cnt = np.zeros((4, 8), np.int32), np.zeros(4, np.int32), np.zeros(4, np.float32), np.zeros(1, np.int32)
    seeds = np.array([1, 2], dtype=np.uint32)
    secs = ctypes.c_double(0.0)
    if which == "beam":
        return L.biogpt_hip_generate_beam_trie(ctx, prompt.ctypes.data, pl.ctypes.data, 1, 8, 4, 8, eos, 1.0, 1, trie, ids.ctypes.data, lens.ctypes.data,
                                               sc.ctypes.data, cnt.ctypes.data, ctypes.byref(secs))
    return L.biogpt_hip_generate_sample_trie(ctx, prompt.ctypes.data, pl.ctypes.data, 1, 2, 8, 8, 1, 0.9, 0.9, seeds.ctypes.data, eos, trie, ids.ctypes.data,
                                             lens.ctypes.data, ctypes.byref(secs))


@pytest.mark.parametrize("which", ["beam", "sample"])
def test_generation_argument_errors_come_before_any_hip_call(pkg, which):
    t = pkg.Trie.build([[1, 2], [3]], 10)
    assert call_generate(pkg, which, None, 9) == -1 and "trie" in pkg._err()
    assert call_generate(pkg, which, t._h, -1) == -1 and "eos_id" in pkg._err()
    assert call_generate(pkg, which, t._h, 10) == -1 and "eos_id" in pkg._err()
    assert call_generate(pkg, which, t._h, 2) == -1 and "eos_id" in pkg._err() and "entry" in pkg._err()      # EOS inside an entry
    assert call_generate(pkg, which, t._h, 9) == -1 and "null context" in pkg._err()
    t.close()


def call_rows(pkg, trie, rows=True, hist=True, out=True, mode=0, n_rows=2, n_vocab=10, eos=9, tokens=(1, 2, 3), lens=(2, 1)):
    a = np.zeros((max(n_rows, 1), n_vocab), dtype=np.float32)
    h, hl = np.asarray(tokens, dtype=np.int32), np.asarray(lens, dtype=np.int32)
    o = np.zeros_like(a)
    return pkg.lib().biogpt_hip_trie_rows_device(0, trie, mode, a.ctypes.data if rows else None, n_rows, n_vocab, h.ctypes.data if hist else None, hl.ctypes.data,
                                                 eos, o.ctypes.data if out else None)


@pytest.mark.parametrize("kw,field", [(dict(rows=False), "rows"), (dict(hist=False), "hist"), (dict(out=False), "rows_out"), (dict(mode=2), "mode"),
                                      (dict(mode=-1), "mode"), (dict(n_rows=0), "n_rows"), (dict(n_rows=4097), "n_rows"), (dict(eos=-1), "eos_id"),
                                      (dict(eos=10), "eos_id"), (dict(eos=3), "eos_id"), (dict(n_vocab=11), "n_vocab"), (dict(tokens=(1, 10, 3)), "hist"),
                                      (dict(lens=(2, -1)), "hist_lens")])
def test_rows_argument_errors_come_before_any_hip_call(pkg, kw, field):
    t = pkg.Trie.build([[1, 2], [3]], 10)
    assert call_rows(pkg, t._h, **kw) == -1
    assert field in pkg._err(), pkg._err()
    assert call_rows(pkg, None) == -1 and "trie" in pkg._err()
    t.close()


def test_python_routes_and_refuses_rules_with_a_trie(pkg):
    t = pkg.Trie.build([[1, 2], [3]], 10)
    m = pkg.BiogptModel.__new__(pkg.BiogptModel)      # no context: the checks in front of the C call
    m._h = None
    for call in (lambda: m.generate_beam([2, 5], 4, trie=t, repetition_penalty=1.2), lambda: m.generate_beam_batch([[2, 5]], 4, trie=t, no_repeat_ngram_size=2),
                 lambda: m.generate_sample([[2, 5]], 4, trie=t, eos_id=9, suppress_tokens=[4])):
        with pytest.raises(pkg.BiogptError, match="rules together with a trie"):
            call()
    with pytest.raises(pkg.BiogptError, match="null context"):
        m.generate_beam_batch([[2, 5]], 4, eos_id=9, trie=t)
    with pytest.raises(pkg.BiogptError, match="eos_id"):
        m.generate_sample([[2, 5]], 4, trie=t)      # the default: no EOS id
    with pytest.raises(pkg.BiogptError, match="open Trie"):
        m.generate_sample([[2, 5]], 4, eos_id=9, trie="names.txt")
    t.close()


def test_trie_kernel_uses_no_scratch(pkg, tmp_path):
    """trie_rows_kernel: the kernel descriptor in obj/engine.o, read as test_rules_capi.py reads the rules kernel's."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(llvm + "/clang-offload-bundler") and shutil.which("objcopy")):
        pytest.skip("no clang-offload-bundler / objcopy in this image")
    pkg.build()
    path = os.path.join(CSRC, "obj", "engine.o")
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
        if m and name and "trie_rows_kernel" in name:
            seen[name] = int(m.group(1))
    assert len(seen) == 1, seen
    assert list(seen.values()) == [0], "trie_rows_kernel uses %s bytes of scratch per lane" % list(seen.values())


def test_host_trie_runs_clean_under_sanitizers(tmp_path):
    """csrc/trie_host.cpp (+ the error plumbing of model_file.cpp) and tests/trie_host_main.cpp, a program of its own, built with
    -fsanitize=address,undefined and run as a subprocess on the CPU: build, walks, the bad inputs, free."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program: nothing about how it is started matters to them
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "trie_host_main")
    srcs = [os.path.join(ROOT, "tests", "trie_host_main.cpp"), os.path.join(CSRC, "trie_host.cpp"), os.path.join(CSRC, "model_file.cpp")]
    r = subprocess.run([cxx] + flags + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
