"""Log-probabilities of generated tokens (biogpt_hip_generate_greedy_batch_lp, biogpt_hip_generate_sample_lp, biogpt_hip_genlp_rows_device) without a
GPU: the C-ABI and the struct are exported and bound, every mistake in the request returns -1 with a message that names the field before any HIP call
(the request is checked in front of the context: no device, no context here -- n_top > n_vocab needs a vocabulary and is checked through the
kernel-alone entry, whose n_vocab is an argument), the Python layer refuses logprobs= with a trie or rules, logprobs=None leaves the calls as they
were, and the two selection kernels hold everything in registers and LDS."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("biogpt_hip_generate_greedy_batch_lp", "biogpt_hip_generate_sample_lp", "biogpt_hip_genlp_rows_device")


def test_symbols_and_struct_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    m = re.search(r"typedef struct biogpt_hip_gen_logprobs \{(.*?)\} biogpt_hip_gen_logprobs;", hdr, re.S)
    assert m, "struct biogpt_hip_gen_logprobs"
    fields = re.findall(r"(int32_t|float)\s*(\*?)\s*(\w+);", m.group(1))
    assert fields == [("int32_t", "", "n_top"), ("float", "*", "lp"), ("int32_t", "*", "top_ids"), ("float", "*", "top_lp")], fields
    assert [f[0] for f in pkg.GenLogprobs._fields_] == ["n_top", "lp", "top_ids", "top_lp"]
    assert ctypes.sizeof(pkg.GenLogprobs) == 8 + 3 * ctypes.sizeof(ctypes.c_void_p)      # the int, its padding, three pointers


class Buffers:
    def __init__(self):
        self.prompt = np.array([2, 5, 7], dtype=np.int32)
        self.lens = np.array([3], dtype=np.int32)
        self.seeds = np.array([1, 2], dtype=np.uint32)
        self.ids = np.zeros((2, 8), dtype=np.int32)
        self.ol = np.zeros(2, dtype=np.int32)
        self.lp = np.zeros((2, 8), dtype=np.float32)
        self.tid = np.zeros((2, 8, 8), dtype=np.int32)
        self.tlp = np.zeros((2, 8, 8), dtype=np.float32)
        self.secs = ctypes.c_double(0.0)

    def request(self, pkg, n_top=5, lp=True, top_ids=True, top_lp=True):
        return pkg.GenLogprobs(n_top, self.lp.ctypes.data if lp else None, self.tid.ctypes.data if top_ids else None, self.tlp.ctypes.data if top_lp else None)


def call(pkg, which, b, req, prefix=None, n_prefix=0):
    L = pkg.lib()
    ref = None if req is None else ctypes.byref(req)
    if which == "greedy":
        return L.biogpt_hip_generate_greedy_batch_lp(None, prefix, n_prefix, b.prompt.ctypes.data, b.lens.ctypes.data, 1, 8, 8, b.ids.ctypes.data, ctypes.byref(b.secs), ref)
    return L.biogpt_hip_generate_sample_lp(None, prefix, n_prefix, b.prompt.ctypes.data, b.lens.ctypes.data, 1, 2, 8, 8, 40, 0.9, 0.9, b.seeds.ctypes.data, -1,
                                           b.ids.ctypes.data, b.ol.ctypes.data, ctypes.byref(b.secs), ref)


REQUEST_ERRORS = [(dict(lp=False), "logprobs.lp"), (dict(n_top=-1), "n_top"), (dict(n_top=9), "n_top"), (dict(top_ids=False), "top_ids"),
                  (dict(top_lp=False), "top_lp"), (dict(n_top=1, top_ids=False), "top_ids"), (dict(n_top=8, top_lp=False), "top_lp")]


@pytest.mark.parametrize("which", ["greedy", "sample"])
def test_request_errors_come_before_the_context_and_any_hip_call(pkg, which):
    b = Buffers()
    assert call(pkg, which, b, None) == -1 and "logprobs" in pkg._err(), pkg._err()
    for kw, field in REQUEST_ERRORS:
        assert call(pkg, which, b, b.request(pkg, **kw)) == -1, kw
        assert field in pkg._err(), (kw, pkg._err())
    # a sound request: the next thing wrong is named -- the context, and with a prefix its pointers, n_prefix without one
    for req in (b.request(pkg), b.request(pkg, n_top=0, top_ids=False, top_lp=False), b.request(pkg, n_top=8)):
        assert call(pkg, which, b, req) == -1 and "null context" in pkg._err(), pkg._err()
    assert call(pkg, which, b, b.request(pkg), None, 3) == -1 and "n_prefix" in pkg._err(), pkg._err()
    assert call(pkg, which, b, b.request(pkg), b.prompt.ctypes.data, 3) == -1 and "null context" in pkg._err(), pkg._err()


def rows_call(pkg, mode=0, rows=True, n_rows=2, n_vocab=10, n_top=3, top_k=4, top_p=0.9, temp=0.9, states=True, ids=True, lp=True, top_ids=True, top_lp=True):
    a = np.zeros((max(n_rows, 1), max(n_vocab, 1)), dtype=np.float32)
    st = np.zeros((max(n_rows, 1), 625), dtype=np.uint32)
    o_id, o_lp = np.zeros(max(n_rows, 1), np.int32), np.zeros(max(n_rows, 1), np.float32)
    o_ti, o_tl = np.zeros((max(n_rows, 1), 8), np.int32), np.zeros((max(n_rows, 1), 8), np.float32)
    return pkg.lib().biogpt_hip_genlp_rows_device(0, mode, a.ctypes.data if rows else None, n_rows, n_vocab, n_top, top_k, top_p, temp, st.ctypes.data if states else None,
                                                  o_id.ctypes.data if ids else None, o_lp.ctypes.data if lp else None, o_ti.ctypes.data if top_ids else None,
                                                  o_tl.ctypes.data if top_lp else None)


@pytest.mark.parametrize("kw,field", [(dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(rows=False), "rows"), (dict(ids=False), "ids_out"), (dict(n_rows=0), "n_rows"),
                                      (dict(n_rows=4097), "n_rows"), (dict(n_vocab=0), "n_vocab"), (dict(lp=False), "logprobs.lp"), (dict(n_top=-1), "n_top"),
                                      (dict(n_top=9), "n_top"), (dict(top_ids=False), "top_ids"), (dict(top_lp=False), "top_lp"),
                                      (dict(n_vocab=4, n_top=5), "n_vocab"), (dict(n_vocab=7, n_top=8, mode=1), "n_vocab"),
                                      (dict(mode=1, states=False), "mt_states"), (dict(mode=1, top_k=0), "top_k"), (dict(mode=1, top_k=65), "top_k"),
                                      (dict(mode=1, top_k=11), "top_k"), (dict(mode=1, temp=0.0), "temp"), (dict(mode=1, top_p=float("inf")), "top_p")])
def test_rows_entry_argument_errors_come_before_any_hip_call(pkg, kw, field):
    assert rows_call(pkg, **kw) == -1
    assert field in pkg._err(), pkg._err()


def test_n_top_beyond_the_vocabulary_names_both(pkg):
    assert rows_call(pkg, n_vocab=4, n_top=5) == -1
    assert "n_top (5)" in pkg._err() and "n_vocab (4)" in pkg._err(), pkg._err()


def test_python_refuses_logprobs_with_a_trie_or_rules(pkg):
    t = pkg.Trie.build([[1, 2], [3]], 10)
    m = pkg.BiogptModel.__new__(pkg.BiogptModel)      # no context: the checks in front of the C call
    m._h = None
    with pytest.raises(ValueError, match="trie"):
        m.generate_sample([[2, 5]], 4, eos_id=9, trie=t, logprobs=2)
    for rules in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=3), dict(suppress_tokens=[4])):
        with pytest.raises(ValueError, match="rules"):
            m.generate_sample([[2, 5]], 4, logprobs=0, **rules)
    for bad in (-1, 9):
        with pytest.raises(ValueError, match="logprobs"):
            m.generate_sample([[2, 5]], 4, logprobs=bad)
        with pytest.raises(ValueError, match="logprobs"):
            m.generate_greedy_batch([[2, 5]], 4, logprobs=bad)
    # a sound request reaches the C call, which names the missing context; with and without a prefix
    for kw in (dict(), dict(prefix=[2, 9, 4])):
        with pytest.raises(pkg.BiogptError, match="null context"):
            m.generate_sample([[2, 5]], 4, logprobs=3, **kw)
        with pytest.raises(pkg.BiogptError, match="null context"):
            m.generate_greedy_batch([[2, 5]], 4, logprobs=3, **kw)
    t.close()


def test_logprobs_none_leaves_the_calls_as_they_were(pkg, monkeypatch):
    """logprobs is a keyword behind every parameter the methods had, None by default; the methods' own signatures are what they were (introspection
    reports them: the keyword is added around them), and without it the calls go to the entry points they went to and return two values."""
    for name in ("generate_greedy_batch", "generate_sample"):
        fn = getattr(pkg.BiogptModel, name)
        outer = inspect.signature(fn, follow_wrapped=False).parameters
        assert outer["logprobs"].kind is inspect.Parameter.KEYWORD_ONLY and outer["logprobs"].default is None, name
        own = list(inspect.signature(fn).parameters)
        assert own[-1] == "prefix" and "logprobs" not in own, name
        assert "logprobs" in fn.__doc__
    called = []

    class Lib:
        def __getattr__(self, name):
            def fn(*args):
                called.append(name)
                return 0      # "n_predict clamped to 0": nothing generated
            return fn

    monkeypatch.setattr(pkg, "lib", lambda: Lib())
    m = pkg.BiogptModel.__new__(pkg.BiogptModel)
    m._h = None
    for kw, entry, entry_lp in ((dict(), "biogpt_hip_generate_greedy_batch", "biogpt_hip_generate_greedy_batch_lp"),
                                (dict(prefix=[2, 3]), "biogpt_hip_generate_greedy_prefix", "biogpt_hip_generate_greedy_batch_lp")):
        del called[:]
        assert len(m.generate_greedy_batch([[2, 5]], 4, **kw)) == 2 and called == [entry]
        assert len(m.generate_greedy_batch([[2, 5]], 4, logprobs=None, **kw)) == 2 and called == [entry] * 2
        out = m.generate_greedy_batch([[2, 5]], 4, logprobs=2, **kw)
        assert len(out) == 3 and called[-1] == entry_lp
        assert out[0].shape == (1, 0) and len(out[1]) == 1 and [a.shape for a in out[1][0]] == [(0,), (0, 2), (0, 2)]
    for kw, entry in ((dict(), "biogpt_hip_generate_sample_rules"), (dict(prefix=[2, 3]), "biogpt_hip_generate_sample_prefix")):
        del called[:]
        assert len(m.generate_sample([[2, 5]], 4, **kw)) == 2 and called == [entry]
        assert len(m.generate_sample([[2, 5]], 4, logprobs=None, **kw)) == 2 and called == [entry] * 2
        assert len(m.generate_sample([[2, 5]], 4, logprobs=0, **kw)) == 3 and called[-1] == "biogpt_hip_generate_sample_lp"


def test_genlp_kernels_use_no_scratch(pkg, tmp_path):
    """genlp_greedy_rows_kernel and sample_lp_rows_kernel: the kernel descriptors in obj/engine.o, read as test_sample_capi.py reads the sampler's."""
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
        if m and name and re.search(r"genlp_greedy_rows_kernel|sample_lp_rows_kernel", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 2, seen
