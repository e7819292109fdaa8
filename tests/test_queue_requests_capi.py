"""Queued generation with request parameters (biogpt_hip_generate_queue_requests, biogpt_hip_queue_req_rows_device) without a GPU: the entry points are
exported and bound with the declared signatures; biogpt_hip_request_params has the size the Python Structure says; every argument error that can be judged
without a model returns -1 and names its field and the request before any HIP call, with no context and no device; log-probabilities together with a rule
are refused by name; the Python wrapper adds one keyword and keeps the others."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = ctypes.c_void_p
NAMES = ("biogpt_hip_generate_queue_requests", "biogpt_hip_queue_req_rows_device")


def test_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert name in bound
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    i32, f64 = ctypes.c_int32, ctypes.c_double
    assert bound["biogpt_hip_generate_queue_requests"][1] == [_P, _P, i32, _P, _P, i32, _P, i32, i32, i32, i32, ctypes.POINTER(pkg.RequestParams), _P, _P, _P, _P, _P, _P,
                                                              ctypes.POINTER(f64), ctypes.POINTER(pkg.QueueStats), ctypes.POINTER(pkg.GenLogprobs)]
    decl = re.search(r"int biogpt_hip_generate_queue_requests\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "prefix", "n_prefix", "prompts", "prompt_lens", "n_requests", "n_predicts", "n_predict",
                                                                     "max_columns", "group", "n_batch", "params", "seeds", "out_ids", "out_lens", "out_finish",
                                                                     "out_admit_step", "out_column", "seconds_out", "stats", "logprobs"]
    decl = re.search(r"int biogpt_hip_queue_req_rows_device\((.*?)\);", hdr, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 20 == len(bound["biogpt_hip_queue_req_rows_device"][1])
    assert callable(pkg.queue_req_rows) and callable(pkg.request_params)


def test_struct_sizes(pkg):
    """biogpt_hip_request_params as the header lays it out (two words, two doubles, the rules with their pointer, a count and two pointers); the records host
    and kernels share keep what the kernel header states: QueueAdmit its 32 bytes, the request record a multiple of 16."""
    rp = pkg.RequestParams
    assert [n for n, _ in rp._fields_] == ["top_k", "eos_id", "top_p", "temp", "rules", "n_stop", "stop", "stop_lens"]
    assert ctypes.sizeof(pkg.GenRules) == 24
    assert ctypes.sizeof(rp) == 72 and (rp.top_p.offset, rp.temp.offset, rp.rules.offset, rp.n_stop.offset, rp.stop.offset, rp.stop_lens.offset) == (8, 16, 24, 48, 56, 64)
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    body = re.search(r"typedef struct biogpt_hip_request_params \{(.*?)\} biogpt_hip_request_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [piece.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert names == ["top_k", "eos_id", "top_p", "temp", "rules", "n_stop", "stop", "stop_lens"], names
    src = open(os.path.join(ROOT, "biogpt.cpp_amd", "csrc", "kernels_queue.hip.h")).read()
    eng = open(os.path.join(ROOT, "biogpt.cpp_amd", "csrc", "engine.hip")).read()      # the C side holds the same numbers at compile time
    assert "static_assert(sizeof(biogpt_hip_request_params) == %d && offsetof(biogpt_hip_request_params, rules) == %d && offsetof(biogpt_hip_request_params, stop) == %d" % (
        ctypes.sizeof(rp), rp.rules.offset, rp.stop.offset) in eng
    assert "static_assert(sizeof(QueueAdmit) == 32" in src and "static_assert(sizeof(QueueReqRec) % 16 == 0" in src
    for name, value in (("QUEUE_REQ_SUPPRESS", 64), ("QUEUE_REQ_STOPS", 4), ("QUEUE_REQ_STOP_LEN", 8)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name


GOOD = dict(top_k=40, top_p=0.95, temp=6.0)


def call(pkg, params=None, ctx=None, prefix=None, n_prefix=None, prompts=True, lens=(3, 2), tokens=(5, 7, 9, 6, 8), n_requests=2, n_predicts=None, n_predict=8,
         max_columns=4, group=4, n_batch=8, seeds=True, ids=True, ol=True, prompt_lens=True, logprobs=None, null_params=False, finish=True):
    """params: one dict of request_params() arguments per request (None: GOOD for both).  logprobs: None, or (n_top, lp?, top_ids?, top_lp?)."""
    entries = [pkg.request_params(**(p if p is not None else GOOD)) for p in (params if params is not None else [None, None])]
    arr, keep = pkg._params_array(entries, len(entries))
    pf = None if prefix is None else np.array(prefix, dtype=np.int32)
    sx = np.array(tokens, dtype=np.int32)
    ln = np.array(lens, dtype=np.int32)
    sd = np.array([1, 2], dtype=np.uint32)
    npr = None if n_predicts is None else np.array(n_predicts, dtype=np.int32)
    out = np.zeros((2, 8), dtype=np.int32)
    lens_out, fin, adm, col = (np.zeros(2, dtype=np.int32) for _ in range(4))
    secs = ctypes.c_double(0.0)
    st = pkg.QueueStats()
    req = None
    if logprobs is not None:
        k, has_lp, has_ids, has_top = logprobs
        a_lp, a_ids, a_top = np.zeros((2, 8), np.float32), np.zeros((2, 8, 8), np.int32), np.zeros((2, 8, 8), np.float32)
        req = pkg.GenLogprobs(k, a_lp.ctypes.data if has_lp else None, a_ids.ctypes.data if has_ids else None, a_top.ctypes.data if has_top else None)
    rc = pkg.lib().biogpt_hip_generate_queue_requests(ctx, None if pf is None else pf.ctypes.data, (0 if pf is None else len(pf)) if n_prefix is None else n_prefix,
                                                      sx.ctypes.data if prompts else None, ln.ctypes.data if prompt_lens else None, n_requests,
                                                      None if npr is None else npr.ctypes.data, n_predict, max_columns, group, n_batch, None if null_params else arr,
                                                      sd.ctypes.data if seeds else None, out.ctypes.data if ids else None, lens_out.ctypes.data if ol else None,
                                                      fin.ctypes.data if finish else None, adm.ctypes.data, col.ctypes.data, ctypes.byref(secs), ctypes.byref(st),
                                                      None if req is None else ctypes.byref(req))
    return rc, pkg._err()


def second(**kw):
    """request 0 in order, request 1 with these parameters: the message must name params[1]"""
    return [None, dict(GOOD, **kw)]


@pytest.mark.parametrize("kw, field", [
    # everything in order: the context is what is missing -- with rules, stop sequences, a prefix, log-probabilities with stop sequences, no finish array
    (dict(), "null context"), (dict(prefix=(2, 11, 12)), "null context"), (dict(finish=False), "null context"),
    (dict(params=second(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=2, eos_id=2, suppress_tokens=range(4, 68), stop=[[5] * 8, [6], [7, 8], [9]])), "null context"),
    (dict(params=second(stop=[[5, 6]]), logprobs=(2, 1, 1, 1)), "null context"),
    (dict(params=second(min_new_tokens=3), logprobs=(0, 1, 0, 0)), "null context"),      # (min_new_tokens without an EOS id is no rule)
    # null pointers, counts and sizes: as the other queue calls
    (dict(prompts=False), "null argument: prompts"), (dict(prefix=(2, 3), prompts=False), "null argument: suffixes"), (dict(prompt_lens=False), "null argument: prompt_lens"),
    (dict(null_params=True), "null argument: params"), (dict(seeds=False), "seeds"), (dict(ids=False), "out_ids"), (dict(ol=False), "out_lens"),
    (dict(n_requests=0), "n_requests must be >= 1"), (dict(max_columns=513), "max_columns must be in [1, 512]"),
    (dict(prefix=(2, 3), max_columns=512), "max_columns must be in [1, 511] behind a prefix (got 512)"), (dict(group=65), "group must be in [1, 64]"),
    (dict(n_batch=0), "n_batch"), (dict(n_predict=-1), "n_predict"), (dict(n_predicts=(3, 9)), "n_predicts[1]"),
    (dict(n_prefix=3), "n_prefix must be 0 without a prefix (got 3)"), (dict(prefix=(2, 3), n_prefix=0), "n_prefix must be >= 1 (got 0)"),
    # the sampler of a request
    (dict(params=second(top_k=0)), "params[1].top_k must be in [1, 64]"), (dict(params=second(top_k=65)), "params[1].top_k must be in [1, 64]"),
    (dict(params=[dict(GOOD, top_k=0), None]), "params[0].top_k"),
    (dict(params=second(temp=0.0)), "params[1].temp must be finite and > 0"), (dict(params=second(temp=float("inf"))), "params[1].temp"),
    (dict(params=second(top_p=float("nan"))), "params[1].top_p must be finite"),
    (dict(params=second(eos_id=-2)), "params[1].eos_id -2 out of range"),
    # its rules, through check_rules
    (dict(params=second(repetition_penalty=0.0)), "params[1].rules: "), (dict(params=second(repetition_penalty=0.0)), "repetition_penalty must be finite and > 0"),
    (dict(params=second(repetition_penalty=float("nan"))), "repetition_penalty"),
    (dict(params=second(no_repeat_ngram_size=-1)), "no_repeat_ngram_size must be >= 0"), (dict(params=second(no_repeat_ngram_size=-1)), "params[1].rules"),
    (dict(params=second(min_new_tokens=-1)), "min_new_tokens must be >= 0"),
    (dict(params=second(suppress_tokens=[5, -3])), "suppress[1] = -3 out of range"), (dict(params=second(suppress_tokens=[5, -3])), "params[1].rules"),
    (dict(params=second(suppress_tokens=range(300))), "n_suppress must be in [0, 256]"),
    (dict(params=second(suppress_tokens=range(65))), "params[1].rules.n_suppress (65) must be in [0, 64]"),
    # its stop sequences
    (dict(params=second(stop=[[5]] * 5)), "params[1].n_stop (5) must be in [0, 4]"),
    (dict(params=second(stop=[[5], [6] * 9])), "params[1].stop_lens[1] (9) must be in [1, 8]"),
    (dict(params=second(stop=[[5], []])), "params[1].stop_lens[1] (0) must be in [1, 8]"),
    (dict(params=second(stop=[[5], [6, -7]])), "params[1].stop: token id -7 (sequence 1, position 1) out of range"),
    # log-probabilities with a rule switched on
    (dict(params=second(repetition_penalty=1.2), logprobs=(2, 1, 1, 1)), "logprobs with generation rules (params[1].rules"),
    (dict(params=second(no_repeat_ngram_size=2), logprobs=(0, 1, 0, 0)), "logprobs with generation rules"),
    (dict(params=second(min_new_tokens=2, eos_id=2), logprobs=(0, 1, 0, 0)), "logprobs with generation rules"),
    (dict(params=[dict(GOOD, suppress_tokens=[9]), None], logprobs=(0, 1, 0, 0)), "logprobs with generation rules (params[0].rules"),
    # the log-probability request itself is named first
    (dict(params=second(top_k=0), logprobs=(9, 1, 1, 1)), "logprobs.n_top must be in [0, 8] (got 9)"), (dict(logprobs=(2, 0, 1, 1)), "null argument: logprobs.lp"),
    # the prompts come behind the parameters
    (dict(lens=(3, 0), tokens=(5, 7, 9)), "empty prompt (request 1)"), (dict(tokens=(5, 7, 9, -4, 8)), "token id -4 (request 1, position 0)"),
    (dict(params=second(top_k=0), tokens=(5, 7, 9, -4, 8)), "params[1].top_k"),
])
def test_argument_errors_come_before_any_device_call(pkg, kw, field):
    rc, msg = call(pkg, **kw)
    assert rc == -1 and field in msg, (rc, msg)


def test_request_params_builder(pkg):
    p = pkg.request_params()
    assert (p.top_k, p.eos_id, p.top_p, p.temp, p.n_stop) == (1, -1, 0.9, 0.9, 0) and not p.stop and not p.stop_lens
    assert (p.rules.repetition_penalty, p.rules.no_repeat_ngram_size, p.rules.min_new_tokens, p.rules.n_suppress) == (1.0, 0, 0, 0)
    p = pkg.request_params(top_k=40, top_p=0.95, temp=6.0, eos_id=2, repetition_penalty=1.5, no_repeat_ngram_size=3, min_new_tokens=4, suppress_tokens=[7, 8],
                           stop=[[5, 6], [9]])
    assert (p.top_k, p.eos_id, p.top_p, p.temp, p.n_stop) == (40, 2, 0.95, 6.0, 2)
    assert [p.stop[i] for i in range(3)] == [5, 6, 9] and [p.stop_lens[i] for i in range(2)] == [2, 1]
    assert p.rules.repetition_penalty == 1.5 and [p.rules.suppress[i] for i in range(2)] == [7, 8]
    for bad in ([5, 6], [[5], 6], [[[5, 6]]]):      # ids where sequences belong: not silently two sequences of one id
        with pytest.raises(pkg.BiogptError, match="stop must be a list of id lists"):
            pkg.request_params(stop=bad)
    assert list(inspect.signature(pkg.request_params).parameters) == ["top_k", "top_p", "temp", "eos_id", "repetition_penalty", "no_repeat_ngram_size", "min_new_tokens",
                                                                      "suppress_tokens", "stop"]


class FakeLib:
    """Records which entry point generate_queue reaches and with what."""

    def __init__(self):
        self.name = None

    def biogpt_hip_generate_queue(self, *a):
        self.name, self.args = "plain", a
        return 0

    def biogpt_hip_generate_queue_prefix(self, *a):
        self.name, self.args = "prefix", a
        return 0

    def biogpt_hip_generate_queue_requests(self, *a):
        self.name, self.args = "requests", a
        self.params = [(a[11][i].top_k, a[11][i].eos_id, a[11][i].n_stop, a[11][i].rules.no_repeat_ngram_size) for i in range(a[5])]
        ctypes.cast(a[15], ctypes.POINTER(ctypes.c_int32))[0] = 3
        return 0


def test_python_wrapper_keyword(pkg, monkeypatch):
    """generate_queue's own parameters are what they were; params is a keyword behind them: without it the calls are today's, with it the new entry point gets
    one record per request and info gains "finish"; the method's own sampler values must then be left alone."""
    sig = inspect.signature(pkg.BiogptModel.generate_queue)
    assert list(sig.parameters)[1:] == ["prompts", "n_predict", "max_columns", "group", "top_k", "top_p", "temp", "seed", "seeds", "eos_id", "n_batch", "n_predicts"]
    fake = FakeLib()
    monkeypatch.setattr(pkg, "lib", lambda: fake)
    model = pkg.BiogptModel.__new__(pkg.BiogptModel)
    model._h = None
    ids, info, secs = model.generate_queue([[2, 5, 7], [2, 9]], 6)
    assert fake.name == "plain" and set(info) == {"stats", "admit_step", "column"}
    model.generate_queue([[5, 7]], 6, prefix=[2, 11, 12])
    assert fake.name == "prefix"
    one = pkg.request_params(top_k=40, eos_id=2, stop=[[5, 6]])
    ids, info, secs = model.generate_queue([[2, 5, 7], [2, 9]], 6, params=one, max_columns=3)
    assert fake.name == "requests" and len(fake.args) == 21 and fake.params == [(40, 2, 1, 0)] * 2 and fake.args[1] is None and fake.args[2] == 0 and fake.args[8] == 3
    assert set(info) == {"stats", "admit_step", "column", "finish"} and info["finish"] == [3, 0]
    ids, info, secs = model.generate_queue([[5, 7], [9]], 6, params=[one, pkg.request_params(no_repeat_ngram_size=3)], prefix=[2, 11], logprobs=2)
    assert fake.name == "requests" and fake.params == [(40, 2, 1, 0), (1, -1, 0, 3)] and fake.args[2] == 2 and fake.args[20] is not None
    assert set(info) == {"stats", "admit_step", "column", "finish", "logprobs"}
    for own in (dict(top_k=40), dict(top_p=0.5), dict(temp=1.0), dict(eos_id=2)):
        with pytest.raises(pkg.BiogptError, match="leave the method's own at their defaults"):
            model.generate_queue([[2, 5]], 6, params=one, **own)
    with pytest.raises(pkg.BiogptError, match="one entry per request"):
        model.generate_queue([[2, 5], [2, 6]], 6, params=[one])
    with pytest.raises(pkg.BiogptError, match="request_params"):
        model.generate_queue([[2, 5]], 6, params=[dict(top_k=1)])


def test_step_kernels_use_no_scratch(pkg, tmp_path):
    """queue_req_rows_kernel, both instances: the kernel descriptors in obj/engine.o, read as test_queue_prefix_capi.py reads queue_rows_lp_kernel's."""
    import shutil
    import subprocess
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
        if m and name and re.search(r"queue_req_rows_kernel", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 2, seen
