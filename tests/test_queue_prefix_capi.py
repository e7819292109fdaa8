"""Queued generation behind a shared prefix, with log-probabilities (biogpt_hip_generate_queue_prefix, biogpt_hip_queue_rows_device) without a GPU: the
entry points are exported and bound with the declared signatures; every argument error that can be judged without a model returns -1 and names its field
before any HIP call, with no context and no device -- first the log-probability request, then the pointers, the counts and the prompts; the records the
host and the kernels share keep their sizes; the Python wrapper keeps generate_queue's own parameters and adds two keywords."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = ctypes.c_void_p
NAMES = ("biogpt_hip_generate_queue_prefix", "biogpt_hip_queue_rows_device")


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
    assert bound["biogpt_hip_generate_queue_prefix"][1] == [_P, _P, i32, _P, _P, i32, _P, i32, i32, i32, i32, i32, f64, f64, _P, i32, _P, _P, _P, _P, ctypes.POINTER(f64),
                                                            ctypes.POINTER(pkg.QueueStats), ctypes.POINTER(pkg.GenLogprobs)]
    decl = re.search(r"int biogpt_hip_generate_queue_prefix\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "prefix", "n_prefix", "suffixes", "suffix_lens", "n_requests", "n_predicts", "n_predict",
                                                                     "max_columns", "group", "n_batch", "top_k", "top_p", "temp", "seeds", "eos_id", "out_ids",
                                                                     "out_lens", "out_admit_step", "out_column", "seconds_out", "stats", "logprobs"]
    decl = re.search(r"int biogpt_hip_queue_rows_device\((.*?)\);", hdr, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 20 == len(bound["biogpt_hip_queue_rows_device"][1])
    assert callable(pkg.queue_rows)


def test_struct_sizes(pkg):
    """The structs of the interface as the header lays them out, and the records host and kernels share as the kernel header states them: QueueAdmit keeps
    its 32 bytes with the shared rows and their slot in two of its three pad words."""
    assert ctypes.sizeof(pkg.QueueStats) == 40 and pkg.QueueStats.busy_column_steps.offset == 24
    assert [n for n, _ in pkg.GenLogprobs._fields_] == ["n_top", "lp", "top_ids", "top_lp"]
    assert ctypes.sizeof(pkg.GenLogprobs) == 32 and pkg.GenLogprobs.lp.offset == 8
    src = open(os.path.join(ROOT, "biogpt.cpp_amd", "csrc", "kernels_queue.hip.h")).read()
    body = re.search(r"struct QueueAdmit \{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    words = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(int32_t|uint32_t)\s+(.*)$", decl, re.S)
        assert m, decl
        for name in m.group(2).split(","):
            arr = re.match(r"\s*(\w+)\s*\[(\d+)\]\s*$", name)
            words += [arr.group(1)] * int(arr.group(2)) if arr else [name.strip()]
    assert words == ["col", "last_token", "len", "limit", "seed", "n_shared", "shared_slot", "pad"], words
    assert 4 * len(words) == 32
    assert "static_assert(sizeof(QueueAdmit) == 32" in src


def call(pkg, ctx=None, prefix=(2, 11, 12), n_prefix=None, suffixes=True, lens=(3, 2), tokens=(5, 7, 9, 6, 8), n_requests=2, n_predicts=None, n_predict=8, max_columns=4,
         group=4, n_batch=8, top_k=40, top_p=0.9, temp=0.9, seeds=True, eos_id=-1, ids=True, ol=True, suffix_lens=True, logprobs=None):
    """logprobs: None, or (n_top, lp?, top_ids?, top_lp?) -- which of the three arrays the request names."""
    pf = None if prefix is None else np.array(prefix, dtype=np.int32)
    sx = np.array(tokens, dtype=np.int32)
    ln = np.array(lens, dtype=np.int32)
    sd = np.array([1, 2], dtype=np.uint32)
    npr = None if n_predicts is None else np.array(n_predicts, dtype=np.int32)
    out = np.zeros((2, 8), dtype=np.int32)
    lens_out, adm, col = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    secs = ctypes.c_double(0.0)
    st = pkg.QueueStats()
    req = None
    if logprobs is not None:
        k, has_lp, has_ids, has_top = logprobs
        a_lp, a_ids, a_top = np.zeros((2, 8), np.float32), np.zeros((2, 8, 8), np.int32), np.zeros((2, 8, 8), np.float32)
        req = pkg.GenLogprobs(k, a_lp.ctypes.data if has_lp else None, a_ids.ctypes.data if has_ids else None, a_top.ctypes.data if has_top else None)
    rc = pkg.lib().biogpt_hip_generate_queue_prefix(ctx, None if pf is None else pf.ctypes.data, (0 if pf is None else len(pf)) if n_prefix is None else n_prefix,
                                                    sx.ctypes.data if suffixes else None, ln.ctypes.data if suffix_lens else None, n_requests,
                                                    None if npr is None else npr.ctypes.data, n_predict, max_columns, group, n_batch, top_k, top_p, temp,
                                                    sd.ctypes.data if seeds else None, eos_id, out.ctypes.data if ids else None, lens_out.ctypes.data if ol else None,
                                                    adm.ctypes.data, col.ctypes.data, ctypes.byref(secs), ctypes.byref(st), None if req is None else ctypes.byref(req))
    return rc, pkg._err()


@pytest.mark.parametrize("kw, field", [
    # everything in order: the context is what is missing, with and without a prefix, with and without log-probabilities, behind an empty suffix
    (dict(), "null context"), (dict(prefix=None), "null context"), (dict(logprobs=(5, 1, 1, 1)), "null context"), (dict(prefix=None, logprobs=(0, 1, 0, 0)), "null context"),
    (dict(lens=(0, 2), tokens=(6, 8)), "null context"),
    # null pointers
    (dict(suffixes=False), "null argument: suffixes"), (dict(suffix_lens=False), "null argument: suffix_lens"), (dict(seeds=False), "seeds"), (dict(ids=False), "out_ids"),
    (dict(ol=False), "out_lens"), (dict(prefix=None, suffixes=False), "null argument: prompts"), (dict(prefix=None, suffix_lens=False), "null argument: prompt_lens"),
    # counts and sizes
    (dict(n_requests=0), "n_requests must be >= 1"), (dict(n_requests=-3), "n_requests"),
    (dict(max_columns=0), "max_columns must be in [1, 511] behind a prefix"), (dict(max_columns=512), "max_columns must be in [1, 511] behind a prefix (got 512)"),
    (dict(prefix=None, max_columns=513), "max_columns must be in [1, 512]"),
    (dict(group=65), "group must be in [1, 64]"), (dict(group=0), "group must be in [1, 64]"), (dict(n_batch=0), "n_batch"), (dict(n_predict=-1), "n_predict"),
    (dict(n_predicts=(3, 9)), "n_predicts[1]"),
    (dict(top_k=0), "top_k"), (dict(temp=0.0), "temp"), (dict(top_p=float("nan")), "top_p"), (dict(eos_id=-2), "eos_id"),
    # the prompts
    (dict(lens=(3, -1)), "suffix_lens[1] (-1) is negative"), (dict(tokens=(5, 7, 9, -4, 8)), "token id -4 (request 1, position 0)"),
    (dict(prefix=(2, -7, 12)), "token id -7 (prefix, position 1)"),
    (dict(prefix=None, lens=(3, 0), tokens=(5, 7, 9)), "empty prompt (request 1)"),
    # the prefix and its length
    (dict(n_prefix=0), "n_prefix must be >= 1 (got 0)"), (dict(n_prefix=-2), "n_prefix must be >= 1 (got -2)"),
    (dict(prefix=None, n_prefix=3), "n_prefix must be 0 without a prefix (got 3)"),
    # the log-probability request: named first, whatever else is wrong
    (dict(logprobs=(5, 0, 1, 1)), "null argument: logprobs.lp"), (dict(logprobs=(-1, 1, 1, 1)), "logprobs.n_top must be in [0, 8] (got -1)"),
    (dict(logprobs=(9, 1, 1, 1)), "logprobs.n_top must be in [0, 8] (got 9)"), (dict(logprobs=(3, 1, 0, 1)), "null argument: logprobs.top_ids"),
    (dict(logprobs=(3, 1, 1, 0)), "null argument: logprobs.top_lp"),
    (dict(logprobs=(5, 0, 1, 1), suffixes=False, n_requests=0), "null argument: logprobs.lp"), (dict(logprobs=(-1, 1, 1, 1), group=65), "logprobs.n_top"),
])
def test_argument_errors_come_before_any_device_call(pkg, kw, field):
    """No device on this machine and no context: a call that reached HIP would return -2, not -1."""
    rc, msg = call(pkg, **kw)
    assert rc == -1, (rc, msg)
    assert field in msg, msg


def test_errors_come_in_the_order_of_the_tiers(pkg):
    """Each call is wrong in everything from its tier on: the message names the first."""
    wrong = [(dict(suffixes=False), "suffixes"), (dict(n_requests=0), "n_requests"), (dict(group=65), "group"), (dict(lens=(3, -1)), "suffix_lens[1]")]
    for i, (_, field) in enumerate(wrong):
        kw = {}
        for later, _ in wrong[i:]:
            kw.update(later)
        rc, msg = call(pkg, **kw)
        assert rc == -1 and field in msg, (i, msg)


def rows_call(pkg, **kw):
    n, nv = 2, 16
    a = dict(with_lp=1, rows=True, n_rows=n, n_vocab=nv, n_top=2, stride=1, top_k=4, top_p=0.9, temp=0.9, eos_id=-1, mt=True, states=True, limits=True, finished=True,
             hdr=True, ids=True, lp=True, mt_index=0)
    a.update(kw)
    rows = np.zeros((n, nv), np.float32)
    mt = np.zeros((n, 625), np.uint32)
    mt[:, 624] = a["mt_index"]
    states, limits, fin, hdr = np.zeros((n, 8), np.int32), np.ones(n, np.int32), np.zeros(n, np.int32), np.zeros(1 + 2 * n, np.int32)
    ids, lp, tid, tlp = np.zeros((n, 1), np.int32), np.zeros((n, 1), np.float32), np.zeros((n, 1, 8), np.int32), np.zeros((n, 1, 8), np.float32)
    p = lambda arr, on: arr.ctypes.data if on else None
    rc = pkg.lib().biogpt_hip_queue_rows_device(0, a["with_lp"], p(rows, a["rows"]), a["n_rows"], a["n_vocab"], a["n_top"], a["stride"], a["top_k"], a["top_p"], a["temp"],
                                                a["eos_id"], p(mt, a["mt"]), p(states, a["states"]), p(limits, a["limits"]), p(fin, a["finished"]), p(hdr, a["hdr"]),
                                                p(ids, a["ids"]), p(lp, a["lp"]), tid.ctypes.data, tlp.ctypes.data)
    return rc, pkg._err()


@pytest.mark.parametrize("kw, field", [
    (dict(rows=False), "rows"), (dict(mt=False), "mt_states"), (dict(states=False), "states"), (dict(limits=False), "limits"), (dict(finished=False), "finished"),
    (dict(hdr=False), "hdr"), (dict(ids=False), "ids_out"), (dict(lp=False), "logprobs.lp"), (dict(n_rows=0), "n_rows"), (dict(n_rows=513), "n_rows"),
    (dict(n_vocab=0), "n_vocab"), (dict(stride=0), "stride"), (dict(n_top=9), "n_top"), (dict(n_top=-1), "n_top"), (dict(top_k=0), "top_k"), (dict(top_k=17), "top_k"),
    (dict(temp=0.0), "temp"), (dict(top_p=float("inf")), "top_p"), (dict(eos_id=16), "eos_id"), (dict(mt_index=625), "generator index"),
])
def test_probe_argument_errors_come_before_any_device_call(pkg, kw, field):
    rc, msg = rows_call(pkg, **kw)
    assert rc == -1, (rc, msg)
    assert field in msg, msg


def _words(addr, n, ctype):
    return [int(v) for v in np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctype)), (n,))]


class FakeLib:
    """Stands where the library is: keeps which entry point a call took and its arguments (the arrays copied while they live), and answers as a run of no
    eligible request would."""
    def __init__(self):
        self.name = self.args = self.prefix = self.lens = self.tokens = self.n_top = None

    def biogpt_hip_generate_queue(self, *args):
        self.name, self.args = "plain", args
        return 0

    def biogpt_hip_generate_queue_prefix(self, *args):
        self.name, self.args = "prefix", args
        R = args[5]
        self.prefix = None if args[1] is None else _words(args[1], args[2], ctypes.c_int32)
        self.lens = _words(args[4], R, ctypes.c_int32)
        self.tokens = _words(args[3], sum(self.lens), ctypes.c_int32)
        self.n_top = None if args[22] is None else int(args[22]._obj.n_top)
        return 0


def test_python_wrapper_keywords(pkg, monkeypatch):
    """generate_queue's own parameters are what they were; prefix and logprobs are keywords behind them, and without either the call is today's."""
    sig = inspect.signature(pkg.BiogptModel.generate_queue)
    assert list(sig.parameters)[1:] == ["prompts", "n_predict", "max_columns", "group", "top_k", "top_p", "temp", "seed", "seeds", "eos_id", "n_batch", "n_predicts"]
    fake = FakeLib()
    monkeypatch.setattr(pkg, "lib", lambda: fake)
    model = pkg.BiogptModel.__new__(pkg.BiogptModel)
    model._h = None
    ids, info, secs = model.generate_queue([[2, 5, 7], [2, 9]], 6)
    assert fake.name == "plain" and len(fake.args) == 20 and set(info) == {"stats", "admit_step", "column"}
    ids, info, secs = model.generate_queue([[5, 7], [], [9]], 6, prefix=[2, 11, 12], max_columns=3, group=2, top_k=40, n_batch=4)
    assert fake.name == "prefix" and fake.prefix == [2, 11, 12] and fake.args[2] == 3 and fake.lens == [2, 0, 1] and fake.tokens == [5, 7, 9] and fake.n_top is None
    assert fake.args[5] == 3 and fake.args[7:12] == (6, 3, 2, 4, 40) and set(info) == {"stats", "admit_step", "column"}
    ids, info, secs = model.generate_queue([[2, 5, 7], [2, 9]], 6, logprobs=5)
    assert fake.name == "prefix" and fake.prefix is None and fake.args[2] == 0 and fake.n_top == 5 and fake.tokens == [2, 5, 7, 2, 9]
    assert len(info["logprobs"]) == 2 and [a.shape for a in info["logprobs"][0]] == [(0,), (0, 5), (0, 5)]
    model.generate_queue([[5]], 6, prefix=[2, 3], logprobs=0)
    assert fake.prefix == [2, 3] and fake.n_top == 0
    with pytest.raises(ValueError, match="logprobs"):
        model.generate_queue([[5]], 6, logprobs=9)


def test_queue_lp_kernel_uses_no_scratch(pkg, tmp_path):
    """queue_rows_lp_kernel: the kernel descriptor in obj/engine.o, read as test_queue_capi.py reads the plain kernels'."""
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
        if m and name and re.search(r"queue_rows_lp_kernel", name):
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (name, m.group(1))
            seen.add(name)
    assert len(seen) == 1, seen
