"""Queue sessions (biogpt_hip_queue_open / _submit / _cancel / _poll / _session_stats / _close, biogpt_hip_queue_plan_script and the two kernel probes) without a
GPU: the entry points are declared, exported and bound with the declared signatures; the structs have the layout the Python Structures say; a null session and
a closed one are refused with a message; every refusal of the options that needs no model comes before any HIP call, with no context and no device.  (A
request's own n_predict is held against the session's: a session needs a device, so that refusal stands in tests/test_gpu_queue_session.py.)"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = ctypes.c_void_p
NAMES = {"biogpt_hip_queue_open": 2, "biogpt_hip_queue_submit": 6, "biogpt_hip_queue_cancel": 2, "biogpt_hip_queue_poll": 3, "biogpt_hip_queue_session_stats": 4,
         "biogpt_hip_queue_close": 1, "biogpt_hip_queue_plan_script": 11, "biogpt_hip_queue_stream_device": 13, "biogpt_hip_queue_cancel_device": 6}


def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name, n_args in NAMES.items():
        decl = re.search(r"^(?:int|int64_t|biogpt_hip_queue_session \*) ?%s\((.*?)\);" % name, hdr, re.S | re.M)
        assert decl, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == n_args == len(bound[name][1]), name
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is bound[name][0]
    assert bound["biogpt_hip_queue_open"][0] is _P and bound["biogpt_hip_queue_stream_device"][0] is ctypes.c_int64
    assert callable(pkg.queue_plan_script) and callable(pkg.queue_stream_rows) and callable(pkg.queue_cancel_cols)
    sig = inspect.signature(pkg.BiogptModel.queue_session)
    assert list(sig.parameters)[1:7] == ["max_columns", "group", "n_predict", "prefix", "logprobs", "stream"]
    for method in ("submit", "poll", "cancel", "drain", "stats", "close", "__enter__", "__exit__"):
        assert callable(getattr(pkg.QueueSession, method))
    assert list(inspect.signature(pkg.QueueSession.submit).parameters) == ["self", "prompt", "n_predict", "seed", "params"]
    assert inspect.signature(pkg.QueueSession.poll).parameters["max_groups"].default == 1


def struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [piece.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for piece in decl.split(",")]


def test_struct_layouts(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    o, e = pkg.QueueOpts, pkg.QueueEvent
    assert struct_fields(hdr, "biogpt_hip_queue_opts") == [n for n, _ in o._fields_]
    assert struct_fields(hdr, "biogpt_hip_queue_event") == [n for n, _ in e._fields_]
    assert ctypes.sizeof(o) == 64 and (o.prefix.offset, o.logprobs.offset, o.top_k.offset, o.top_p.offset, o.temp.offset) == (24, 32, 40, 48, 56)
    assert ctypes.sizeof(e) == 64 and (e.finish.offset, e.n_top.offset, e.ids.offset, e.top_lp.offset) == (16, 28, 32, 56)
    src = open(os.path.join(ROOT, "biogpt.cpp_amd", "csrc", "kernels_queue.hip.h")).read()
    for kernel in ("queue_stream_kernel", "queue_cancel_kernel"):
        assert re.search(r"__global__[^\n]*void %s\(" % kernel, src), kernel


GOOD = dict(max_columns=4, group=4, n_batch=8, n_predict=8, max_len=0, prefix=None, n_prefix=None, logprobs=-1, stream=0, top_k=40, eos_id=-1, top_p=0.95, temp=6.0)


def open_session(pkg, ctx=None, null_opts=False, **kw):
    a = dict(GOOD, **kw)
    pre = None if a["prefix"] is None else np.array(a["prefix"], dtype=np.int32)
    n_prefix = (0 if pre is None else len(pre)) if a["n_prefix"] is None else a["n_prefix"]
    o = pkg.QueueOpts(a["max_columns"], a["group"], a["n_batch"], a["n_predict"], a["max_len"], n_prefix, None if pre is None else pre.ctypes.data, a["logprobs"],
                      a["stream"], a["top_k"], a["eos_id"], a["top_p"], a["temp"])
    h = pkg.lib().biogpt_hip_queue_open(ctx, None if null_opts else ctypes.byref(o))
    return h, pkg._err()


@pytest.mark.parametrize("kw, field", [
    # everything in order: the context is what is missing -- plain, streaming, behind a prefix, with log-probabilities
    (dict(), "null context"), (dict(stream=1, logprobs=3), "null context"), (dict(prefix=(2, 11, 12), max_columns=511), "null context"), (dict(logprobs=0), "null context"),
    (dict(max_columns=512, group=64, max_len=100), "null context"),
    (dict(null_opts=True), "null argument: opts"),
    (dict(max_columns=0), "max_columns must be in [1, 512]"), (dict(max_columns=513), "max_columns must be in [1, 512]"),
    (dict(prefix=(2, 3), max_columns=512), "max_columns must be in [1, 511] behind a prefix (got 512)"),
    (dict(group=0), "group must be in [1, 64]"), (dict(group=65), "group must be in [1, 64]"),
    (dict(n_batch=0), "n_batch must be >= 1"), (dict(n_predict=-1), "n_predict must be >= 0"), (dict(max_len=-1), "max_len"),
    (dict(logprobs=-2), "logprobs must be -1 (none) or in [0, 8] (got -2)"), (dict(logprobs=9), "logprobs must be -1 (none) or in [0, 8] (got 9)"),
    (dict(n_prefix=3), "n_prefix must be 0 without a prefix (got 3)"), (dict(prefix=(2, 3), n_prefix=0), "n_prefix must be >= 1 (got 0)"),
    (dict(prefix=(2, -3)), "token id -3 (prefix, position 1)"),
    (dict(top_k=0), "top_k must be in [1, 64]"), (dict(top_k=65), "top_k must be in [1, 64]"), (dict(temp=0.0), "temp must be finite and > 0"),
    (dict(top_p=float("nan")), "top_p must be finite"), (dict(eos_id=-2), "eos_id -2 out of range"),
    # the order: the sizes before the sampler, the sampler before the prefix's tokens
    (dict(group=65, top_k=0), "group"), (dict(top_k=0, prefix=(2, -3)), "top_k"),
])
def test_open_refusals_come_before_any_device_call(pkg, kw, field):
    h, msg = open_session(pkg, **kw)
    assert not h and field in msg, (h, msg)


def test_null_sessions_are_refused_with_a_message(pkg):
    lib = pkg.lib()
    ids = np.array([2, 5, 7], dtype=np.int32)
    ev = ctypes.POINTER(pkg.QueueEvent)()
    st = pkg.QueueStats()
    for rc in (lib.biogpt_hip_queue_submit(None, ids.ctypes.data, 3, 4, 0, None), lib.biogpt_hip_queue_cancel(None, 0), lib.biogpt_hip_queue_poll(None, 1, ctypes.byref(ev)),
               lib.biogpt_hip_queue_session_stats(None, ctypes.byref(st), None, None), lib.biogpt_hip_queue_close(None)):
        assert rc == -1 and "null queue session" in pkg._err()


class FakeLib:
    def __init__(self):
        self.calls = []

    def biogpt_hip_queue_open(self, ctx, opts):
        self.calls.append("open")
        self.opts = opts._obj
        self.opts_seen = (opts._obj.max_columns, opts._obj.group, opts._obj.n_predict, opts._obj.n_prefix, opts._obj.logprobs, opts._obj.stream, opts._obj.top_k)
        return 1234

    def biogpt_hip_queue_submit(self, h, prompt, n, n_predict, seed, params):
        self.calls.append(("submit", h, n, n_predict, seed, params is not None))
        return 7

    def biogpt_hip_queue_close(self, h):
        self.calls.append(("close", h))
        return 0

    def biogpt_hip_last_error(self):
        return b""


def test_a_closed_session_is_refused_and_the_wrapper_passes_its_arguments(pkg, monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(pkg, "lib", lambda: fake)
    model = pkg.BiogptModel.__new__(pkg.BiogptModel)
    model._h = None
    with model.queue_session(max_columns=3, group=2, n_predict=9, prefix=[2, 11], logprobs=2, stream=True, top_k=40) as s:
        assert fake.opts_seen == (3, 2, 9, 2, 2, 1, 40)
        assert s.submit([5, 6, 7]) == 7 and fake.calls[-1] == ("submit", 1234, 3, 9, 0, False)      # n_predict None: the session's
        assert s.submit([], n_predict=4, seed=-1, params=pkg.request_params(top_k=3)) == 7 and fake.calls[-1] == ("submit", 1234, 0, 4, 0xFFFFFFFF, True)
        with pytest.raises(pkg.BiogptError, match="request_params"):
            s.submit([5], params=dict(top_k=1))
    assert fake.calls[-1] == ("close", 1234)
    for call in (lambda: s.submit([5]), lambda: s.poll(), lambda: s.cancel(0), lambda: s.stats(), lambda: list(s.drain())):
        with pytest.raises(pkg.BiogptError, match="the queue session is closed"):
            call()
    s.close()      # twice: nothing
    assert fake.calls.count(("close", 1234)) == 1
