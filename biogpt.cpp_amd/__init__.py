"""Host-side Python mirror of the reference's model-library interface, bound over the C-ABI.

The reference is compiled C++ (biogpt.h:128-151); its drop-in C++ wrappers live in
include/biogpt_compat.h.  This module is the thin ctypes stub used by tests/, bench.py and
__graft_entry__.py -- it only marshals pointers and sizes into libbiogpt_hip.so
(include/biogpt_hip.h).  No compute happens here and there is NO fallback: if the HIP library
is missing or no GPU is present the calls raise.

Names mirror the reference: biogpt_model_load() -> BiogptModel, biogpt_eval() -> .eval(),
biogpt_model_quantize_internal()/quantize CLI -> quantize_file().
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BIOGPT_HIP_LIB") or os.path.join(_HERE, "libbiogpt_hip.so")   # override: profiling builds (tools/)
CSRC = os.path.join(_HERE, "csrc")

FTYPES = {"f32": 0, "f16": 1, "q4_0": 2, "q4_1": 3, "q8_0": 7, "q5_0": 8, "q5_1": 9}
FTYPE_NAMES = {v: k for k, v in FTYPES.items()}
# bytes per 32-element block in the FILE layout
FILE_BLOCK_BYTES = {0: 128, 1: 64, 2: 18, 3: 20, 7: 34, 8: 22, 9: 24}


class HParams(C.Structure):
    """biogpt_hparams (biogpt.h:25-35) in file order + n_merges as found in the file."""
    _fields_ = [("n_vocab", C.c_int32), ("n_layer", C.c_int32), ("n_head", C.c_int32),
                ("n_positions", C.c_int32), ("d_ff", C.c_int32), ("d_model", C.c_int32),
                ("ftype", C.c_int32), ("n_merges", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class GenRules(C.Structure):
    """biogpt_hip_gen_rules (include/biogpt_hip.h): generation rules of generate_beam / generate_sample."""
    _fields_ = [("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32), ("min_new_tokens", C.c_int32),
                ("n_suppress", C.c_int32), ("suppress", C.POINTER(C.c_int32))]


class GenLogprobs(C.Structure):
    """biogpt_hip_gen_logprobs (include/biogpt_hip.h)."""
    _fields_ = [("n_top", C.c_int32), ("lp", C.c_void_p), ("top_ids", C.c_void_p), ("top_lp", C.c_void_p)]


class RequestParams(C.Structure):
    """biogpt_hip_request_params (include/biogpt_hip.h): one request's sampler, EOS id, rules and stop sequences for generate_queue(params=), made by
    request_params() -- `keep` holds the arrays its pointers name."""
    _fields_ = [("top_k", C.c_int32), ("eos_id", C.c_int32), ("top_p", C.c_double), ("temp", C.c_double), ("rules", GenRules),
                ("n_stop", C.c_int32), ("stop", C.POINTER(C.c_int32)), ("stop_lens", C.POINTER(C.c_int32))]
    keep = ()


def request_params(top_k=1, top_p=0.9, temp=0.9, eos_id=-1, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=(), stop=()):
    """An entry of generate_queue(params=): the request's own sampler and EOS id, its generation rules (gen_rules; at most 64 suppress_tokens here) and `stop`,
    up to 4 stop sequences of 1 .. 8 ids each ("Generation over a queue").  The ranges are checked by the call that uses it."""
    rules, ids = gen_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)
    if any(np.ndim(q) != 1 for q in stop):
        raise BiogptError("stop must be a list of id lists, one per stop sequence (a single sequence: stop=[[...]]); got %r" % (stop,))
    seqs = [np.asarray(q, dtype=np.int32).reshape(-1) for q in stop]
    flat = np.ascontiguousarray(np.concatenate(seqs + [np.zeros(1, np.int32)]))
    lens = np.ascontiguousarray([q.size for q in seqs] + [0], dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    p = RequestParams(int(top_k), int(eos_id), float(top_p), float(temp), rules, len(seqs), flat.ctypes.data_as(ip) if seqs else None,
                      lens.ctypes.data_as(ip) if seqs else None)
    p.keep = (ids, flat, lens)
    return p


def _params_array(params, n):
    """(RequestParams * n, the entries it was copied from -- they keep its pointers' arrays alive): one entry for all requests, or a list of n."""
    entries = [params] * n if isinstance(params, RequestParams) else list(params)
    if len(entries) != n:
        raise BiogptError("params must have one entry per request (%d != %d)" % (len(entries), n))
    for e in entries:
        if not isinstance(e, RequestParams):
            raise BiogptError("params: every entry must come from request_params() (got %r)" % (type(e).__name__,))
    arr = (RequestParams * max(n, 1))()
    for i, e in enumerate(entries):
        C.memmove(C.byref(arr, i * C.sizeof(RequestParams)), C.byref(e), C.sizeof(RequestParams))
    return arr, entries


class Sampler(C.Structure):
    """biogpt_hip_sampler (include/biogpt_hip.h): a sampler of any width, made by sampler()."""
    _fields_ = [("top_k", C.c_int32), ("pad", C.c_int32), ("top_p", C.c_double), ("min_p", C.c_double), ("temp", C.c_double)]

    def __repr__(self):
        return "sampler(top_k=%d, top_p=%r, min_p=%r, temp=%r)" % (self.top_k, self.top_p, self.min_p, self.temp)


def sampler(top_k=0, top_p=1.0, min_p=0.0, temp=1.0):
    """A sampler for generate_sample(sampler=) and sample_wide_rows: top_k 0 is the whole vocabulary, top_p >= 1 no cut, min_p 0 off -- the defaults draw from
    the model's own distribution ("Sampled generation").  The ranges are checked by the call that uses it."""
    return Sampler(int(top_k), 0, float(top_p), float(min_p), float(temp))


def _as_sampler(s):
    return s if isinstance(s, Sampler) else sampler(*s)


def sample_wide_rows(rows, sampler, states, device=0):
    """sample_wide_rows_kernel on rows held in host memory (biogpt_hip_sample_wide_rows_device): rows float32 [n][n_vocab]; states uint32 [n][625], the
    generators, advanced in place.  Returns (ids int32[n], n_cand int32[n]): the drawn ids and the candidates left after all cuts."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv = int(a.shape[0]), int(a.shape[1])
    if not (isinstance(states, np.ndarray) and states.dtype == np.uint32 and states.flags["C_CONTIGUOUS"] and states.shape == (n, 625)):
        raise BiogptError("states must be a contiguous uint32 array [n][625]")
    sp = _as_sampler(sampler)
    ids, nc = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    if lib().biogpt_hip_sample_wide_rows_device(int(device), a.ctypes.data, n, nv, C.byref(sp), states.ctypes.data, ids.ctypes.data, nc.ctypes.data) != 0:
        raise BiogptError(_err())
    return ids, nc


def sample_wide_rows_bench(rows, sampler, states, which=0, reps=20, device=0):
    """One kernel alone on such rows (biogpt_hip_sample_wide_rows_bench): which 0 sample_wide_rows_kernel, 1 sample_rows_kernel.  Returns the seconds of
    reps launches, each from the states as given (they are not advanced), by device events."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv = int(a.shape[0]), int(a.shape[1])
    st = np.ascontiguousarray(states, dtype=np.uint32)
    if st.shape != (n, 625):
        raise BiogptError("states must be a uint32 array [n][625]")
    sp = _as_sampler(sampler)
    secs = np.zeros(max(int(reps), 1), dtype=np.float64)
    if lib().biogpt_hip_sample_wide_rows_bench(int(device), a.ctypes.data, n, nv, C.byref(sp), st.ctypes.data, int(which), int(reps), secs.ctypes.data) != 0:
        raise BiogptError(_err())
    return secs


class _LogprobArrays:
    """The arrays of a logprobs=K request for n sequences of w entries, and the struct that names them."""

    def __init__(self, k, n, w):
        self.k = int(k)
        if not 0 <= self.k <= 8:
            raise ValueError("logprobs must be None or an integer in [0, 8] (got %r)" % (k,))
        self.lp = np.zeros((max(n, 1), w), dtype=np.float32)
        self.ids = np.full((max(n, 1), w, max(self.k, 1)), -1, dtype=np.int32)
        self.top = np.zeros((max(n, 1), w, max(self.k, 1)), dtype=np.float32)
        self.req = GenLogprobs(self.k, self.lp.ctypes.data, self.ids.ctypes.data, self.top.ctypes.data)

    def info(self, n, got, lens):
        """[(logprobs float32[len], top_ids int32[len, K], top_logprobs float32[len, K]), ...]: the call wrote rows of `got` entries."""
        k = self.k
        lp = self.lp.reshape(-1)[:n * got].reshape(n, got)
        ids = self.ids.reshape(-1)[:n * got * k].reshape(n, got, k)
        top = self.top.reshape(-1)[:n * got * k].reshape(n, got, k)
        return [(lp[r, :lens[r]].copy(), ids[r, :lens[r]].copy(), top[r, :lens[r]].copy()) for r in range(n)]


class QueueSession:
    """BiogptModel.queue_session(): see there.  An event is a dict: id, kind ("delta" / "finished" / "cancelled"), first, ids (int32 array of the tokens
    [first, first + len(ids))), finish (0 limit, 1 EOS, 2 + i stop sequence i; -1 otherwise), admit_step, column, and with logprobs= "logprobs":
    (float32[n], top_ids int32[n, K], top_logprobs float32[n, K]).  The arrays are copies: they stay valid."""

    def __init__(self, model, max_columns, group, n_predict, prefix, logprobs, stream, n_batch, max_len, top_k, top_p, temp, eos_id):
        self._h = None
        self._model = model
        self.n_predict = int(n_predict)
        pre = None if prefix is None else _flat_ids([prefix])
        o = QueueOpts(int(max_columns), int(group), int(n_batch), int(n_predict), int(max_len), 0 if prefix is None else len(prefix),
                      None if pre is None else pre.ctypes.data, -1 if logprobs is None else int(logprobs), 1 if stream else 0, int(top_k), int(eos_id), float(top_p),
                      float(temp))
        h = lib().biogpt_hip_queue_open(model._h, C.byref(o))
        if not h:
            raise BiogptError(_err())
        self._h = h

    def _handle(self):
        if not self._h:
            raise BiogptError("the queue session is closed")
        return self._h

    def submit(self, prompt, n_predict=None, seed=0, params=None):
        """Copies the request (behind a prefix: its suffix, which may be empty) and returns its id: 0, 1, 2, ... in submission order."""
        if params is not None and not isinstance(params, RequestParams):
            raise BiogptError("params must come from request_params() (got %r)" % (type(params).__name__,))
        h = self._handle()
        ids = np.ascontiguousarray(list(prompt) or [0], dtype=np.int32)
        rc = lib().biogpt_hip_queue_submit(h, ids.ctypes.data, len(prompt), self.n_predict if n_predict is None else int(n_predict), int(seed) & 0xFFFFFFFF,
                                           None if params is None else C.byref(params))
        if rc < 0:
            raise BiogptError(_err())
        return rc

    def cancel(self, id):
        h = self._handle()
        if lib().biogpt_hip_queue_cancel(h, int(id)) != 0:
            raise BiogptError(_err())

    def poll(self, max_groups=1):
        """At most max_groups groups of steps; the events they produced, in order."""
        h, ev = self._handle(), C.POINTER(QueueEvent)()
        n = lib().biogpt_hip_queue_poll(h, int(max_groups), C.byref(ev))
        if n < 0:
            raise BiogptError(_err())
        out = []
        for i in range(n):
            e = ev[i]
            c, k = int(e.count), int(e.n_top)
            d = {"id": int(e.id), "kind": QUEUE_EVENT_KINDS[e.kind], "first": int(e.first), "ids": np.ctypeslib.as_array(e.ids, (c,)).copy() if c else np.zeros(0, np.int32),
                 "finish": int(e.finish), "admit_step": int(e.admit_step), "column": int(e.column)}
            if k >= 0:
                d["logprobs"] = (np.ctypeslib.as_array(e.lp, (c,)).copy() if c else np.zeros(0, np.float32),
                                 np.ctypeslib.as_array(e.top_ids, (c, k)).copy() if c and k else np.zeros((c, k), np.int32),
                                 np.ctypeslib.as_array(e.top_lp, (c, k)).copy() if c and k else np.zeros((c, k), np.float32))
            out.append(d)
        return out

    def stats(self):
        """{"stats": the counts of generate_queue, accumulated, "seconds": host time inside polls, "submitted", "pending", "running"}"""
        h, st, secs, cnt = self._handle(), QueueStats(), C.c_double(0.0), np.zeros(3, dtype=np.int32)
        if lib().biogpt_hip_queue_session_stats(h, C.byref(st), C.byref(secs), cnt.ctypes.data) != 0:
            raise BiogptError(_err())
        return {"stats": st.as_dict(), "seconds": secs.value, "submitted": int(cnt[0]), "pending": int(cnt[1]), "running": int(cnt[2])}

    def idle(self):
        s = self.stats()
        return s["pending"] == 0 and s["running"] == 0

    def drain(self, max_groups=1):
        """Polls until nothing runs and nothing waits; yields every poll's events."""
        while True:
            events = self.poll(max_groups)
            if events:
                yield events
            if self.idle():
                return

    def close(self):
        if self._h:
            h, self._h = self._h, None
            if lib().biogpt_hip_queue_close(h) != 0:
                raise BiogptError(_err())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QueueStats(C.Structure):
    """biogpt_hip_queue_stats"""
    _fields_ = [("columns", C.c_int32), ("steps", C.c_int32), ("groups", C.c_int32), ("admissions", C.c_int32), ("prompt_columns", C.c_int32),
                ("busy_column_steps", C.c_int64), ("column_steps", C.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class EmbedOpts(C.Structure):
    """biogpt_hip_embed_opts (include/biogpt_hip.h): what embed_batch returns per sequence."""
    _fields_ = [("layer", C.c_int32), ("pooling", C.c_int32), ("normalize", C.c_int32), ("n_out", C.c_int32),
                ("w", C.POINTER(C.c_float)), ("b", C.POINTER(C.c_float))]


POOLING = {"none": 0, "last": 1, "mean": 2}


def embed_opts(layer=-1, pooling="last", normalize=False, head=None):
    """(EmbedOpts, the arrays its `w` / `b` point into -- keep them alive for the call).  head: W [n_out, d_model] or (W, b)."""
    if pooling not in POOLING:
        raise BiogptError("pooling must be one of 'none', 'last', 'mean' (got %r)" % (pooling,))
    w = b = None
    if head is not None:
        if isinstance(head, (tuple, list)) and len(head) == 2 and np.ndim(head[0]) == 2:
            w, b = head
        else:
            w = head
        w = np.ascontiguousarray(w, dtype=np.float32)
        if w.ndim != 2:
            raise BiogptError("head: W must be a [n_out, d_model] matrix")
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
            if b.size != w.shape[0]:
                raise BiogptError("head: b must have one entry per row of W (%d != %d)" % (b.size, w.shape[0]))
    fp = C.POINTER(C.c_float)
    o = EmbedOpts(int(layer), POOLING[pooling], 1 if normalize else 0, 0 if w is None else int(w.shape[0]),
                  None if w is None else w.ctypes.data_as(fp), None if b is None else b.ctypes.data_as(fp))
    return o, (w, b)


def gen_rules(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=()):
    """(GenRules, the array its `suppress` points into -- keep it alive for the call)."""
    ids = np.ascontiguousarray(list(suppress_tokens), dtype=np.int32)
    r = GenRules(float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens), int(ids.size),
                 ids.ctypes.data_as(C.POINTER(C.c_int32)) if ids.size else None)
    return r, ids


def rules_rows(rows, histories, prompt_lens=None, mode=0, eos_id=-1, device=0, **rules):
    """rules_rows_kernel on rows held in host memory (biogpt_hip_rules_rows_device): rows float32 [n][n_vocab], histories a list of id lists (row r's
    prompt + generated tokens, the first prompt_lens[r] its prompt; None: all of it).  mode 0: logits; 1: log-probabilities first.  Returns the rows."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv = a.shape
    hl = np.asarray([len(h) for h in histories], dtype=np.int32)
    pl = hl.copy() if prompt_lens is None else np.ascontiguousarray(prompt_lens, dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.int32) for h in histories] + [np.zeros(1, np.int32)]))
    r, keep = gen_rules(**rules)
    out = np.empty_like(a)
    if lib().biogpt_hip_rules_rows_device(int(device), int(mode), a.ctypes.data, n, nv, flat.ctypes.data, hl.ctypes.data, pl.ctypes.data, int(eos_id),
                                          C.byref(r), out.ctypes.data) != 0:
        raise BiogptError(_err())
    return out


class Trie:
    """A closed set of token sequences for constrained decoding (biogpt_hip_trie; INTEGRATION.md, "Constrained decoding"): pass it as trie= to
    generate_beam / generate_beam_batch / generate_sample.  Built on the host; the device copy is made at the first use on a device and freed by
    close()."""

    def __init__(self, handle, n_vocab):
        self._h = handle
        self.n_vocab = int(n_vocab)

    @classmethod
    def build(cls, seqs, n_vocab):
        """seqs: a list of id lists, each of at least one token in [0, n_vocab).  Duplicates merge; an entry may be a prefix of another."""
        seqs = [np.asarray(q, dtype=np.int32).reshape(-1) for q in seqs]
        lens = np.asarray([q.size for q in seqs], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(seqs + [np.zeros(1, np.int32)]))
        h = lib().biogpt_hip_trie_build(flat.ctypes.data, lens.ctypes.data, len(seqs), int(n_vocab))
        if not h:
            raise BiogptError(_err())
        return cls(h, n_vocab)

    def info(self):
        """dict(entries (after merging), nodes, edges, max_depth, max_fanout)."""
        out = (C.c_int64 * 5)()
        if lib().biogpt_hip_trie_info(self._h, out) != 0:
            raise BiogptError(_err())
        return dict(zip(("entries", "nodes", "edges", "max_depth", "max_fanout"), (int(v) for v in out)))

    def allowed(self, gen, eos_id):
        """The ids allowed after the generated tokens `gen`, ascending (biogpt_hip_trie_allowed_host: the definition of the mask)."""
        g = np.ascontiguousarray(gen, dtype=np.int32).reshape(-1)
        n = lib().biogpt_hip_trie_allowed_host(self._h, g.ctypes.data if g.size else None, g.size, int(eos_id), None, 0)
        if n < 0:
            raise BiogptError(_err())
        out = np.zeros(max(n, 1), dtype=np.int32)
        if lib().biogpt_hip_trie_allowed_host(self._h, g.ctypes.data if g.size else None, g.size, int(eos_id), out.ctypes.data, n) != n:
            raise BiogptError(_err())
        return out[:n].copy()

    def close(self):
        if getattr(self, "_h", None):
            lib().biogpt_hip_trie_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _trie_handle(trie):
    if not isinstance(trie, Trie) or not trie._h:
        raise BiogptError("trie must be an open Trie (Trie.build(seqs, n_vocab))")
    return trie._h


def trie_rows(rows, trie, histories, mode=0, eos_id=2, device=0, reps=0):
    """trie_rows_kernel on rows held in host memory (biogpt_hip_trie_rows_device): rows float32 [n][n_vocab], histories a list of id lists (row r's
    generated tokens; the prompt is no part of the walk).  mode 0: logits; 1: the allowed entries become log-probabilities.  Returns the rows; with
    reps > 0 (biogpt_hip_trie_rows_bench) also the microseconds of reps further launches, by device events."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv = a.shape
    hl = np.asarray([len(h) for h in histories], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(h, dtype=np.int32) for h in histories] + [np.zeros(1, np.int32)]))
    out = np.empty_like(a)
    if reps:
        us = np.zeros(int(reps), dtype=np.float32)
        if lib().biogpt_hip_trie_rows_bench(int(device), _trie_handle(trie), int(mode), a.ctypes.data, n, nv, flat.ctypes.data, hl.ctypes.data, int(eos_id),
                                            out.ctypes.data, int(reps), us.ctypes.data) != 0:
            raise BiogptError(_err())
        return out, us
    if lib().biogpt_hip_trie_rows_device(int(device), _trie_handle(trie), int(mode), a.ctypes.data, n, nv, flat.ctypes.data, hl.ctypes.data, int(eos_id),
                                         out.ctypes.data) != 0:
        raise BiogptError(_err())
    return out


def _no_rules_with_trie(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens):
    if float(repetition_penalty) != 1.0 or int(no_repeat_ngram_size) or int(min_new_tokens) or len(tuple(suppress_tokens)):
        raise BiogptError("generation rules together with a trie are not supported")


def logprob_rows(rows, targets, device=0):
    """logprob_rows_kernel on rows held in host memory (biogpt_hip_logprob_rows_device): rows float32 [n][n_vocab], targets [n] (-1: none).
    Returns (lp float32[n], argmax int32[n], logit float32[n])."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv = a.shape
    t = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
    if t.size != n:
        raise BiogptError("logprob_rows: one target per row (%d != %d)" % (t.size, n))
    lp, am, lg = np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.float32)
    if lib().biogpt_hip_logprob_rows_device(int(device), a.ctypes.data, n, nv, t.ctypes.data, lp.ctypes.data, am.ctypes.data, lg.ctypes.data) != 0:
        raise BiogptError(_err())
    return lp, am, lg


def genlp_rows(rows, n_top, mode=0, top_k=40, top_p=0.9, temp=0.9, states=None, device=0):
    """The selection kernels of generation with log-probabilities on rows held in host memory (biogpt_hip_genlp_rows_device): mode 0
    genlp_greedy_rows_kernel, mode 1 sample_lp_rows_kernel drawing from states (uint32 [n][625], advanced in place).  Returns (ids int32[n],
    logprobs float32[n], top_ids int32[n, n_top], top_logprobs float32[n, n_top])."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv, k = int(a.shape[0]), int(a.shape[1]), int(n_top)
    ids, lp = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
    tid, tlp = np.zeros((n, max(k, 1)), dtype=np.int32), np.zeros((n, max(k, 1)), dtype=np.float32)
    if states is not None and not (states.dtype == np.uint32 and states.flags["C_CONTIGUOUS"] and states.shape == (n, 625)):
        raise BiogptError("states must be a contiguous uint32 array [n][625]")
    if lib().biogpt_hip_genlp_rows_device(int(device), int(mode), a.ctypes.data, n, nv, k, int(top_k), float(top_p), float(temp),
                                          None if states is None else states.ctypes.data, ids.ctypes.data, lp.ctypes.data,
                                          tid.ctypes.data if k > 0 else None, tlp.ctypes.data if k > 0 else None) != 0:
        raise BiogptError(_err())
    return ids, lp, tid[:, :k], tlp[:, :k]


def queue_rows(rows, states, limits, finished, mt_states, hdr, n_top=0, stride=1, top_k=40, top_p=0.9, temp=0.9, eos_id=-1, with_lp=True, device=0):
    """One launch of the queue's step kernel on rows held in host memory (biogpt_hip_queue_rows_device): queue_rows_lp_kernel, or with_lp=False
    queue_rows_kernel; row r is column r.  states int32 [n][8] (n_past, token, n_gen, seq_id, t_vis, 3 more words), finished int32 [n], mt_states uint32
    [n][625] and hdr int32 [1 + 2 n] (n_live, fin[], len[]) are contiguous arrays, changed in place as the launch leaves them; limits int32 [n].  Returns
    (ids int32[n, stride], logprobs float32[n, stride], top_ids int32[n, stride, n_top], top_logprobs float32[n, stride, n_top]) with 0xff bytes (-1, NaN)
    wherever the launch wrote nothing."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv, k, w = int(a.shape[0]), int(a.shape[1]), int(n_top), int(stride)
    lim = np.ascontiguousarray(limits, dtype=np.int32).reshape(-1)
    for name, arr, dt, shape in (("states", states, np.int32, (n, 8)), ("finished", finished, np.int32, (n,)), ("mt_states", mt_states, np.uint32, (n, 625)),
                                 ("hdr", hdr, np.int32, (1 + 2 * n,))):
        if not (isinstance(arr, np.ndarray) and arr.dtype == dt and arr.flags["C_CONTIGUOUS"] and arr.shape == shape):
            raise BiogptError("%s must be a contiguous %s array of shape %s" % (name, np.dtype(dt).name, shape))
    if lim.size != n:
        raise BiogptError("limits must have one entry per row (%d != %d)" % (lim.size, n))
    ids, lp = np.zeros((n, max(w, 1)), dtype=np.int32), np.zeros((n, max(w, 1)), dtype=np.float32)
    tid, tlp = np.zeros((n, max(w, 1), max(k, 1)), dtype=np.int32), np.zeros((n, max(w, 1), max(k, 1)), dtype=np.float32)
    if lib().biogpt_hip_queue_rows_device(int(device), 1 if with_lp else 0, a.ctypes.data, n, nv, k, w, int(top_k), float(top_p), float(temp), int(eos_id),
                                          mt_states.ctypes.data, states.ctypes.data, lim.ctypes.data, finished.ctypes.data, hdr.ctypes.data, ids.ctypes.data,
                                          lp.ctypes.data, tid.ctypes.data if k > 0 else None, tlp.ctypes.data if k > 0 else None) != 0:
        raise BiogptError(_err())
    return ids, lp, tid[:, :, :k], tlp[:, :, :k]


def queue_req_rows(rows, params, histories, prompt_lens, states, limits, finished, mt_states, hdr, n_top=0, stride=1, with_lp=False, device=0):
    """One launch of queue_req_rows_kernel on rows held in host memory (biogpt_hip_queue_req_rows_device): row r is column r with the record of params[r]
    (request_params entries) and the history histories[r], the first prompt_lens[r] tokens its prompt and the rest its generated tokens.  states int32 [n][8],
    finished int32 [n], mt_states uint32 [n][625] and hdr int32 [1 + 3 n] (n_live, fin[], len[], reason[]) are changed in place.  Returns (ids int32
    [n][stride], lp float32 [n][stride], top_ids int32 [n][stride][n_top], top_lp): 0xff bytes wherever the launch wrote nothing, but for the generated tokens
    given, which stand in the first entries of their ids rows."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv = int(a.shape[0]), int(a.shape[1])
    for name, arr, dt, shape in (("states", states, np.int32, (n, 8)), ("finished", finished, np.int32, (n,)), ("mt_states", mt_states, np.uint32, (n, 625)),
                                 ("hdr", hdr, np.int32, (1 + 3 * n,))):
        if not (isinstance(arr, np.ndarray) and arr.dtype == dt and arr.flags["C_CONTIGUOUS"] and arr.shape == shape):
            raise BiogptError("%s must be a contiguous %s array of shape %r" % (name, np.dtype(dt).name, shape))
    lim = np.ascontiguousarray(limits, dtype=np.int32).reshape(-1)
    pl = np.ascontiguousarray(prompt_lens, dtype=np.int32).reshape(-1)
    hl = np.ascontiguousarray([len(h) for h in histories], dtype=np.int32)
    if lim.size != n or pl.size != n or hl.size != n:
        raise BiogptError("limits, prompt_lens and histories must have one entry per row")
    flat = _flat_ids(histories)
    arr, keep = _params_array(params, n)
    k, w = int(n_top), int(stride)
    ids = np.zeros((n, w), dtype=np.int32)
    lp = np.zeros((n, w), dtype=np.float32)
    tid, tlp = np.zeros((n, w, max(k, 1)), dtype=np.int32), np.zeros((n, w, max(k, 1)), dtype=np.float32)
    if lib().biogpt_hip_queue_req_rows_device(int(device), 1 if with_lp else 0, a.ctypes.data, n, nv, k, w, arr, flat.ctypes.data, hl.ctypes.data, pl.ctypes.data,
                                              mt_states.ctypes.data, states.ctypes.data, lim.ctypes.data, finished.ctypes.data, hdr.ctypes.data, ids.ctypes.data,
                                              lp.ctypes.data, tid.ctypes.data if k else None, tlp.ctypes.data if k else None) != 0:
        raise BiogptError(_err())
    return ids, lp, tid[:, :, :k], tlp[:, :, :k]


def lookup_draft(texts, n_gen, n_past, n_predict, max_draft=7, max_ngram=3, finished=None, device=0):
    """lookup_draft_kernel on texts held in host memory (biogpt_hip_lookup_draft_device): texts a list of id lists (corpus + prompt + generated tokens), n_gen[s]
    how many of text s were generated, n_past[s] the position of its last token.  Returns (drafts: list of id lists, d int32[n], cols int32[n][1 + max_draft][4]:
    token, n_past, seq_id, t_vis of every packed column state)."""
    n = len(texts)
    lens = np.asarray([len(t) for t in texts], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in texts] + [np.zeros(1, np.int32)]))
    ng = np.ascontiguousarray(n_gen, dtype=np.int32).reshape(-1)
    npast = np.ascontiguousarray(n_past, dtype=np.int32).reshape(-1)
    if ng.size != n or npast.size != n:
        raise BiogptError("lookup_draft: one n_gen and one n_past per text")
    fin = None if finished is None else np.ascontiguousarray(finished, dtype=np.int32).reshape(-1)
    dr = np.zeros((max(n, 1), 16), np.int32)
    d = np.zeros(max(n, 1), np.int32)
    cols = np.zeros((max(n, 1), 1 + max(int(max_draft), 0), 4), np.int32)
    if lib().biogpt_hip_lookup_draft_device(int(device), flat.ctypes.data, lens.ctypes.data, n, ng.ctypes.data, npast.ctypes.data,
                                            None if fin is None else fin.ctypes.data, int(n_predict), int(max_draft), int(max_ngram), dr.ctypes.data,
                                            d.ctypes.data, cols.ctypes.data) != 0:
        raise BiogptError(_err())
    return [dr[s, :int(d[s])].tolist() for s in range(n)], d[:n].copy(), cols[:n].copy()


def lookup_accept(rows, drafts, n_gen, n_past, n_predict, max_draft, eos_id=-1, finished=None, device=0):
    """lookup_accept_kernel on logits rows held in host memory (biogpt_hip_lookup_accept_device): rows float32 [n * (1 + max_draft)][n_vocab], drafts a list of
    id lists (at most max_draft each).  Returns (emitted: list of id lists, state int32[n][4]: token, n_past, n_gen, finished; stats int32[n][3]: passes, drafted,
    accepted; (live count, furthest position))."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n = len(drafts)
    S = 1 + int(max_draft)
    if a.ndim != 2 or a.shape[0] != n * S:
        raise BiogptError("lookup_accept: rows must be [n * (1 + max_draft)][n_vocab]")
    dr = np.full((max(n, 1), 16), -1, np.int32)
    d = np.zeros(max(n, 1), np.int32)
    for s, t in enumerate(drafts):
        if len(t) > 15:
            raise BiogptError("lookup_accept: a draft holds at most 15 tokens")
        d[s] = len(t)
        dr[s, :len(t)] = np.asarray(t, dtype=np.int32)
    ng = np.ascontiguousarray(n_gen, dtype=np.int32).reshape(-1)
    npast = np.ascontiguousarray(n_past, dtype=np.int32).reshape(-1)
    if ng.size != n or npast.size != n:
        raise BiogptError("lookup_accept: one n_gen and one n_past per sequence")
    fin = None if finished is None else np.ascontiguousarray(finished, dtype=np.int32).reshape(-1)
    emit = np.zeros((max(n, 1), 16), np.int32)
    state = np.zeros((max(n, 1), 4), np.int32)
    stats = np.zeros((max(n, 1), 3), np.int32)
    live = np.zeros(2, np.int32)
    if lib().biogpt_hip_lookup_accept_device(int(device), a.ctypes.data, n, a.shape[1], int(max_draft), dr.ctypes.data, d.ctypes.data, ng.ctypes.data,
                                             npast.ctypes.data, None if fin is None else fin.ctypes.data, int(n_predict), int(eos_id), emit.ctypes.data,
                                             state.ctypes.data, stats.ctypes.data, live.ctypes.data) != 0:
        raise BiogptError(_err())
    return [[int(v) for v in emit[s] if v >= 0] for s in range(n)], state[:n].copy(), stats[:n].copy(), (int(live[0]), int(live[1]))


def queue_plan(gen_lens, max_columns, group, limits=None):
    """The schedule of BiogptModel.generate_queue from the generated lengths alone (biogpt_hip_queue_plan: the host struct the call itself drives, no device):
    ({"stats": {...}, "admit_step": [...], "column": [...]}); a request of length 0 never takes a column (-1 in both lists); prompt_columns stays 0.
    limits (biogpt_hip_queue_plan_limits): what every request may generate at most, as clamped -- the schedule of a run whose requests end before their
    limits (an EOS, a beam search that stops), where a group is sized from the limits; for generate_beam_queue gen_lens are info["steps"] and max_columns
    the number of slots."""
    gl = np.ascontiguousarray(gen_lens, dtype=np.int32).reshape(-1)
    n = int(gl.size)
    if n == 0:
        gl = np.zeros(1, np.int32)
    adm, col = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    st = QueueStats()
    if limits is not None:
        lm = np.ascontiguousarray(limits, dtype=np.int32).reshape(-1)
        if lm.size != n:
            raise BiogptError("limits must have one entry per request (%d != %d)" % (lm.size, n))
        if n == 0:
            lm = np.zeros(1, np.int32)
        rc = lib().biogpt_hip_queue_plan_limits(gl.ctypes.data, lm.ctypes.data, n, int(max_columns), int(group), adm.ctypes.data, col.ctypes.data, C.byref(st))
    else:
        rc = lib().biogpt_hip_queue_plan(gl.ctypes.data, n, int(max_columns), int(group), adm.ctypes.data, col.ctypes.data, C.byref(st))
    if rc != 0:
        raise BiogptError(_err())
    return {"stats": st.as_dict(), "admit_step": [int(v) for v in adm[:n]], "column": [int(v) for v in col[:n]]}


class QueueOpts(C.Structure):
    """biogpt_hip_queue_opts (include/biogpt_hip.h)"""
    _fields_ = [("max_columns", C.c_int32), ("group", C.c_int32), ("n_batch", C.c_int32), ("n_predict", C.c_int32), ("max_len", C.c_int32), ("n_prefix", C.c_int32),
                ("prefix", C.c_void_p), ("logprobs", C.c_int32), ("stream", C.c_int32), ("top_k", C.c_int32), ("eos_id", C.c_int32), ("top_p", C.c_double),
                ("temp", C.c_double)]


class QueueEvent(C.Structure):
    """biogpt_hip_queue_event (include/biogpt_hip.h)"""
    _fields_ = [("id", C.c_int32), ("kind", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("finish", C.c_int32), ("admit_step", C.c_int32),
                ("column", C.c_int32), ("n_top", C.c_int32), ("ids", C.POINTER(C.c_int32)), ("lp", C.POINTER(C.c_float)), ("top_ids", C.POINTER(C.c_int32)),
                ("top_lp", C.POINTER(C.c_float))]


QUEUE_EVENT_KINDS = ("delta", "finished", "cancelled")
SUBMIT, POLL, CANCEL = 0, 1, 2      # the operations of a queue_plan_script script


def queue_plan_script(ops, gen_lens, limits, max_columns, group):
    """The schedule of a queue session (BiogptModel.queue_session) on a script, from the lengths alone (biogpt_hip_queue_plan_script: the scheduler the session
    itself drives, no device).  ops: (SUBMIT,), (POLL, n) and (CANCEL, r) in order; the i-th SUBMIT is request i, which generates gen_lens[i] tokens under the
    limit limits[i].  Returns {"stats": {...}, "admit_step": [...], "column": [...], "finish_group": [...], "lens": [...]}: -1 in the first two where a request
    never took a column; finish_group the groups run when the request's finished or cancelled event came (-1: the script ends before); lens what it had then."""
    flat = np.zeros((max(len(ops), 1), 2), dtype=np.int32)
    for i, op in enumerate(ops):
        flat[i, 0] = int(op[0])
        flat[i, 1] = int(op[1]) if len(op) > 1 else 0
    gl = np.ascontiguousarray(gen_lens, dtype=np.int32).reshape(-1)
    lm = np.ascontiguousarray(limits, dtype=np.int32).reshape(-1)
    n = sum(1 for op in ops if int(op[0]) == SUBMIT)
    if gl.size != n or lm.size != n:
        raise BiogptError("gen_lens and limits must have one entry per SUBMIT (%d, %d != %d)" % (gl.size, lm.size, n))
    if n == 0:
        gl = lm = np.zeros(1, np.int32)
    adm, col, fg, ln = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(4))
    st = QueueStats()
    if lib().biogpt_hip_queue_plan_script(flat.ctypes.data, len(ops), gl.ctypes.data, lm.ctypes.data, int(max_columns), int(group), adm.ctypes.data, col.ctypes.data,
                                          fg.ctypes.data, ln.ctypes.data, C.byref(st)) != 0:
        raise BiogptError(_err())
    return {"stats": st.as_dict(), "admit_step": [int(v) for v in adm[:n]], "column": [int(v) for v in col[:n]], "finish_group": [int(v) for v in fg[:n]],
            "lens": [int(v) for v in ln[:n]]}


def queue_stream_rows(n_gen, gen_rows, g, lp=None, top_ids=None, top_lp=None, guard=256, device=0):
    """queue_stream_kernel on constructed columns (biogpt_hip_queue_stream_device): n_gen int32 [C], gen_rows int32 [C][gen_stride]; lp float32 [C][lp_stride]
    with top_ids / top_lp [C][lp_stride][K] for the form with log-probabilities (K may be 0).  Returns (block uint8, layout bytes): the block as the launch
    left it, preset to 0xff bytes, `guard` bytes longer than its layout."""
    ng = np.ascontiguousarray(n_gen, dtype=np.int32).reshape(-1)
    rows = np.ascontiguousarray(gen_rows, dtype=np.int32)
    c, stride = int(rows.shape[0]), int(rows.shape[1])
    k, lps = -1, 1
    a_lp = a_ti = a_tl = None
    if lp is not None:
        a_lp = np.ascontiguousarray(lp, dtype=np.float32)
        lps = int(a_lp.shape[1])
        a_ti = np.ascontiguousarray(top_ids, dtype=np.int32)
        a_tl = np.ascontiguousarray(top_lp, dtype=np.float32)
        k = int(a_ti.shape[2])
    per = c * int(g)
    need = sum((b + 15) // 16 * 16 for b in ([c * 4, per * 4] + ([per * 4, per * k * 4, per * k * 4] if k >= 0 else [])))
    block = np.zeros(need + int(guard), dtype=np.uint8)
    got = lib().biogpt_hip_queue_stream_device(int(device), ng.ctypes.data, rows.ctypes.data, c, stride, int(g), k, lps, None if a_lp is None else a_lp.ctypes.data,
                                               None if a_ti is None or k == 0 else a_ti.ctypes.data, None if a_tl is None or k == 0 else a_tl.ctypes.data,
                                               block.ctypes.data, block.size)
    if got < 0:
        raise BiogptError(_err())
    return block, int(got)


def queue_cancel_cols(cols, finished, n_gen, hdr, device=0):
    """queue_cancel_kernel on the list `cols` over 512 constructed columns (biogpt_hip_queue_cancel_device): finished int32 [512] and hdr int32 [1 + 1024]
    (n_live, fin[], len[]) are changed in place, n_gen int32 [512] is read."""
    cl = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
    ng = np.ascontiguousarray(n_gen, dtype=np.int32).reshape(-1)
    for a, size, name in ((finished, 512, "finished"), (hdr, 1025, "hdr")):
        if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] and a.size == size):
            raise BiogptError("%s must be a contiguous int32 array of %d" % (name, size))
    if ng.size != 512:
        raise BiogptError("n_gen must have 512 entries")
    if lib().biogpt_hip_queue_cancel_device(int(device), cl.ctypes.data, int(cl.size), finished.ctypes.data, ng.ctypes.data, hdr.ctypes.data) != 0:
        raise BiogptError(_err())


PREFIX_BATCH_SLOTS = 512      # one biogpt_hip_score_continuations_batch call: a slot per prefix and one per continuation


def prefix_batch_chunks(n_conts, max_slots=PREFIX_BATCH_SLOTS):
    """How score_continuations_batch cuts a dataset into calls: n_conts[g] continuations per group -> [(first group, one past the last)], greedily and in
    order, each call within max_slots slots (1 + n_conts[g] per group).  A group that alone needs more raises."""
    chunks, g0, used = [], 0, 0
    for g, n in enumerate(n_conts):
        need = 1 + int(n)
        if need > max_slots:
            raise BiogptError("group %d alone needs %d slots (1 prefix + %d continuations): more than the %d of one call" % (g, need, int(n), max_slots))
        if used + need > max_slots:
            chunks.append((g0, g))
            g0, used = g, 0
        used += need
    if used:
        chunks.append((g0, len(n_conts)))
    return chunks


def attn_runs_plan(seq_states):
    """The planner of attn_runs_kernel (biogpt_hip_attn_runs_plan) on packed column states int32 [N][8]: int32 [n_runs][4] rows (c0, n, R, S)."""
    st = np.ascontiguousarray(seq_states, dtype=np.int32).reshape(-1, 8)
    runs = np.zeros((max(len(st), 1), 4), dtype=np.int32)
    n = lib().biogpt_hip_attn_runs_plan(st.ctypes.data, len(st), runs.ctypes.data)
    if n < 0:
        raise BiogptError(_err())
    return runs[:n].copy()


def attn_runs_device(H, P, t_max, n_slots, q, k_slots, v_slots, seq_states, runs=None, q8=0, device=0, reps=0):
    """One attn_runs_kernel<8> launch on arrays held in host memory (biogpt_hip_attn_runs_device): q float32 [N][H * 64], k_slots / v_slots float32
    [n_slots][H][P][64], seq_states int32 [N][8], runs int32 [n_runs][4] or None (the planner's).  Returns (rc, out, out_q, out_d, out_s, launched) with
    the outputs whole: N rounded up to 16 rows plus a guard row, preset to 0xff.  reps > 0: a seventh item, the microseconds of reps further launches."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    k = np.ascontiguousarray(k_slots, dtype=np.float32)
    v = np.ascontiguousarray(v_slots, dtype=np.float32)
    st = np.ascontiguousarray(seq_states, dtype=np.int32).reshape(-1, 8)
    N, D = len(st), H * 64
    rows = (N + 15) // 16 * 16 + 1
    out = np.zeros((rows, D), dtype=np.float32)
    oq, od, os_ = np.zeros((rows, D), dtype=np.int8), np.zeros((rows, D // 32), dtype=np.float32), np.zeros((rows, D // 32), dtype=np.uint32)
    launched = np.full(8, -1, dtype=np.int32)
    rn = None if runs is None else np.ascontiguousarray(runs, dtype=np.int32).reshape(-1, 4)
    args = (int(device), int(H), N, int(P), int(t_max), int(n_slots), q.ctypes.data, k.ctypes.data, v.ctypes.data, st.ctypes.data,
            None if rn is None else rn.ctypes.data, 0 if rn is None else len(rn), int(q8), out.ctypes.data, oq.ctypes.data if q8 else None,
            od.ctypes.data if q8 else None, os_.ctypes.data if q8 else None, launched.ctypes.data)
    if reps > 0:
        us = np.zeros(reps, dtype=np.float32)
        rc = lib().biogpt_hip_attn_runs_bench(*args, int(reps), us.ctypes.data)
        return rc, out, oq, od, os_, launched, us
    rc = lib().biogpt_hip_attn_runs_device(*args)
    return rc, out, oq, od, os_, launched


def beam_rows(rows, n_beams, run_score, given=False, first_step=False, device=0, masked=False):
    """beam_group_rows_kernel on rows held in host memory (biogpt_hip_beam_rows_device): rows float32 [G * n_beams][n_vocab], run_score [G * n_beams].
    Returns (score float32, col int32, id int32), each [G * n_beams][2 * n_beams]; rows the kernel left alone hold (NaN, -1, -1).  masked (with given):
    the rows may hold fewer than 2 * n_beams finite values, as a trie step leaves them (biogpt_hip_beam_rows_masked_device)."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    n, nv = a.shape
    rs = np.ascontiguousarray(run_score, dtype=np.float32).reshape(-1)
    if rs.size != n:
        raise BiogptError("beam_rows: one run_score per row (%d != %d)" % (rs.size, n))
    K = 2 * int(n_beams)
    sc, col, ids = np.empty((n, K), np.float32), np.empty((n, K), np.int32), np.empty((n, K), np.int32)
    if masked:
        if not given:
            raise BiogptError("beam_rows: masked rows are log-probabilities (given=True)")
        if lib().biogpt_hip_beam_rows_masked_device(int(device), a.ctypes.data, n, nv, int(n_beams), rs.ctypes.data, 1 if first_step else 0, sc.ctypes.data,
                                                    col.ctypes.data, ids.ctypes.data) != 0:
            raise BiogptError(_err())
        return sc, col, ids
    if lib().biogpt_hip_beam_rows_device(int(device), a.ctypes.data, n, nv, 1 if given else 0, int(n_beams), rs.ctypes.data, 1 if first_step else 0,
                                         sc.ctypes.data, col.ctypes.data, ids.ctypes.data) != 0:
        raise BiogptError(_err())
    return sc, col, ids


def beam_table(table, start_tokens, prompt_lens, n_beams, n_predict, eos_id=-1, length_penalty=1.0, early_stopping=True, given=True, max_steps=None,
               device=0):
    """A beam search over the beam kernels with a table for a model (biogpt_hip_beam_table_device): table float32 [R][n_vocab], one start token and
    prompt length per group.  Returns (results, state): results = per group [(ids, score), ...] best first, or None if max_steps ended the run first;
    state = dict of token, n_gen, run_score, rank [G][B], hist [G][B][n_predict], done, step [G], k, v [G][B][2][P][4]."""
    a = np.ascontiguousarray(table, dtype=np.float32)
    R, nv = a.shape
    st = np.ascontiguousarray(start_tokens, dtype=np.int32).reshape(-1)
    pl = np.ascontiguousarray(prompt_lens, dtype=np.int32).reshape(-1)
    if st.size != pl.size or st.size < 1:
        raise BiogptError("beam_table: one start token and one prompt length per group")
    G, B, n = int(st.size), int(n_beams), int(n_predict)
    P = int(pl.max()) + n
    ids = np.empty((G, max(B, 0), max(n, 0)), np.int32)
    lens, scores, counts = np.empty((G, max(B, 0)), np.int32), np.empty((G, max(B, 0)), np.float32), np.empty(G, np.int32)
    shape = (G, max(B, 0))
    tok, ngen, rank, rs = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.float32)
    hist = np.empty(shape + (max(n, 0),), np.int32)
    done, step = np.empty(G, np.int32), np.empty(G, np.int32)
    kv = np.empty((2,) + shape + (2, max(P, 1), 4), np.float32)
    rc = lib().biogpt_hip_beam_table_device(int(device), a.ctypes.data, R, nv, 1 if given else 0, st.ctypes.data, pl.ctypes.data, G, B, n, int(eos_id),
                                            float(length_penalty), 1 if early_stopping else 0, n if max_steps is None else int(max_steps), ids.ctypes.data,
                                            lens.ctypes.data, scores.ctypes.data, counts.ctypes.data, tok.ctypes.data, ngen.ctypes.data, hist.ctypes.data,
                                            rs.ctypes.data, rank.ctypes.data, done.ctypes.data, step.ctypes.data, kv.ctypes.data)
    if rc < 0:
        raise BiogptError(_err())
    state = dict(token=tok, n_gen=ngen, run_score=rs, rank=rank, hist=hist, done=done, step=step, k=kv[0], v=kv[1])
    if rc == 0:
        return None, state
    results = [[([int(t) for t in ids[g, r, :lens[g, r]]], np.float32(scores[g, r])) for r in range(int(counts[g]))] for g in range(G)]
    return results, state


def contrast_rank(cand, ctx_rows, probs, alpha, device=0):
    """The penalty and selection kernels of contrastive search on rows held in host memory (biogpt_hip_contrast_rank_device): cand float32 [k][d],
    ctx_rows float32 [T][d], probs float32 [k].  Returns (pen float32[k], score float32[k], winner)."""
    c = np.ascontiguousarray(cand, dtype=np.float32)
    h = np.ascontiguousarray(ctx_rows, dtype=np.float32)
    p = np.ascontiguousarray(probs, dtype=np.float32).reshape(-1)
    if c.ndim != 2 or h.ndim != 2 or c.shape[1] != h.shape[1] or p.size != c.shape[0]:
        raise BiogptError("contrast_rank: cand [k][d], ctx_rows [T][d] and probs [k] do not fit together")
    k, d = c.shape
    pen = np.zeros(k, dtype=np.float32)
    score = np.zeros(k, dtype=np.float32)
    win = C.c_int32(-1)
    if lib().biogpt_hip_contrast_rank_device(int(device), c.ctypes.data, h.ctypes.data, k, h.shape[0], d, p.ctypes.data, float(alpha), pen.ctypes.data,
                                             score.ctypes.data, C.addressof(win)) != 0:
        raise BiogptError(_err())
    return pen, score, int(win.value)


BIOGPT_BASE = dict(n_vocab=42384, n_layer=24, n_head=16, n_positions=1024, d_ff=4096, d_model=1024,
                   ftype=0, n_merges=40000)


class BiogptError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile libbiogpt_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))] + [os.path.join(_HERE, "..", "include", "biogpt_hip.h")]
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    cmd = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))] + (["-B"] if force else []) + ["all"]   # objects under csrc/obj/ (git-ignored)
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL, stderr=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_lib = None

# every symbol include/biogpt_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("biogpt_hip_last_error", C.c_char_p, []),
    ("biogpt_hip_version", C.c_char_p, []),
    ("biogpt_hip_load", _P, [C.c_char_p, C.c_int, C.c_int]),
    ("biogpt_hip_load_into", _P, [C.c_char_p, C.c_int, C.c_int, _P, C.c_size_t]),
    ("biogpt_hip_attach", _P, [C.POINTER(HParams), C.c_int, _P, C.c_size_t]),
    ("biogpt_hip_arena_bytes_for", C.c_size_t, [C.POINTER(HParams)]),
    ("biogpt_hip_arena_ptr", _P, [_P]),
    ("biogpt_hip_arena_bytes", C.c_size_t, [_P]),
    ("biogpt_hip_free", None, [_P]),
    ("biogpt_hip_refresh_options", C.c_int, [_P]),
    ("biogpt_hip_xpipe_state", C.c_int, [_P]),
    ("biogpt_hip_share_vocab", C.c_int, [_P, _P]),
    ("biogpt_hip_replicas_load", _P, [C.c_char_p, _P, C.c_int, C.c_int]),
    ("biogpt_hip_replicas_count", C.c_int, [_P]),
    ("biogpt_hip_replicas_ctx", _P, [_P, C.c_int]),
    ("biogpt_hip_replicas_broadcast_seconds", C.c_double, [_P]),
    ("biogpt_hip_replicas_generate_greedy", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_replicas_free", None, [_P]),
    ("biogpt_hip_get_hparams", C.c_int, [_P, C.POINTER(HParams)]),
    ("biogpt_hip_n_tensors", C.c_int, [_P]),
    ("biogpt_hip_vocab_token", C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32)]),
    ("biogpt_hip_merge", C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32)]),
    ("biogpt_hip_eval", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    ("biogpt_hip_eval_inplace", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(C.POINTER(C.c_float))]),
    ("biogpt_hip_resident_stats", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("biogpt_hip_chunk_launches", C.c_int64, [_P]),
    ("biogpt_hip_mfma_launches", C.c_int64, [_P]),
    ("biogpt_hip_chain_kind", C.c_int, [_P]),
    ("biogpt_hip_wide_launches", C.c_int64, [_P]),
    ("biogpt_hip_float_chain", C.c_int, [_P, C.c_int]),
    ("biogpt_hip_float_launches", C.c_int64, [_P]),
    ("biogpt_hip_assoc", C.c_int, [_P, C.c_int]),
    ("biogpt_hip_get_assoc", C.c_int, [_P]),
    ("biogpt_hip_assoc_chain", C.c_int, [_P, C.c_int]),
    ("biogpt_hip_get_assoc_chain", C.c_int, [_P]),
    ("biogpt_hip_simd_chain_launches", C.c_int64, [_P]),
    ("biogpt_hip_fpipe_launches", C.c_int64, [_P]),
    ("biogpt_hip_fpipe_stamps", C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    ("biogpt_hip_generate_launches", C.c_int, [_P, C.POINTER(C.c_int32), C.c_int]),
    ("biogpt_hip_lineage_stats", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("biogpt_hip_bench_sweep", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("biogpt_hip_bench_sweep_ex", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_size_t,
                                            C.POINTER(C.c_int8), C.POINTER(C.c_float)]),
    ("biogpt_hip_eval_device", C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    ("biogpt_hip_eval_topk", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("biogpt_hip_logits_device", _P, [_P]),
    ("biogpt_hip_read_logits", C.c_int, [_P, _P]),
    ("biogpt_hip_synchronize", C.c_int, [_P]),
    ("biogpt_hip_eval_all", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    ("biogpt_hip_eval_prompt", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("biogpt_hip_generate_greedy", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_greedy_batch", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_beam", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _P, _P,
                                          C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_sample", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, C.c_int32, _P, _P,
                                            C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_beam_rules", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _P, _P,
                                                C.POINTER(C.c_double), C.POINTER(GenRules)]),
    ("biogpt_hip_generate_sample_rules", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, C.c_int32, _P, _P,
                                                  C.POINTER(C.c_double), C.POINTER(GenRules)]),
    ("biogpt_hip_generate_beam_batch", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.POINTER(GenRules),
                                                _P, _P, _P, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_contrastive", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_contrast_rank_device", C.c_int, [C.c_int, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_float, _P, _P, _P]),
    ("biogpt_hip_generate_lookup", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_queue", C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, C.c_int32,
                                           _P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(QueueStats)]),
    ("biogpt_hip_generate_queue_prefix", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                                  _P, C.c_int32, _P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(QueueStats), C.POINTER(GenLogprobs)]),
    ("biogpt_hip_queue_plan", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(QueueStats)]),
    ("biogpt_hip_queue_plan_limits", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(QueueStats)]),
    ("biogpt_hip_read_column_state", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    ("biogpt_hip_generate_beam_queue", C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P,
                                                _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(QueueStats)]),
    ("biogpt_hip_lookup_draft_device", C.c_int, [C.c_int, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("biogpt_hip_lookup_accept_device", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("biogpt_hip_rules_rows_device", C.c_int, [C.c_int, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.POINTER(GenRules), _P]),
    ("biogpt_hip_trie_build", _P, [_P, _P, C.c_int32, C.c_int32]),
    ("biogpt_hip_trie_free", None, [_P]),
    ("biogpt_hip_trie_info", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("biogpt_hip_trie_allowed_host", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    ("biogpt_hip_generate_beam_trie", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _P, _P, _P, _P,
                                               C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_sample_trie", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, C.c_int32, _P, _P, _P,
                                                 C.POINTER(C.c_double)]),
    ("biogpt_hip_trie_rows_device", C.c_int, [C.c_int, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
    ("biogpt_hip_trie_rows_bench", C.c_int, [C.c_int, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, _P]),
    ("biogpt_hip_beam_rows_masked_device", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("biogpt_hip_logprob_rows_device", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("biogpt_hip_beam_rows_device", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("biogpt_hip_beam_table_device", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                              C.c_int32, C.c_int32] + [_P] * 12),
    ("biogpt_hip_mt19937_seed", C.c_int, [C.c_uint32, _P]),
    ("biogpt_hip_sample_candidates_host", C.c_int, [_P, _P, C.c_int32, C.c_double, C.c_double, _P, _P]),
    ("biogpt_hip_sample_rows_device", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, _P]),
    ("biogpt_hip_score", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("biogpt_hip_score_batch", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P]),
    ("biogpt_hip_score_continuations", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_score_continuations_batch", C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_prefix_batch_stats", C.c_int, [_P, _P]),
    ("biogpt_hip_attn_runs_plan", C.c_int, [_P, C.c_int32, _P]),
    ("biogpt_hip_attn_runs_device", C.c_int, [C.c_int] + [C.c_int32] * 5 + [_P] * 5 + [C.c_int32, C.c_int32] + [_P] * 5),
    ("biogpt_hip_attn_runs_bench", C.c_int, [C.c_int] + [C.c_int32] * 5 + [_P] * 5 + [C.c_int32, C.c_int32] + [_P] * 5 + [C.c_int32, _P]),
    ("biogpt_hip_generate_greedy_prefix", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_sample_prefix", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P,
                                                    C.c_int32, _P, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_prefix_stats", C.c_int, [_P, _P]),
    ("biogpt_hip_generate_sample_wide", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_generate_sample_wide_prefix", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P, _P,
                                                         C.POINTER(C.c_double)]),
    ("biogpt_hip_sample_wide_rows_device", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("biogpt_hip_sample_wide_rows_bench", C.c_int, [C.c_int, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P]),
    ("biogpt_hip_generate_greedy_batch_lp", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double), C.POINTER(GenLogprobs)]),
    ("biogpt_hip_generate_sample_lp", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P,
                                                C.c_int32, _P, _P, C.POINTER(C.c_double), C.POINTER(GenLogprobs)]),
    ("biogpt_hip_genlp_rows_device", C.c_int, [C.c_int, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, _P, _P, _P, _P]),
    ("biogpt_hip_queue_rows_device", C.c_int, [C.c_int, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32] + [_P] * 9),
    ("biogpt_hip_generate_queue_requests", C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RequestParams), _P,
                                                    _P, _P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(QueueStats), C.POINTER(GenLogprobs)]),
    ("biogpt_hip_queue_req_rows_device", C.c_int, [C.c_int, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RequestParams)] + [_P] * 12),
    ("biogpt_hip_queue_open", _P, [_P, C.POINTER(QueueOpts)]),
    ("biogpt_hip_queue_submit", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(RequestParams)]),
    ("biogpt_hip_queue_cancel", C.c_int, [_P, C.c_int32]),
    ("biogpt_hip_queue_poll", C.c_int, [_P, C.c_int32, C.POINTER(C.POINTER(QueueEvent))]),
    ("biogpt_hip_queue_session_stats", C.c_int, [_P, C.POINTER(QueueStats), C.POINTER(C.c_double), _P]),
    ("biogpt_hip_queue_close", C.c_int, [_P]),
    ("biogpt_hip_queue_plan_script", C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.POINTER(QueueStats)]),
    ("biogpt_hip_queue_stream_device", C.c_int64, [C.c_int, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64]),
    ("biogpt_hip_queue_cancel_device", C.c_int, [C.c_int, _P, C.c_int32, _P, _P, _P]),
    ("biogpt_hip_attn_device", C.c_int, [C.c_int] + [C.c_int32] * 7 + [_P] * 5 + [C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("biogpt_hip_chain_device", C.c_int, [C.c_int] + [C.c_int32] * 5 + [_P] * 4 + [C.c_int32] + [_P] * 7 + [C.c_int32] * 3 + [_P] * 7),
    ("biogpt_hip_wide_chain_device", C.c_int, [C.c_int] + [C.c_int32] * 5 + [_P] * 8 + [C.c_int32] * 3 + [_P] * 4),
    ("biogpt_hip_wide_chain_bench", C.c_int, [C.c_int] + [C.c_int32] * 6 + [_P]),
    ("biogpt_hip_fchain_device", C.c_int, [C.c_int] + [C.c_int32] * 6 + [_P] * 8 + [C.c_int32] * 3 + [_P] * 5),
    ("biogpt_hip_fchain_bench", C.c_int, [C.c_int] + [C.c_int32] * 7 + [_P]),
    ("biogpt_hip_assoc_device", C.c_int, [C.c_int] + [C.c_int32] * 9 + [_P] * 17),
    ("biogpt_hip_assoc_bench", C.c_int, [C.c_int] + [C.c_int32] * 6 + [_P]),
    ("biogpt_hip_schain_device", C.c_int, [C.c_int] + [C.c_int32] * 12 + [_P] * 16),
    ("biogpt_hip_schain_bench", C.c_int, [C.c_int] + [C.c_int32] * 7 + [_P]),
    ("biogpt_hip_embed_device", C.c_int, [C.c_int] + [C.c_int32] * 3 + [_P] * 4 + [C.c_int32] * 5 + [_P] + [C.c_int32] * 2 + [_P] * 3 + [C.c_int32] + [_P] * 3),
    ("biogpt_hip_tail_device", C.c_int, [C.c_int] + [C.c_int32] * 3 + [_P] * 7 + [C.c_int32] * 2 + [_P] + [C.c_int32] * 3 + [_P] * 5),
    ("biogpt_hip_attn_prefix_device", C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("biogpt_hip_attn_prefix_bench", C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P]),
    ("biogpt_hip_hidden", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    ("biogpt_hip_embed_batch", C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(EmbedOpts), _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_read_kv", C.c_int, [_P, C.c_int, C.c_size_t, C.c_size_t, _P]),
    ("biogpt_hip_debug_stamps", C.c_int, [_P, C.c_size_t, C.c_size_t, C.POINTER(C.c_ulonglong)]),
    ("biogpt_hip_bench_matvec", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("biogpt_hip_bench_decode", C.c_int, [_P, C.c_int32, C.c_int, C.POINTER(C.c_double)]),
    ("biogpt_hip_bench_api_loop", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    ("biogpt_hip_bench_stream", C.c_int, [_P, C.c_int32, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("biogpt_hip_quantize_file", C.c_int, [C.c_char_p, C.c_char_p, C.c_int32]),
    ("biogpt_hip_quantize_rows_device", C.c_int, [C.c_int, C.c_int32, _P, C.c_int64, C.c_int64, _P]),
    ("biogpt_hip_ln_q8_device", C.c_int, [C.c_int, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_float, C.c_int32, C.c_int32, _P, _P, _P]),
    ("biogpt_hip_q8_forms_device", C.c_int, [C.c_int, _P]),
    ("biogpt_hip_write_synthetic", C.c_int, [C.c_char_p, C.POINTER(HParams), C.c_uint64]),
    # text <-> ids (host-only)
    ("biogpt_hip_vocab_load", _P, [C.c_char_p]),
    ("biogpt_hip_vocab_create", _P, [_P, _P, C.c_int32, _P, _P, C.c_int32]),
    ("biogpt_hip_vocab_free", None, [_P]),
    ("biogpt_hip_ctx_vocab", _P, [_P]),
    ("biogpt_hip_tokenizer_set_data_dir", C.c_int, [C.c_char_p]),
    ("biogpt_hip_tokenize", C.c_int, [_P, C.c_char_p, C.c_char_p, _P, C.c_int32]),
    ("biogpt_hip_decode", C.c_int, [_P, _P, C.c_int32, C.c_char_p, C.c_char_p, C.c_int32]),
    ("biogpt_hip_decode_strings", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32]),
    ("biogpt_hip_moses_tokenize", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32]),
    ("biogpt_hip_moses_detokenize", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32]),
    ("biogpt_hip_bpe", C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_int32]),
    ("biogpt_hip_tokenizer_byte_class", C.c_int, [C.c_int, _P]),
]
E_LENGTH = -7   # BIOGPT_HIP_E_LENGTH


def lib():
    """Load libbiogpt_hip.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BiogptError("%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _flat_ids(seqs):
    """The id lists concatenated, int32; never a zero-sized buffer (its address would be null for a call that names no token at all)."""
    parts = [np.asarray(s, dtype=np.int32).reshape(-1) for s in seqs]
    flat = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    return np.ascontiguousarray(flat if flat.size else np.zeros(1, np.int32))


def _err():
    return lib().biogpt_hip_last_error().decode("utf-8", "replace")


def quantize_file(src, dst, ftype):
    """examples/quantize equivalent (quantize.cpp:8-135): ftype by name or ggml_ftype id."""
    ft = FTYPES[ftype] if isinstance(ftype, str) else int(ftype)
    if lib().biogpt_hip_quantize_file(os.fsencode(src), os.fsencode(dst), ft) != 0:
        raise BiogptError(_err())


def quantize_rows_device(rows, type_id, device=0):
    """ggml_quantize_* on the device: a [nrows, k] float32 array -> the file's block bytes (uint8 array)."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    nrows, k = a.shape
    bb = {2: 18, 3: 20, 6: 22, 7: 24, 8: 34}[int(type_id)]
    out = np.empty(nrows * (k // 32) * bb, dtype=np.uint8)
    if lib().biogpt_hip_quantize_rows_device(int(device), int(type_id), a.ctypes.data, nrows, k, out.ctypes.data) != 0:
        raise BiogptError(_err())
    return out


def ln_q8_device(x, ln_w=None, ln_b=None, q81=False, want_sum=True, eps=1e-5, blocks=False, device=0):
    """The decode launches' LayerNorm + Q8 stage alone (biogpt_hip_ln_q8_device): x [n, 1024] with ln_w / ln_b [1024] or [n, 1024]; blocks=True: the launches'
    activation quantizer on x [n, 32].  Returns (codes int8 [n, k], d float32 [n, k / 32], s uint32 [n, k / 32])."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    n, k = a.shape
    if k != (32 if blocks else 1024):
        raise ValueError("rows of %d values" % (32 if blocks else 1024))
    w = b = None
    if not blocks:
        w, b = np.ascontiguousarray(ln_w, dtype=np.float32), np.ascontiguousarray(ln_b, dtype=np.float32)
        if w.shape != b.shape or w.shape not in ((1024,), (n, 1024)):
            raise ValueError("ln_w and ln_b: [1024] or [n, 1024]")
    q, d, s = np.empty((n, k), np.int8), np.empty((n, k // 32), np.float32), np.empty((n, k // 32), np.uint32)
    if lib().biogpt_hip_ln_q8_device(int(device), 1 if blocks else 0, a.ctypes.data, n, None if blocks else w.ctypes.data, None if blocks else b.ctypes.data,
                                     0 if blocks else int(w.ndim == 2), float(eps), int(bool(q81)), int(bool(want_sum)), q.ctypes.data, d.ctypes.data, s.ctypes.data) != 0:
        raise BiogptError(_err())
    return q, d, s


Q8_FORMS_CHECKS = ("ln_inv_std_short in range", "ln_inv_std every pattern", "q8_round |x| <= 2^22", "q8_round every other pattern", "q8_scales_short in range",
                   "q8_scales every pattern")


def q8_forms_device(device=0):
    """All 2^32 float bit patterns through the short forms of the decode launches' LayerNorm + Q8 arithmetic (biogpt_hip_q8_forms_device): a dict per check of
    Q8_FORMS_CHECKS: tested, mismatches, first (the lowest mismatching pattern, None without one)."""
    out = np.zeros(18, np.uint64)
    if lib().biogpt_hip_q8_forms_device(int(device), out.ctypes.data) != 0:
        raise BiogptError(_err())
    return {name: {"tested": int(out[c]), "mismatches": int(out[6 + c]), "first": None if int(out[12 + c]) == 2 ** 64 - 1 else int(out[12 + c])}
            for c, name in enumerate(Q8_FORMS_CHECKS)}


CHAIN_OPS = {"LNQ": 0, "QKV": 1, "OPROJ": 2, "FC1_LN": 3, "FC1_Q8": 4, "FC2": 5, "LMHEAD": 6}
CHAIN_ROUTES = {"VALU_1": 0, "VALU_8": 1, "MFMA_1": 2, "MFMA_2": 3}
CHAIN_SHAPES = {"QKV": (3072, 1024), "OPROJ": (1024, 1024), "FC1_LN": (4096, 1024), "FC1_Q8": (4096, 1024), "FC2": (1024, 4096)}      # LMHEAD: (any, 1024)


def chain_device(op, route=None, wtype=0, M=0, N=1, w_rows=None, x=None, ln_w=None, ln_b=None, q81=0, aq_q=None, aq_d=None, aq_s=None, bias=None, resid=None,
                 dev_state=None, seq_states=None, col_mode=0, P=0, k_slots=None, v_slots=None, device=0):
    """One stand-alone launch of a linear stage of the many-column chain (biogpt_hip_chain_device; include/biogpt_hip.h has the inputs of each op).  op and route by
    name (CHAIN_OPS, CHAIN_ROUTES; LNQ has no route).  Returns a dict of the outputs WHOLE as the probe allocated them, guard columns and rows included and preset to
    0xff bytes: "out" float32 [cols, ldo] ([cols, 1024] for QKV), "out_q" int8 / "out_d" float32 / "out_s" uint32 for the ops that write Q8 blocks, "k" / "v" (copies
    of k_slots / v_slots after the launch, QKV), "launched" (kernel, threads, grid x, grid y, dynamic LDS bytes, cols, ldo, 0).  Raises BiogptError on a refusal."""
    opn = CHAIN_OPS[op]
    rt = -1 if op == "LNQ" else CHAIN_ROUTES[route]
    cols, ldo = ((N + 15) & ~15) + 1, (0 if op == "LNQ" else ((M + 127) & ~127) + 16)
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    res = {}
    q8_out = op in ("LNQ", "FC1_LN", "FC1_Q8")
    if q8_out:
        mq = 1024 if op == "LNQ" else M
        res["out_q"], res["out_d"], res["out_s"] = np.zeros((cols, mq), np.int8), np.zeros((cols, mq // 32), np.float32), np.zeros((cols, mq // 32), np.uint32)
    else:
        res["out"] = np.zeros((cols, 1024 if op == "QKV" else ldo), np.float32)
    n_slots = 0
    if op == "QKV":
        res["k"], res["v"] = np.array(k_slots, dtype=np.float32, order="C"), np.array(v_slots, dtype=np.float32, order="C")
        n_slots = res["k"].shape[0]
        assert res["k"].shape == res["v"].shape == (n_slots, 16, P, 64)
    launched = np.zeros(8, np.int32)
    o = lambda name: res[name].ctypes.data if name in res else None
    rc = lib().biogpt_hip_chain_device(int(device), opn, rt, int(wtype), int(M), int(N), ptr(w_rows, np.uint8), ptr(x, np.float32), ptr(ln_w, np.float32),
                                       ptr(ln_b, np.float32), int(q81), ptr(aq_q, np.int8), ptr(aq_d, np.float32), ptr(aq_s, np.uint32), ptr(bias, np.float32),
                                       ptr(resid, np.float32), ptr(dev_state, np.int32), ptr(seq_states, np.int32), int(col_mode), int(P), n_slots, o("k"), o("v"),
                                       o("out"), o("out_q"), o("out_d"), o("out_s"), launched.ctypes.data)
    if rc != 0:
        raise BiogptError(_err())
    res["launched"] = launched
    return res


WIDE_EPIS = {"QKV": 0, "RESID": 1, "GELU": 2, "LOGITS": 3}


def wide_chain_device(epi, wtype, M, K, N, w_rows, aq_q, aq_d, aq_s, bias=None, resid=None, dev_state=None, seq_states=None, col_mode=0, P=0, k_slots=None,
                      v_slots=None, device=0):
    """One stand-alone launch of the wide chain's linear stage (biogpt_hip_wide_chain_device; include/biogpt_hip.h has the inputs of each epilogue).  epi by name
    (WIDE_EPIS).  Returns a dict of the outputs WHOLE as the probe allocated them, guard column and rows included and preset to 0xff bytes: "out" float32
    [cols, ldo] ([cols, K] for QKV), "k" / "v" (copies of k_slots / v_slots after the launch, QKV), "launched" (threads, grid x, grid y, LDS bytes, cols, ldo,
    row tiles, 0).  Raises BiogptError on a refusal."""
    cols, ldo = ((N + 15) & ~15) + 1, ((M + 127) & ~127) + 16
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    res = {"out": np.zeros((cols, K if epi == "QKV" else ldo), np.float32)}
    n_slots = 0
    if epi == "QKV":
        res["k"], res["v"] = np.array(k_slots, dtype=np.float32, order="C"), np.array(v_slots, dtype=np.float32, order="C")
        n_slots = res["k"].shape[0]
        assert res["k"].shape == res["v"].shape == (n_slots, K // 64, P, 64)
    launched = np.zeros(8, np.int32)
    o = lambda name: res[name].ctypes.data if name in res else None
    rc = lib().biogpt_hip_wide_chain_device(int(device), WIDE_EPIS[epi], int(wtype), int(M), int(K), int(N), ptr(w_rows, np.uint8), ptr(aq_q, np.int8),
                                            ptr(aq_d, np.float32), ptr(aq_s, np.uint32), ptr(bias, np.float32), ptr(resid, np.float32), ptr(dev_state, np.int32),
                                            ptr(seq_states, np.int32), int(col_mode), int(P), n_slots, o("k"), o("v"), o("out"), launched.ctypes.data)
    if rc != 0:
        raise BiogptError(_err())
    res["launched"] = launched
    return res


def wide_chain_bench(which, wtype, M, K, N, reps=9, device=0):
    """A linear stage alone, timed (biogpt_hip_wide_chain_bench): microseconds of `reps` launches, float32 [reps].  which "wide": the wide chain's kernel at
    any (M, K); "base": the BioGPT-base matrix-core kernel at (1024, 1024) or (1024, 4096)."""
    us = np.zeros(int(reps), np.float32)
    if lib().biogpt_hip_wide_chain_bench(int(device), {"wide": 0, "base": 1}[which], int(wtype), int(M), int(K), int(N), int(reps), us.ctypes.data) != 0:
        raise BiogptError(_err())
    return us


def fchain_device(epi, wtype, M, K, N, w_rows, x, ln_w=None, ln_b=None, bias=None, resid=None, dev_state=None, seq_states=None, col_mode=0, P=0, k_slots=None,
                  v_slots=None, cfg=-1, device=0):
    """One stand-alone launch of the float chain's linear stage (biogpt_hip_fchain_device; include/biogpt_hip.h has the inputs of each epilogue).  epi by name
    (WIDE_EPIS); wtype 0: w_rows float32 [M, K], 1: float16 [M, K] (or its bits as uint16); x float32 [N, K]; ln_w / ln_b: the LayerNorm producer runs first.
    Returns a dict of the outputs WHOLE as the probe allocated them, guard column and rows included and preset to 0xff bytes: "out" float32 [cols, ldo] ([cols, K]
    for QKV), "ln" float32 [cols, K] (with ln_w), "k" / "v" (copies of k_slots / v_slots after the launch, QKV), "launched" (threads, grid x, grid y, LDS bytes,
    cols, ldo, tile shape, 0).  Raises BiogptError on a refusal."""
    cols, ldo = ((N + 15) & ~15) + 1, ((M + 127) & ~127) + 16
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    if w_rows is not None and int(wtype) == 1 and np.asarray(w_rows).dtype == np.uint16:
        w_rows = np.asarray(w_rows).view(np.float16)
    res = {"out": np.zeros((cols, K if epi == "QKV" else ldo), np.float32)}
    if ln_w is not None:
        res["ln"] = np.zeros((cols, K), np.float32)
    n_slots = 0
    if epi == "QKV":
        res["k"], res["v"] = np.array(k_slots, dtype=np.float32, order="C"), np.array(v_slots, dtype=np.float32, order="C")
        n_slots = res["k"].shape[0]
        assert res["k"].shape == res["v"].shape == (n_slots, K // 64, P, 64)
    launched = np.zeros(8, np.int32)
    o = lambda name: res[name].ctypes.data if name in res else None
    rc = lib().biogpt_hip_fchain_device(int(device), WIDE_EPIS[epi], int(wtype), int(M), int(K), int(N), int(cfg), ptr(w_rows, np.float16 if int(wtype) == 1 else np.float32),
                                        ptr(x, np.float32), ptr(ln_w, np.float32), ptr(ln_b, np.float32), ptr(bias, np.float32), ptr(resid, np.float32),
                                        ptr(dev_state, np.int32), ptr(seq_states, np.int32), int(col_mode), int(P), n_slots, o("k"), o("v"), o("out"), o("ln"),
                                        launched.ctypes.data)
    if rc != 0:
        raise BiogptError(_err())
    res["launched"] = launched
    return res


ASSOC_STAGES = {"Q8": 0, "MATVEC": 1, "ATTN": 2}
ASSOC_MODES = {"scalar": 0, "simd": 1}
ASSOC_MAX_PARTS = 1025      # arg-max partials a MATVEC / LOGITS probe returns: the launch's grid limit, plus a guard


def assoc_device(stage, wtype=2, M=0, K=0, N=None, w_rows=None, x=None, ln_w=None, ln_b=None, epi=None, bias=None, resid=None, dev_state=None, P=0, k_slots=None,
                 v_slots=None, q=None, H=0, partials=False, device=0):
    """One stand-alone launch of a kernel of the SIMD association (biogpt_hip_assoc_device; include/biogpt_hip.h has the inputs of each stage).  stage "Q8": x
    float32 [N, K] (ln_w / ln_b: the LayerNorm in front) -> "q" int8 [N + 1, K], "d" float32 and "s" uint32 [N + 1, K / 32].  "MATVEC": w_rows (uint8 bytes of M
    rows in the file's format), x [N, K], epi by name (WIDE_EPIS; the LayerNorm prologue goes with ln_w / ln_b), bias, resid, for QKV dev_state, P and k_slots /
    v_slots [K / 64, P, 64] -> "out" float32 [N + 1, M + 16] ([N + 1, K] for QKV), "k" / "v", with partials=True "pmax_val" / "pmax_idx" [ASSOC_MAX_PARTS].
    "ATTN": q [N, H * 64], k_slots / v_slots [H, P, 64], dev_state -> "out" [N + 1, H * 64].  Outputs come back WHOLE, guard rows included and preset to 0xff
    bytes; "launched" as the header lists it.  Raises BiogptError on a refusal."""
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    st = ASSOC_STAGES[stage] if isinstance(stage, str) else int(stage)
    if N is None:
        N = int(np.shape(q if st == 2 else x)[0])
    M, K, N, H, P = int(M), int(K), int(N), int(H), int(P)
    res = {}
    if st == 0:
        res["q"], res["d"], res["s"] = np.zeros((N + 1, max(K, 0)), np.int8), np.zeros((N + 1, max(K, 0) // 32), np.float32), np.zeros((N + 1, max(K, 0) // 32), np.uint32)
    elif st == 1:
        res["out"] = np.zeros((N + 1, K if epi == "QKV" else M + 16), np.float32)
        if epi == "QKV":
            res["k"], res["v"] = np.array(k_slots, dtype=np.float32, order="C"), np.array(v_slots, dtype=np.float32, order="C")
        if partials:
            res["pmax_val"], res["pmax_idx"] = np.zeros(ASSOC_MAX_PARTS, np.float32), np.zeros(ASSOC_MAX_PARTS, np.int32)
    else:
        res["out"] = np.zeros((N + 1, max(H, 0) * 64), np.float32)
    launched = np.zeros(8, np.int32)
    o = lambda name: res[name].ctypes.data if name in res else None
    kv = (o("k"), o("v")) if st == 1 else (ptr(k_slots, np.float32), ptr(v_slots, np.float32))
    rc = lib().biogpt_hip_assoc_device(int(device), st, int(wtype), 0 if ln_w is None else 1, WIDE_EPIS[epi] if isinstance(epi, str) else int(epi or 0), M, K, N, H, P,
                                       ptr(w_rows, np.uint8), ptr(x, np.float32), ptr(ln_w, np.float32), ptr(ln_b, np.float32), ptr(bias, np.float32),
                                       ptr(resid, np.float32), ptr(dev_state, np.int32), ptr(q, np.float32), kv[0], kv[1], o("out"), o("q"), o("d"), o("s"),
                                       o("pmax_val"), o("pmax_idx"), launched.ctypes.data)
    if rc != 0:
        raise BiogptError(_err())
    res["launched"] = launched
    return res


def assoc_bench(which, wtype, M, K, N, reps=9, device=0):
    """A kernel of the SIMD association alone, timed (biogpt_hip_assoc_bench): microseconds of `reps` launches, float32 [reps].  which "simd": the SIMD mat-vec
    with the residual epilogue at (M, K, N); "scalar": the scalar association's mat-vec of the five-launch route at the same shape; "attn": the SIMD attention
    with M heads, N causal query columns, K keys for the last."""
    us = np.zeros(int(reps), np.float32)
    if lib().biogpt_hip_assoc_bench(int(device), {"simd": 0, "scalar": 1, "attn": 2}[which], int(wtype), int(M), int(K), int(N), int(reps), us.ctypes.data) != 0:
        raise BiogptError(_err())
    return us


SCHAIN_STAGES = {"Q8": 0, "STAGE": 1, "ATTN": 2}


def schain_device(stage, wtype=2, M=0, K=0, N=None, w_rows=None, x=None, ln_w=None, ln_b=None, epi=None, bias=None, resid=None, dev_state=None, seq_states=None,
                  col_mode=0, shared=0, P=0, k_slots=None, v_slots=None, q=None, H=0, cfg=-1, device=0):
    """One stand-alone run of a kernel of the SIMD chain (biogpt_hip_schain_device; include/biogpt_hip.h has the inputs of each stage).  stage "Q8": x float32
    [N, K] (ln_w / ln_b: the LayerNorm in front) -> "q" int8 [N + 1, K], "d" float32 and "s" uint32 [N + 1, K / 32].  "STAGE": the producer, then the linear
    stage at tile shape cfg (-1: the launch's choice): w_rows (uint8 bytes of M rows in the file's format), x [N, K], epi by name (WIDE_EPIS), bias, resid, for QKV
    dev_state or seq_states [N, 8] (+ col_mode), P and k_slots / v_slots [n_slots, K / 64, P, 64] -> "out" float32 [cols, ldo] ([cols, K] for QKV), "k" / "v".
    "ATTN": q [N, H * 64], k_slots / v_slots [n_slots, H, P, 64], seq_states [N, 8], col_mode, shared -> "out" [N + 1, H * 64].  Outputs come back WHOLE, guard
    rows and columns included and preset to 0xff bytes; "launched" as the header lists it.  Raises BiogptError on a refusal."""
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    st = SCHAIN_STAGES[stage] if isinstance(stage, str) else int(stage)
    if N is None:
        N = int(np.shape(q if st == 2 else x)[0])
    M, K, N, H, P = int(M), int(K), int(N), int(H), int(P)
    res, n_slots = {}, 0
    if st == 0:
        res["q"], res["d"], res["s"] = np.zeros((N + 1, max(K, 0)), np.int8), np.zeros((N + 1, max(K, 0) // 32), np.float32), np.zeros((N + 1, max(K, 0) // 32), np.uint32)
    elif st == 1:
        cols, ldo = ((max(N, 0) + 31) & ~31) + 1, ((max(M, 0) + 63) & ~63) + 16
        res["out"] = np.zeros((cols, max(K, 0) if epi == "QKV" else ldo), np.float32)
        if epi == "QKV" and k_slots is not None and v_slots is not None:
            res["k"], res["v"] = np.array(k_slots, dtype=np.float32, order="C"), np.array(v_slots, dtype=np.float32, order="C")
            n_slots = res["k"].shape[0]
            assert res["k"].shape == res["v"].shape == (n_slots, K // 64, P, 64)
    else:
        res["out"] = np.zeros((max(N, 0) + 1, max(H, 0) * 64), np.float32)
        if k_slots is not None:
            n_slots = int(np.shape(k_slots)[0])
    launched = np.zeros(8, np.int32)
    o = lambda name: res[name].ctypes.data if name in res else None
    kv = (o("k"), o("v")) if st == 1 else (ptr(k_slots, np.float32), ptr(v_slots, np.float32))
    rc = lib().biogpt_hip_schain_device(int(device), st, int(wtype), WIDE_EPIS[epi] if isinstance(epi, str) else int(epi or 0), M, K, N, int(cfg), H, P, n_slots,
                                        int(col_mode), int(shared), ptr(w_rows, np.uint8), ptr(x, np.float32), ptr(ln_w, np.float32), ptr(ln_b, np.float32),
                                        ptr(bias, np.float32), ptr(resid, np.float32), ptr(dev_state, np.int32), ptr(seq_states, np.int32), ptr(q, np.float32),
                                        kv[0], kv[1], o("out"), o("q"), o("d"), o("s"), launched.ctypes.data)
    if rc != 0:
        raise BiogptError(_err())
    res["launched"] = launched
    return res


def schain_bench(which, wtype, M, K, N, cfg=-1, reps=9, device=0):
    """A linear stage of the SIMD association alone, timed (biogpt_hip_schain_bench): microseconds of `reps` launches, float32 [reps].  which "stage": the SIMD
    chain's stage with the residual epilogue at tile shape cfg (-1: the launch's choice); "q8": its producer; "matvec": the SIMD mat-vec of a context's own pass at
    N columns; "wide": the scalar association's matrix-core stage (for scale)."""
    us = np.zeros(int(reps), np.float32)
    if lib().biogpt_hip_schain_bench(int(device), {"stage": 0, "q8": 1, "matvec": 2, "wide": 3}[which], int(wtype), int(M), int(K), int(N), int(cfg), int(reps),
                                     us.ctypes.data) != 0:
        raise BiogptError(_err())
    return us


EMBED_STAGES = {"LN": 0, "POOL": 1, "HEAD": 2}
EMBED_POOLING = {"none": 0, "last": 1, "mean": 2}


def embed_device(stage, x, ln_w=None, ln_b=None, seq_states=None, slot_div=0, P=0, n_out_rows=None, pooling="none", normalize=False, lens=None, pass_cols=None,
                 w=None, b=None, n_out=None, device=0):
    """One stand-alone run of a stage of the embedding tail (biogpt_hip_embed_device; include/biogpt_hip.h has the inputs of each stage), through the launch code
    of the engine's own calls.  stage "LN": x float32 [N, W], ln_w / ln_b [W], optionally seq_states int32 [N, 8] (n_past in word 0, seq_id in word 3) with
    slot_div, P and n_out_rows.  "POOL": x the rows of all passes [n_rows, W], pass_cols the columns of each pass, seq_states, lens, pooling by name, normalize.
    "HEAD": x [n_rows, W], w [n_out, W], b [n_out] or None.  Returns a dict of the outputs WHOLE as the probe allocated them, the guard row included and preset
    to 0xff bytes: "out" float32 [rows + 1, W] ([n_rows + 1, n_out] for HEAD), "acc" float64 [n_seqs + 1, W] (mean pooling), "launched" (kernel or template,
    threads, grid x, grid y, LDS bytes, pool_finish_kernel's grid or 0, pool_rows_kernel launches, 0).  Raises BiogptError on a refusal."""
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    x = np.ascontiguousarray(x, dtype=np.float32)
    n_rows, W = (int(v) for v in x.shape)
    mode = EMBED_POOLING[pooling]
    n_seqs = 0 if lens is None else len(lens)
    n_passes = 0 if pass_cols is None else len(pass_cols)
    res = {}
    if stage == "LN":
        n_out_rows = n_rows if n_out_rows is None else int(n_out_rows)
        res["out"] = np.zeros((max(n_out_rows, 0) + 1, W), np.float32)
    elif stage == "POOL":
        res["out"] = np.zeros(((n_rows if mode == 0 else n_seqs) + 1, W), np.float32)
        if mode == 2:
            res["acc"] = np.zeros((n_seqs + 1, W), np.float64)
    else:
        n_out = int(np.shape(w)[0]) if n_out is None else int(n_out)
        res["out"] = np.zeros((n_rows + 1, max(n_out, 1)), np.float32)
    launched = np.zeros(8, np.int32)
    rc = lib().biogpt_hip_embed_device(int(device), EMBED_STAGES[stage], W, n_rows, x.ctypes.data, ptr(ln_w, np.float32), ptr(ln_b, np.float32), ptr(seq_states, np.int32),
                                       int(slot_div), int(P), int(n_out_rows or 0), mode, int(normalize), ptr(lens, np.int32), n_seqs, n_passes, ptr(pass_cols, np.int32),
                                       ptr(w, np.float32), ptr(b, np.float32), int(n_out or 0), res["out"].ctypes.data, res["acc"].ctypes.data if "acc" in res else None,
                                       launched.ctypes.data)
    if rc != 0:
        raise BiogptError(_err())
    res["launched"] = launched
    return res


TAIL_STAGES = {"PARTIALS": 0, "FINISH": 1, "TOPK": 2, "HOST_TOPK": 3, "HOST_BLOCKS": 4, "HOST_FULL": 5}


def tail_device(stage, wtype=0, w_rows=None, M=None, x=None, ln_w=None, ln_b=None, row=None, pmax_val=None, pmax_idx=None, nparts=None, k=0, state=(0, 0, 0, 0), n_eval=1,
                n_positions=8, n_vocab=42384, device=0):
    """One stand-alone run of a stage of the token tail (biogpt_hip_tail_device; include/biogpt_hip.h has the inputs of each stage), through the launch code of
    the engine's own calls.  "PARTIALS": w_rows (M rows of 1024 weights in the file's format, wtype 0 for float32), x, ln_w, ln_b -> "row", "pmax_val", "pmax_idx"
    WHOLE ([M + 16], unwritten entries 0xff bytes), "grid" and "rows_per_part".  "FINISH": pmax_val, pmax_idx, state, n_eval, n_positions, n_vocab -> "block" (the
    state block whole), "token", "n_past", "n_gen", "recorded" (gen_ids[state's n_gen], or None beyond n_positions).  "TOPK" / "HOST_TOPK" / "HOST_BLOCKS" /
    "HOST_FULL": row, k (and pmax_val [nparts]) -> "n" (k, -1, or the count found), "vals" / "ids" whole ([80]).  "launched" always.  Raises BiogptError on a refusal."""
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    st = TAIL_STAGES[stage]
    launched = np.zeros(8, np.int32)
    res = {"launched": launched}
    if st == 0:
        n = int(M if M is not None else (np.shape(w_rows)[0] if w_rows is not None else 0))
        cap = max(n, 0) + 16
        out_val, out_idx = np.zeros(cap, np.float32), np.zeros(1, np.int32)
        part_val, part_idx = np.zeros(cap, np.float32), np.zeros(cap, np.int32)
        w_ptr = ptr(w_rows, np.float32 if int(wtype) == 0 else np.uint8)
    elif st == 1:
        n = int(nparts if nparts is not None else (len(pmax_val) if pmax_val is not None else 0))
        out_val, out_idx = np.zeros(1, np.float32), np.zeros(4 + 2 * max(int(n_positions), 0) + 16, np.int32)
        part_val, part_idx = np.zeros(1, np.float32), np.zeros(1, np.int32)
        w_ptr = None
    else:
        n = int(len(row) if row is not None else 0)
        nparts = int(nparts if nparts is not None else (len(pmax_val) if pmax_val is not None else 0))
        out_val, out_idx = np.zeros(80, np.float32), np.zeros(80, np.int32)
        part_val, part_idx = np.zeros(1, np.float32), np.zeros(16, np.int32)
        w_ptr = None
    rc = lib().biogpt_hip_tail_device(int(device), st, int(wtype), n, w_ptr, ptr(x, np.float32), ptr(ln_w, np.float32), ptr(ln_b, np.float32), ptr(row, np.float32),
                                      ptr(pmax_val, np.float32), ptr(pmax_idx, np.int32), int(nparts or 0), int(k), ptr(state, np.int32), int(n_eval), int(n_positions),
                                      int(n_vocab), out_val.ctypes.data, out_idx.ctypes.data, part_val.ctypes.data, part_idx.ctypes.data, launched.ctypes.data)
    if rc != 0:
        raise BiogptError(_err())
    if st == 0:
        res.update(row=out_val, pmax_val=part_val, pmax_idx=part_idx, kernel=int(launched[0]), grid=int(launched[1]), rows_per_part=int(launched[2]))
    elif st == 1:
        g0, P = int(np.asarray(state)[1]), int(n_positions)
        res.update(block=out_idx, n_past=int(out_idx[0]), n_gen=int(out_idx[1]), token=int(out_idx[4]), recorded=int(out_idx[4 + P + g0]) if g0 < P else None)
    else:
        res.update(n=int(part_idx[0]), vals=out_val, ids=out_idx, count=part_idx)
    return res


def fchain_bench(which, wtype, M, K, N, cfg=-1, reps=9, device=0):
    """A linear stage of a float file alone, timed (biogpt_hip_fchain_bench): microseconds of `reps` launches, float32 [reps].  which "float": the float chain's
    kernel at tile shape cfg (-1: the launch's choice); "generic": the generic mat-vec kernel a prompt pass of the context's own columns takes."""
    us = np.zeros(int(reps), np.float32)
    if lib().biogpt_hip_fchain_bench(int(device), {"float": 0, "generic": 1}[which], int(wtype), int(M), int(K), int(N), int(cfg), int(reps), us.ctypes.data) != 0:
        raise BiogptError(_err())
    return us


def write_synthetic(path, seed=0x42494F47, **hparams):
    """Write a seeded synthetic model file. hparams default to BioGPT-base."""
    hp = HParams(**{**BIOGPT_BASE, **hparams})
    if lib().biogpt_hip_write_synthetic(os.fsencode(path), C.byref(hp), C.c_uint64(seed)) != 0:
        raise BiogptError(_err())
    return hp


class TokenizerLengthError(BiogptError):
    """The reference's moses_tokenize throws std::length_error for this text (mosestokenizer.cpp:264)."""


def _bytes(s):
    return s if isinstance(s, bytes) else s.encode("utf-8")


def _string_result(fn, *args):
    """C-ABI string protocol: the call returns the needed length; retry once with a buffer that fits."""
    cap = 4096
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        n = fn(*args, buf, cap)
        if n == E_LENGTH:
            raise TokenizerLengthError(_err())
        if n < 0:
            raise BiogptError(_err())
        if n + 1 <= cap:
            return buf.raw[:n]
        cap = n + 1
    raise BiogptError("string result did not fit")


def set_tokenizer_data_dir(path):
    """Directory holding nonbreaking_prefixes/ (the reference's data/); default $BIOGPT_DATA_DIR or ../data."""
    lib().biogpt_hip_tokenizer_set_data_dir(os.fsencode(path))


def moses_tokenize(text, lang=""):
    """moses_tokenize (mosestokenizer.cpp:290-358): list of byte strings."""
    raw = _string_result(lib().biogpt_hip_moses_tokenize, _bytes(text), _bytes(lang))
    return raw.split(b"\n") if raw else []


def moses_detokenize(tokens, lang=""):
    """moses_detokenize (mosestokenizer.cpp:360-466)."""
    return _string_result(lib().biogpt_hip_moses_detokenize, b"\n".join(_bytes(t) for t in tokens), _bytes(lang))


def decode_strings(tokens, lang=""):
    """gpt_decode (biogpt.cpp:877-906) on vocabulary strings."""
    return _string_result(lib().biogpt_hip_decode_strings, b"\n".join(_bytes(t) for t in tokens), _bytes(lang))


def byte_class(which):
    """256 flags of a perluniprops byte class: 0 IsAlnum, 1 IsAlpha, 2 IsLower, 3 IsN, 4 IsSc."""
    out = (C.c_uint8 * 256)()
    if lib().biogpt_hip_tokenizer_byte_class(which, out) != 0:
        raise BiogptError("bad class index")
    return bytes(out)


class Vocab:
    """biogpt_vocab (biogpt.h:37-48) for the tokenizer: gpt_tokenize / gpt_decode / bpe.  Host-only."""

    def __init__(self, handle, owned):
        self._h, self._owned = handle, owned

    @classmethod
    def load(cls, path):
        h = lib().biogpt_hip_vocab_load(os.fsencode(path))
        if not h:
            raise BiogptError(_err())
        return cls(h, True)

    @classmethod
    def create(cls, tokens, merges):
        """tokens: id -> bytes; merges: rank -> b"left right" records (what the model file stores)."""
        tokens = [_bytes(t) for t in tokens]
        merges = [_bytes(m) for m in merges]
        tp = (C.c_char_p * max(1, len(tokens)))(*tokens)
        tl = (C.c_int32 * max(1, len(tokens)))(*[len(t) for t in tokens])
        mp = (C.c_char_p * max(1, len(merges)))(*merges)
        ml = (C.c_int32 * max(1, len(merges)))(*[len(m) for m in merges])
        h = lib().biogpt_hip_vocab_create(tp, tl, len(tokens), mp, ml, len(merges))
        if not h:
            raise BiogptError(_err())
        return cls(h, True)

    def close(self):
        if self._h and self._owned:
            lib().biogpt_hip_vocab_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bpe(self, word):
        return _string_result(lib().biogpt_hip_bpe, self._h, _bytes(word))

    def tokenize(self, text, lang=""):
        """gpt_tokenize (biogpt.cpp:850-875): ids, starting with 2."""
        cap = 256
        for _ in range(2):
            out = (C.c_int32 * cap)()
            n = lib().biogpt_hip_tokenize(self._h, _bytes(text), _bytes(lang), out, cap)
            if n == E_LENGTH:
                raise TokenizerLengthError(_err())
            if n < 0:
                raise BiogptError(_err())
            if n <= cap:
                return list(out[:n])
            cap = n
        raise BiogptError("id result did not fit")

    def decode(self, ids, lang=""):
        arr = (C.c_int32 * max(1, len(ids)))(*ids)
        return _string_result(lib().biogpt_hip_decode, self._h, arr, len(ids), _bytes(lang))


def arena_bytes_for(hp):
    return int(lib().biogpt_hip_arena_bytes_for(C.byref(hp)))


def _logprobs_keyword(plain):
    """Adds the keyword-only logprobs=None to the generation method `plain`, whose own parameters, defaults and return value stay what they are (functools.wraps:
    introspection reports the plain method; logprobs is the one keyword more the call accepts, behind all of them).  None: the method itself.  K: the method
    of the same name with a leading underscore, given the same arguments and logprobs=K, which returns (ids, info, seconds)."""
    @functools.wraps(plain)
    def call(self, *args, logprobs=None, **kw):
        if logprobs is None:
            return plain(self, *args, **kw)
        return getattr(BiogptModel, "_" + plain.__name__)(self, *args, logprobs=logprobs, **kw)
    return call


def _queue_keywords(plain):
    """Adds the keyword-only prefix=None, logprobs=None and params=None to generate_queue, as _logprobs_keyword adds logprobs: the method's own parameters,
    defaults and return value stay what they are.  None given: the method itself.  Otherwise _generate_queue with the same arguments and the keywords."""
    @functools.wraps(plain)
    def call(self, *args, prefix=None, logprobs=None, params=None, **kw):
        if prefix is None and logprobs is None and params is None:
            return plain(self, *args, **kw)
        return BiogptModel._generate_queue(self, *args, prefix=prefix, logprobs=logprobs, params=params, **kw)
    return call


def _sampler_keyword(plain):
    """Adds the keyword-only sampler=None to generate_sample, as _logprobs_keyword adds logprobs: the method's own parameters stay what they are.  None: the
    method itself.  A sampler: _generate_sample with the same arguments and sampler=."""
    @functools.wraps(plain)
    def call(self, *args, sampler=None, **kw):
        if sampler is None:
            return plain(self, *args, **kw)
        return BiogptModel._generate_sample(self, *args, sampler=sampler, **kw)
    return call


class BiogptModel:
    """biogpt_model + biogpt_vocab handle (biogpt.h:78-107, :37-48) living on one HIP device."""

    def __init__(self, handle):
        if not handle:
            raise BiogptError(_err())
        self._h = handle
        self.hparams = HParams()
        lib().biogpt_hip_get_hparams(self._h, C.byref(self.hparams))
        self.n_vocab = self.hparams.n_vocab
        self.n_tensors = lib().biogpt_hip_n_tensors(self._h)

    # -- biogpt_model_load (biogpt.h:128-132) --
    @classmethod
    def load(cls, fname, device=0, verbosity=0, arena=None, arena_bytes=0, float_chain=False, assoc=None, assoc_chain=None):
        """float_chain=True: switch the float chain on behind the load (float_chain(); an F32 / F16 file with head size 64 only -- anything else raises).
        assoc="scalar" | "simd": set the association behind the load (set_assoc(); None: the default, scalar unless BIOGPT_HIP_ASSOC=1).
        assoc_chain=True | False: set the SIMD chain's switch behind the load (set_assoc_chain(); None: the default, off unless BIOGPT_HIP_ASSOC_CHAIN=1)."""
        if arena is None:
            m = cls(lib().biogpt_hip_load(os.fsencode(fname), device, verbosity))
        else:
            m = cls(lib().biogpt_hip_load_into(os.fsencode(fname), device, verbosity, arena, arena_bytes))
        try:
            if float_chain:
                m.float_chain(True)
            if assoc is not None:
                m.set_assoc(assoc)
            if assoc_chain is not None:
                m.set_assoc_chain(assoc_chain)
        except BiogptError:
            m.close()
            raise
        return m

    @classmethod
    def attach(cls, hparams, device, arena, arena_bytes):
        return cls(lib().biogpt_hip_attach(C.byref(hparams), device, arena, arena_bytes))

    # -- biogpt_eval (biogpt.h:145-151): logits of the last token --
    def eval(self, tokens, n_past):
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.n_vocab, dtype=np.float32)
        if lib().biogpt_hip_eval(self._h, toks.ctypes.data, toks.size, int(n_past), out.ctypes.data) != 0:
            raise BiogptError(_err())
        return out

    def eval_topk(self, tokens, n_past, k):
        """biogpt_eval + device-side top-k: (values descending, ids) of the k <= 64 largest logits of the last token."""
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        vals = np.zeros(64, dtype=np.float32)
        ids = np.zeros(64, dtype=np.int32)
        got = lib().biogpt_hip_eval_topk(self._h, toks.ctypes.data, toks.size, int(n_past), int(k), vals.ctypes.data, ids.ctypes.data)
        if got < 0:
            raise BiogptError(_err())
        return vals[:got].copy(), ids[:got].copy()

    def eval_all(self, tokens, n_past):
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty((toks.size, self.n_vocab), dtype=np.float32)
        if lib().biogpt_hip_eval_all(self._h, toks.ctypes.data, toks.size, int(n_past), out.ctypes.data) != 0:
            raise BiogptError(_err())
        return out

    def eval_prompt(self, tokens, n_past=0, n_batch=8, want_logits=True):
        """== eval() on consecutive chunks of n_batch tokens (main.cpp prompt loop), several chunks per pass.
        Returns the last token's logits, or None (asynchronous) with want_logits=False."""
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.n_vocab, dtype=np.float32) if want_logits else None
        if lib().biogpt_hip_eval_prompt(self._h, toks.ctypes.data, toks.size, int(n_past), int(n_batch),
                                        out.ctypes.data if want_logits else None) != 0:
            raise BiogptError(_err())
        return out

    def eval_device(self, tokens, n_past):
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        if lib().biogpt_hip_eval_device(self._h, toks.ctypes.data, toks.size, int(n_past)) != 0:
            raise BiogptError(_err())

    def read_logits(self):
        """The device-side logits row of the last evaluated token (biogpt_hip_logits_device), copied to host memory."""
        out = np.empty(self.n_vocab, dtype=np.float32)
        if lib().biogpt_hip_read_logits(self._h, out.ctypes.data) != 0:
            raise BiogptError(_err())
        return out

    def resident_stats(self):
        """{hits, misses, streak, need} of the resident launch's speculative continuation (biogpt_hip_resident_stats)."""
        out = (C.c_int64 * 4)()
        if lib().biogpt_hip_resident_stats(self._h, out) != 0:
            raise BiogptError(_err())
        return dict(hits=int(out[0]), misses=int(out[1]), streak=int(out[2]), need=int(out[3]))

    def lineage_stats(self):
        """{graph_evals, stale_rows}: single-token evals replayed as captured five-launch steps / rows found to be another call's and repeated (biogpt_hip_lineage_stats)."""
        out = (C.c_int64 * 2)()
        if lib().biogpt_hip_lineage_stats(self._h, out) != 0:
            raise BiogptError(_err())
        return dict(graph_evals=int(out[0]), stale_rows=int(out[1]))

    def synchronize(self):
        if lib().biogpt_hip_synchronize(self._h) != 0:
            raise BiogptError(_err())

    # -- main.cpp:91-151 with --top_k 1 --
    def generate_greedy(self, prompt, n_predict, n_batch=8):
        pr = np.ascontiguousarray(prompt, dtype=np.int32)
        out = np.zeros(max(int(n_predict), 1), dtype=np.int32)
        secs = C.c_double(0.0)
        n = lib().biogpt_hip_generate_greedy(self._h, pr.ctypes.data, pr.size, int(n_batch), int(n_predict),
                                             out.ctypes.data, C.byref(secs))
        if n < 0:
            raise BiogptError(_err())
        return out[:n].copy(), secs.value

    @_logprobs_keyword
    def generate_greedy_batch(self, prompts, n_predict, n_batch=8, prefix=None):
        """Batched decode of several independent prompts (list of id lists) on this device.  prefix: a list of ids that stands in front of every
        prompt -- sequence s is prefix + prompts[s], and a prompt may then be empty.  The ids are those of the call on the concatenations; the
        prefix is evaluated once ("Generation behind a shared prefix"; prefix_stats()).  logprobs (keyword only): None, or K in [0, 8] -- the
        call then returns (ids, info, seconds) with info[s] = (logprobs float32[n], top_ids int32[n, K], top_logprobs float32[n, K]), n the
        n_predict as clamped: the model's log-probability of every generated token, as score_batch gives it, and every row's K best entries
        ("Log-probabilities of generated tokens"); the ids are those of the call without it."""
        return BiogptModel._generate_greedy_batch(self, prompts, n_predict, n_batch, prefix)

    def _generate_greedy_batch(self, prompts, n_predict, n_batch=8, prefix=None, logprobs=None):
        """generate_greedy_batch, and with logprobs=K its form that returns (ids, info, seconds)."""
        lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
        secs = C.c_double(0.0)
        if logprobs is not None:
            n_seqs = len(prompts)
            out = np.zeros((max(n_seqs, 1), max(int(n_predict), 1)), dtype=np.int32)
            arr = _LogprobArrays(logprobs, n_seqs, out.shape[1])
            pre = None if prefix is None else _flat_ids([prefix])
            flat = _flat_ids(prompts)
            n = lib().biogpt_hip_generate_greedy_batch_lp(self._h, None if pre is None else pre.ctypes.data, 0 if prefix is None else len(prefix), flat.ctypes.data,
                                                          lens.ctypes.data, n_seqs, int(n_batch), int(n_predict), out.ctypes.data, C.byref(secs), C.byref(arr.req))
            if n < 0:
                raise BiogptError(_err())
            return out.reshape(-1)[:n_seqs * n].reshape(n_seqs, n).copy(), arr.info(n_seqs, n, [n] * n_seqs), secs.value
        if prefix is not None:
            out = np.zeros((max(len(prompts), 1), max(int(n_predict), 1)), dtype=np.int32)
            n_pre, pre = len(prefix), _flat_ids([prefix])
            flat = _flat_ids(prompts)
            n = lib().biogpt_hip_generate_greedy_prefix(self._h, pre.ctypes.data, n_pre, flat.ctypes.data, lens.ctypes.data, len(prompts), int(n_batch),
                                                        int(n_predict), out.ctypes.data, C.byref(secs))
            if n < 0:
                raise BiogptError(_err())
            return out.reshape(-1)[:len(prompts) * n].reshape(len(prompts), n).copy(), secs.value
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
        out = np.zeros((len(prompts), max(int(n_predict), 1)), dtype=np.int32)
        n = lib().biogpt_hip_generate_greedy_batch(self._h, flat.ctypes.data, lens.ctypes.data, len(prompts), int(n_batch),
                                                   int(n_predict), out.ctypes.data, C.byref(secs))
        if n < 0:
            raise BiogptError(_err())
        return out.reshape(-1)[:len(prompts) * n].reshape(len(prompts), n).copy(), secs.value

    def prefix_stats(self):
        """Of the last generate_greedy_batch / generate_sample with prefix= on this model: n_shared (prefix rows evaluated once), prompt_columns (all
        prompt columns evaluated), path (the route of the decode steps -- 0: the launch chain, shared rows read in place; 1: column-per-XCD launches, shared
        rows copied into every column's slot, also reported when n_shared is 0 and nothing was copied), columns."""
        out = np.zeros(4, dtype=np.int32)
        if lib().biogpt_hip_prefix_stats(self._h, out.ctypes.data) != 0:
            raise BiogptError(_err())
        return dict(n_shared=int(out[0]), prompt_columns=int(out[1]), path=int(out[2]), columns=int(out[3]))

    def generate_beam(self, prompt, n_predict, n_beams=5, eos_id=2, length_penalty=1.0, early_stopping=True, n_batch=8,
                      repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=(), trie=None):
        """Beam search (transformers' num_beams with do_sample=False).  Returns ([(ids int32[len], score), ...] best first,
        seconds): each hypothesis's generated ids (an EOS that ended it included) and its normalized score.  The four rule arguments are
        transformers' logits processors of the same names, applied to each beam row's log-probabilities ("Generation rules").
        trie: a Trie -- the output is restricted to its entries ("Constrained decoding": keep the hypotheses with a finite score)."""
        if trie is not None:
            hyps, secs = self.generate_beam_batch([list(prompt)], n_predict, n_beams, eos_id, length_penalty, early_stopping, n_batch, repetition_penalty,
                                                  no_repeat_ngram_size, min_new_tokens, suppress_tokens, trie=trie)
            return hyps[0], secs
        rules, keep = gen_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)
        pr = np.ascontiguousarray(prompt, dtype=np.int32)
        w = max(int(n_predict), 1)
        out = np.zeros((max(int(n_beams), 1), w), dtype=np.int32)
        lens = np.zeros(max(int(n_beams), 1), dtype=np.int32)
        scores = np.zeros(max(int(n_beams), 1), dtype=np.float32)
        secs = C.c_double(0.0)
        n = lib().biogpt_hip_generate_beam_rules(self._h, pr.ctypes.data, pr.size, int(n_batch), int(n_beams), int(n_predict), int(eos_id),
                                                 float(length_penalty), 1 if early_stopping else 0, out.ctypes.data, lens.ctypes.data,
                                                 scores.ctypes.data, C.byref(secs), C.byref(rules))
        if n < 0:
            raise BiogptError(_err())
        if n == 0:
            return [], secs.value
        stride = min(int(n_predict), self.hparams.n_positions - pr.size)   # rows are [n_beams][n_predict as clamped]
        flat = out.reshape(-1)
        return [(flat[r * stride:r * stride + int(lens[r])].copy(), float(scores[r])) for r in range(n)], secs.value

    def generate_beam_batch(self, prompts, n_predict, n_beams=5, eos_id=2, length_penalty=1.0, early_stopping=True, n_batch=8,
                            repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=(), trie=None):
        """Beam search over a batch of prompts (list of id lists, or one flat id list) in one call: every prompt is a search of its own, all of them
        columns of the same decode steps ("Beam search over a batch").  Returns ([[(ids int32[len], score), ...] best first, one list
        per prompt], seconds); prompt p's list is generate_beam(prompts[p], n_predict as clamped for the longest prompt, ...), bit for bit.  trie: a Trie
        shared by all prompts -- every search is restricted to its entries (biogpt_hip_generate_beam_trie)."""
        rules, keep = gen_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)
        if len(prompts) and np.isscalar(prompts[0]):
            prompts = [prompts]
        G, B = len(prompts), max(int(n_beams), 1)
        lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]) if G else np.zeros(0, np.int32))
        w = max(int(n_predict), 1)
        out = np.zeros((max(G, 1) * B, w), dtype=np.int32)
        ol = np.zeros(max(G, 1) * B, dtype=np.int32)
        scores = np.zeros(max(G, 1) * B, dtype=np.float32)
        counts = np.zeros(max(G, 1), dtype=np.int32)
        secs = C.c_double(0.0)
        if trie is not None:
            _no_rules_with_trie(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)
            got = lib().biogpt_hip_generate_beam_trie(self._h, flat.ctypes.data, lens.ctypes.data, G, int(n_batch), int(n_beams), int(n_predict), int(eos_id),
                                                      float(length_penalty), 1 if early_stopping else 0, _trie_handle(trie), out.ctypes.data, ol.ctypes.data,
                                                      scores.ctypes.data, counts.ctypes.data, C.byref(secs))
        else:
            got = lib().biogpt_hip_generate_beam_batch(self._h, flat.ctypes.data, lens.ctypes.data, G, int(n_batch), int(n_beams), int(n_predict), int(eos_id),
                                                       float(length_penalty), 1 if early_stopping else 0, C.byref(rules), out.ctypes.data, ol.ctypes.data,
                                                       scores.ctypes.data, counts.ctypes.data, C.byref(secs))
        if got < 0:
            raise BiogptError(_err())
        if got == 0:
            return [[] for _ in range(G)], secs.value
        rows = out.reshape(-1)      # rows are [G][n_beams][n_predict as clamped]
        return [[(rows[(p * B + r) * got:(p * B + r) * got + int(ol[p * B + r])].copy(), float(scores[p * B + r])) for r in range(int(counts[p]))]
                for p in range(G)], secs.value

    def generate_contrastive(self, prompts, n_predict, top_k=4, penalty_alpha=0.6, eos_id=-1, n_batch=8):
        """Contrastive search (transformers' generate(penalty_alpha, top_k)) over a batch of prompts (list of id lists, or one flat id list), the
        degeneration penalty and the selection on the device ("Contrastive search").  Returns ([ids int32[len], ...] one per prompt,
        [scores float32[len], ...] the winning score of every token); an EOS that ended a prompt's search is included."""
        if len(prompts) and np.isscalar(prompts[0]):
            prompts = [prompts]
        G = len(prompts)
        lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]) if G else np.zeros(0, np.int32))
        w = max(int(n_predict), 1)
        out = np.zeros((max(G, 1), w), dtype=np.int32)
        sc = np.zeros((max(G, 1), w), dtype=np.float32)
        ol = np.zeros(max(G, 1), dtype=np.int32)
        secs = C.c_double(0.0)
        got = lib().biogpt_hip_generate_contrastive(self._h, flat.ctypes.data, lens.ctypes.data, G, int(n_batch), int(top_k), float(penalty_alpha), int(n_predict),
                                                    int(eos_id), out.ctypes.data, ol.ctypes.data, sc.ctypes.data, C.byref(secs))
        if got < 0:
            raise BiogptError(_err())
        if got == 0:
            return [np.zeros(0, np.int32) for _ in range(G)], [np.zeros(0, np.float32) for _ in range(G)]
        rows, srows = out.reshape(-1), sc.reshape(-1)      # rows are [G][n_predict as clamped]
        return ([rows[p * got:p * got + int(ol[p])].copy() for p in range(G)], [srows[p * got:p * got + int(ol[p])].copy() for p in range(G)])

    def generate_lookup(self, prompts, n_predict, max_draft=7, max_ngram=3, corpus=None, eos_id=-1, n_batch=8):
        """Prompt-lookup speculative decoding (transformers' generate(prompt_lookup_num_tokens=max_draft, max_matching_ngram_size=max_ngram)) over a batch
        of prompts (list of id lists, or one flat id list): the ids of generate_greedy_batch, in fewer passes where the output copies from the prompt,
        from what was generated so far or from corpus[p] (an id list per prompt of material likely to be copied; INTEGRATION.md, "Prompt-lookup decoding").
        Returns ([ids int32[len], ...] one per prompt, [{"passes", "drafted", "accepted"}, ...], seconds); an EOS that ended a prompt is included."""
        if len(prompts) and np.isscalar(prompts[0]):
            prompts = [prompts]
            if corpus is not None and (len(corpus) == 0 or np.isscalar(corpus[0])):
                corpus = [corpus]
        G = len(prompts)
        lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]) if G else np.zeros(0, np.int32))
        cflat = clens = None
        if corpus is not None:
            if len(corpus) != G:
                raise BiogptError("generate_lookup: one corpus per prompt (%d != %d)" % (len(corpus), G))
            clens = np.asarray([len(c) for c in corpus], dtype=np.int32)
            cflat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.int32) for c in corpus] + [np.zeros(1, np.int32)]))
        w = max(int(n_predict), 1)
        out = np.zeros((max(G, 1), w), dtype=np.int32)
        ol = np.zeros(max(G, 1), dtype=np.int32)
        st = np.zeros((max(G, 1), 3), dtype=np.int32)
        secs = C.c_double(0.0)
        got = lib().biogpt_hip_generate_lookup(self._h, flat.ctypes.data, lens.ctypes.data, G, None if cflat is None else cflat.ctypes.data,
                                               None if clens is None else clens.ctypes.data, int(n_batch), int(n_predict), int(max_draft), int(max_ngram),
                                               int(eos_id), out.ctypes.data, ol.ctypes.data, st.ctypes.data, C.byref(secs))
        if got < 0:
            raise BiogptError(_err())
        if got == 0:
            return [np.zeros(0, np.int32) for _ in range(G)], [dict(passes=0, drafted=0, accepted=0) for _ in range(G)], secs.value
        rows = out.reshape(-1)      # rows are [G][n_predict as clamped]
        return ([rows[p * got:p * got + int(ol[p])].copy() for p in range(G)],
                [dict(passes=int(st[p, 0]), drafted=int(st[p, 1]), accepted=int(st[p, 2])) for p in range(G)], secs.value)

    @_queue_keywords
    def generate_queue(self, prompts, n_predict, max_columns=64, group=4, top_k=1, top_p=0.9, temp=0.9, seed=0, seeds=None, eos_id=-1, n_batch=8, n_predicts=None):
        """Generation over a queue of requests (continuous batching; INTEGRATION.md, "Generation over a queue"): prompts is a list of id lists of any length,
        at most max_columns of them run at a time, and a request that finishes -- by eos_id, or after its own n_predicts[r] (None: n_predict) tokens as
        clamped to ITS prompt -- hands its column to the next one.  Request r's ids are those of generate_sample([prompts[r]], n_r, top_k, top_p, temp,
        seeds=[seeds[r]], eos_id, n_batch) alone, whatever else is in the queue; seeds=None: seed + r.  top_k=1 (the default) never draws: greedy decoding
        with an EOS.  group: steps between two looks at the columns.  Returns ([ids int32[len], ...] in request order, {"stats": {...}, "admit_step":
        [...], "column": [...]}, seconds); a request without room for a token gets no ids and -1 in both lists.
        prefix (keyword only): a list of ids in front of every prompt -- request r is prefix + prompts[r], a prompt may then be empty, the prefix's first
        rows (a multiple of n_batch) are evaluated once and read in place by every column, and max_columns is at most 511 ("Generation
        over a queue"; prefix_stats()).  The ids, admit_step, column and stats are those of the call on the concatenations, but for
        stats["prompt_columns"], the prompt columns really evaluated.
        logprobs (keyword only): None, or K in [0, 8] -- info["logprobs"][r] = (logprobs float32[len_r], top_ids int32[len_r, K], top_logprobs float32[len_r,
        K]) as generate_sample(logprobs=K) of the request alone gives them, bit for bit; the ids are those of the call without it.
        params (keyword only): one request_params() entry for all requests or a list with one per request -- every request has its own sampler, EOS id,
        generation rules and stop sequences (biogpt_hip_generate_queue_requests), and the method's own top_k / top_p / temp / eos_id must be left at their
        defaults.  Request r's ids are those of generate_sample of r alone with r's parameters and rules, cut just behind the first position at which one of
        its stop sequences is complete inside the generated tokens; info["finish"][r] says why it ended: 0 its limit, 1 its EOS id, 2 + i stop sequence i,
        -1 it never ran.  logprobs= together with a request that has a rule switched on is an error; no trie, wide sampler or several samples."""
        return BiogptModel._generate_queue(self, prompts, n_predict, max_columns, group, top_k, top_p, temp, seed, seeds, eos_id, n_batch, n_predicts)

    def _generate_queue(self, prompts, n_predict, max_columns=64, group=4, top_k=1, top_p=0.9, temp=0.9, seed=0, seeds=None, eos_id=-1, n_batch=8, n_predicts=None,
                        prefix=None, logprobs=None, params=None):
        """generate_queue, with prefix= and logprobs= its form behind a shared prefix and with log-probabilities (biogpt_hip_generate_queue_prefix), with
        params= the form whose requests carry their own parameters (biogpt_hip_generate_queue_requests)."""
        if params is not None and (top_k, top_p, temp, eos_id) != (1, 0.9, 0.9, -1):
            raise BiogptError("params= carries every request's top_k / top_p / temp / eos_id: leave the method's own at their defaults")
        if len(prompts) and np.isscalar(prompts[0]):
            prompts = [prompts]
        R = len(prompts)
        lens = np.asarray([len(p) for p in prompts] or [0], dtype=np.int32)
        flat = _flat_ids(prompts)
        if seeds is None:
            seeds = [(int(seed) + r) & 0xFFFFFFFF for r in range(R)]
        sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        if sd.size != R:
            raise BiogptError("seeds must have one entry per request (%d != %d)" % (sd.size, R))
        np_arr = None
        if n_predicts is not None:
            np_arr = np.ascontiguousarray(n_predicts, dtype=np.int32).reshape(-1)
            if np_arr.size != R:
                raise BiogptError("n_predicts must have one entry per request (%d != %d)" % (np_arr.size, R))
        if sd.size == 0:
            sd = np.zeros(1, np.uint32)
        w = max(int(n_predict), 0)
        out = np.zeros((max(R, 1), max(w, 1)), dtype=np.int32)
        ol, adm, col = (np.zeros(max(R, 1), dtype=np.int32) for _ in range(3))
        st = QueueStats()
        secs = C.c_double(0.0)
        arr = fin = None
        pre = None if prefix is None else _flat_ids([prefix])
        if logprobs is not None:
            arr = _LogprobArrays(logprobs, R, max(w, 1))
        if params is not None:
            pa, keep = _params_array(params, R)
            fin = np.zeros(max(R, 1), dtype=np.int32)
            rc = lib().biogpt_hip_generate_queue_requests(self._h, None if pre is None else pre.ctypes.data, 0 if prefix is None else len(prefix), flat.ctypes.data,
                                                          lens.ctypes.data, R, None if np_arr is None or R == 0 else np_arr.ctypes.data, int(n_predict), int(max_columns),
                                                          int(group), int(n_batch), pa, sd.ctypes.data, out.ctypes.data, ol.ctypes.data, fin.ctypes.data, adm.ctypes.data,
                                                          col.ctypes.data, C.byref(secs), C.byref(st), None if arr is None else C.byref(arr.req))
        elif prefix is None and logprobs is None:
            rc = lib().biogpt_hip_generate_queue(self._h, flat.ctypes.data, lens.ctypes.data, R, None if np_arr is None or R == 0 else np_arr.ctypes.data, int(n_predict),
                                                 int(max_columns), int(group), int(n_batch), int(top_k), float(top_p), float(temp), sd.ctypes.data, int(eos_id),
                                                 out.ctypes.data, ol.ctypes.data, adm.ctypes.data, col.ctypes.data, C.byref(secs), C.byref(st))
        else:
            rc = lib().biogpt_hip_generate_queue_prefix(self._h, None if pre is None else pre.ctypes.data, 0 if prefix is None else len(prefix), flat.ctypes.data,
                                                        lens.ctypes.data, R, None if np_arr is None or R == 0 else np_arr.ctypes.data, int(n_predict), int(max_columns),
                                                        int(group), int(n_batch), int(top_k), float(top_p), float(temp), sd.ctypes.data, int(eos_id), out.ctypes.data,
                                                        ol.ctypes.data, adm.ctypes.data, col.ctypes.data, C.byref(secs), C.byref(st),
                                                        None if arr is None else C.byref(arr.req))
        if rc < 0:
            raise BiogptError(_err())
        rows = out.reshape(-1)      # rows are [R][n_predict as given]
        ids = [rows[r * w:r * w + int(ol[r])].copy() for r in range(R)]
        info = {"stats": st.as_dict(), "admit_step": [int(v) for v in adm[:R]], "column": [int(v) for v in col[:R]]}
        if arr is not None:
            info["logprobs"] = arr.info(R, w, [int(v) for v in ol[:R]]) if w > 0 else [arr.info(1, 0, [0])[0] for _ in range(R)]
        if fin is not None:
            info["finish"] = [int(v) for v in fin[:R]]
        return ids, info, secs.value

    def queue_session(self, max_columns=64, group=4, n_predict=64, prefix=None, logprobs=None, stream=False, n_batch=8, max_len=0, top_k=1, top_p=0.9, temp=0.9,
                      eos_id=-1):
        """A queue session ("A serving loop"; biogpt_hip_queue_open): generate_queue(params=, prefix=, logprobs=) for requests that arrive over
        time.  A context manager with submit(prompt, n_predict=None, seed=0, params=None) -> id, poll(max_groups=1) -> [events], cancel(id), drain() and
        stats().  n_predict is the most any request may ask for; top_k / top_p / temp / eos_id the sampler of a request submitted without params; stream=True
        adds "delta" events for the tokens running requests append.  While it is open the model serves nothing else."""
        return QueueSession(self, max_columns, group, n_predict, prefix, logprobs, stream, n_batch, max_len, top_k, top_p, temp, eos_id)

    def read_column_state(self, column, pos, which=0, n_ids=0):
        """Tests of slot reuse (biogpt_hip_read_column_state): (the K (which 0) or V (1) row of position pos in every layer of column `column`'s own cache slot,
        float32 [n_layer, d_model]; the first n_ids ids of the column's beam pool row) as the last column call left them."""
        hp = self.hparams
        kv = np.zeros((hp.n_layer, hp.d_model), dtype=np.float32)
        ids = np.zeros(max(int(n_ids), 1), dtype=np.int32)
        if lib().biogpt_hip_read_column_state(self._h, int(column), int(which), int(pos), kv.ctypes.data, int(n_ids), ids.ctypes.data if n_ids else None) != 0:
            raise BiogptError(_err())
        return kv, ids[:int(n_ids)].copy()

    def generate_beam_queue(self, prompts, n_predict, n_beams=5, max_columns=510, group=4, eos_id=2, length_penalty=1.0, early_stopping=True, n_batch=8,
                            n_predicts=None, trie=None):
        """Beam search over a queue of requests (continuous batching; INTEGRATION.md, "Beam search over a queue"): prompts is a list of id lists of any
        length, max_columns // n_beams searches run at a time, and a search that stops -- by transformers' stopping rules, or after its own n_predicts[r]
        (None: n_predict) steps as clamped to ITS prompt -- hands its n_beams columns to the next request.  Request r's list is generate_beam(prompts[r],
        n_r, n_beams, eos_id, length_penalty, early_stopping, n_batch, trie=trie) alone, whatever else is in the queue.  group: steps between two looks at
        the slots; max_columns=510 is the fastest setting measured and 510 K / V caches, 96 GiB at BioGPT-base, where they are all used: 160 was
        1.26 x slower on a workload without an EOS.  The caches stay allocated to this model after the call, until close().  No generation rules, prefix= or
        logprobs=.  Returns ([[(ids int32[len], score), ...] best first, one list per request], {"stats":
        {...} counted in slots, "admit_step": [...], "slot": [...], "steps": [...]}, seconds) -- queue_plan(steps, slots, group, limits=[n_r, ...]) computes the last
        three from the first; a request without room for a token gets an empty list, -1 in
        admit_step and slot, and 0 steps."""
        if len(prompts) and np.isscalar(prompts[0]):
            prompts = [prompts]
        R, B = len(prompts), max(int(n_beams), 1)
        lens = np.asarray([len(p) for p in prompts] or [0], dtype=np.int32)
        flat = _flat_ids(prompts)
        np_arr = None
        if n_predicts is not None:
            np_arr = np.ascontiguousarray(n_predicts, dtype=np.int32).reshape(-1)
            if np_arr.size != R:
                raise BiogptError("n_predicts must have one entry per request (%d != %d)" % (np_arr.size, R))
        w = max(int(n_predict), 0)
        out = np.zeros((max(R, 1) * B, max(w, 1)), dtype=np.int32)
        ol = np.zeros(max(R, 1) * B, dtype=np.int32)
        scores = np.zeros(max(R, 1) * B, dtype=np.float32)
        counts, steps, adm, slot = (np.zeros(max(R, 1), dtype=np.int32) for _ in range(4))
        st = QueueStats()
        secs = C.c_double(0.0)
        rc = lib().biogpt_hip_generate_beam_queue(self._h, flat.ctypes.data, lens.ctypes.data, R, None if np_arr is None or R == 0 else np_arr.ctypes.data,
                                                  int(n_predict), int(n_beams), int(max_columns), int(group), int(n_batch), int(eos_id), float(length_penalty),
                                                  1 if early_stopping else 0, None if trie is None else _trie_handle(trie), out.ctypes.data, ol.ctypes.data,
                                                  scores.ctypes.data, counts.ctypes.data, steps.ctypes.data, adm.ctypes.data, slot.ctypes.data, C.byref(secs),
                                                  C.byref(st))
        if rc < 0:
            raise BiogptError(_err())
        rows = out.reshape(-1)      # rows are [R][n_beams][n_predict as given]
        hyps = [[(rows[(r * B + i) * w:(r * B + i) * w + int(ol[r * B + i])].copy(), float(scores[r * B + i])) for i in range(int(counts[r]))] for r in range(R)]
        return hyps, {"stats": st.as_dict(), "admit_step": [int(v) for v in adm[:R]], "slot": [int(v) for v in slot[:R]], "steps": [int(v) for v in steps[:R]]}, secs.value

    @_logprobs_keyword
    @_sampler_keyword
    def generate_sample(self, prompts, n_predict, n_samples=1, top_k=40, top_p=0.9, temp=0.9, seed=0, seeds=None, eos_id=-1, n_batch=8,
                        repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=(), trie=None, prefix=None):
        """n_samples sampled continuations of every prompt (list of id lists, or one flat id list), drawn on the device by the reference's top-k / top-p
        sampler ("Sampled generation").  Sequence p * n_samples + j is sample j of prompt p with std::mt19937(seeds[...]); seeds=None:
        seed + sequence index.  Returns ([ids int32[len], ...] in sequence order, seconds); an EOS that ended a sequence is included.  The last four arguments
        are transformers' logits processors of the same names, applied to the raw logits row in front of the sampler ("Generation
        rules"); top_k=1 never draws: greedy decoding with rules and an EOS.  trie: a Trie -- every row is masked to the tokens that continue an entry
        (or EOS where one ends) in front of the sampler (biogpt_hip_generate_sample_trie; needs eos_id >= 0); top_k=1: constrained greedy decoding.
        prefix: a list of ids in front of every prompt -- sequence p is prefix + prompts[p], a prompt may then be empty ([[]]: n_samples of the prefix
        alone), the ids are those of the call on the concatenations and the prefix is evaluated once ("Generation behind a shared
        prefix").  Not with rules or a trie: ValueError.
        logprobs (keyword only): None, or K in [0, 8] -- the call then returns (ids, info, seconds) with info[r] = (logprobs float32[len], top_ids int32[len, K],
        top_logprobs float32[len, K]): the model's log-probability of every generated token under the RAW row (temperature 1, no top_k / top_p cut: the
        number score_batch gives, not the probability under the truncated sampling distribution) and every row's K best entries (INTEGRATION.md,
        "Log-probabilities of generated tokens").  The ids are those of the call without it.  Not with rules or a trie: ValueError.
        sampler (keyword only): None, or a sampler(top_k, top_p, min_p, temp) of any width -- top_k 0 or up to n_vocab, with min-p -- drawn by
        sample_wide_rows_kernel ("Sampled generation"); top_k, top_p and temp must then be left at their defaults (BiogptError), everything
        else works as without it.  With top_k in [1, 64] and min_p 0 the call is the plain one with the sampler's values.  Not with logprobs, rules or a
        trie: ValueError."""
        return BiogptModel._generate_sample(self, prompts, n_predict, n_samples, top_k, top_p, temp, seed, seeds, eos_id, n_batch, repetition_penalty, no_repeat_ngram_size,
                                            min_new_tokens, suppress_tokens, trie, prefix)

    def _generate_sample(self, prompts, n_predict, n_samples=1, top_k=40, top_p=0.9, temp=0.9, seed=0, seeds=None, eos_id=-1, n_batch=8,
                         repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=(), trie=None, prefix=None, logprobs=None, sampler=None):
        """generate_sample, with logprobs=K its form that returns (ids, info, seconds), with sampler= the wide sampler's."""
        if sampler is not None:
            if logprobs is not None:
                raise ValueError("sampler= cannot be combined with logprobs=")
            if trie is not None:
                raise ValueError("sampler= cannot be combined with trie=")
            if float(repetition_penalty) != 1.0 or int(no_repeat_ngram_size) != 0 or int(min_new_tokens) != 0 or len(suppress_tokens):
                raise ValueError("sampler= cannot be combined with generation rules")
            if (top_k, top_p, temp) != (40, 0.9, 0.9):
                raise BiogptError("sampler= carries top_k, top_p and temp: leave the call's own at their defaults")
            sampler = _as_sampler(sampler)
        if logprobs is not None:
            if trie is not None:
                raise ValueError("logprobs= cannot be combined with trie=")
            if float(repetition_penalty) != 1.0 or int(no_repeat_ngram_size) != 0 or int(min_new_tokens) != 0 or len(suppress_tokens):
                raise ValueError("logprobs= cannot be combined with generation rules")
        if prefix is not None:
            if trie is not None:
                raise ValueError("prefix= cannot be combined with trie=")
            if float(repetition_penalty) != 1.0 or int(no_repeat_ngram_size) != 0 or int(min_new_tokens) != 0 or len(suppress_tokens):
                raise ValueError("prefix= cannot be combined with generation rules")
        rules, keep = gen_rules(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)
        if len(prompts) and np.isscalar(prompts[0]):
            prompts = [prompts]
        lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
        if prefix is not None:
            flat = _flat_ids(prompts)
        else:
            flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]) if len(prompts) else np.zeros(0, np.int32))
        n = len(prompts) * int(n_samples)
        if seeds is None:
            seeds = [(int(seed) + r) & 0xFFFFFFFF for r in range(max(n, 0))]
        sd = np.ascontiguousarray(seeds, dtype=np.uint32)
        if sd.size != max(n, 0):
            raise BiogptError("seeds must have one entry per sequence (%d != %d)" % (sd.size, n))
        w = max(int(n_predict), 1)
        out = np.zeros((max(n, 1), w), dtype=np.int32)
        ol = np.zeros(max(n, 1), dtype=np.int32)
        secs = C.c_double(0.0)
        if logprobs is not None:
            arr = _LogprobArrays(logprobs, n, w)
            pre = None if prefix is None else _flat_ids([prefix])
            flat = _flat_ids(prompts)
            got = lib().biogpt_hip_generate_sample_lp(self._h, None if pre is None else pre.ctypes.data, 0 if prefix is None else len(prefix), flat.ctypes.data,
                                                      lens.ctypes.data, len(prompts), int(n_samples), int(n_batch), int(n_predict), int(top_k), float(top_p), float(temp),
                                                      sd.ctypes.data, int(eos_id), out.ctypes.data, ol.ctypes.data, C.byref(secs), C.byref(arr.req))
            if got < 0:
                raise BiogptError(_err())
            if got == 0:
                return [], [], secs.value
            rows = out.reshape(-1)
            return [rows[r * got:r * got + int(ol[r])].copy() for r in range(n)], arr.info(n, got, [int(v) for v in ol[:n]]), secs.value
        if sampler is not None and prefix is not None:
            pre = _flat_ids([prefix])
            got = lib().biogpt_hip_generate_sample_wide_prefix(self._h, pre.ctypes.data, len(prefix), flat.ctypes.data, lens.ctypes.data, len(prompts), int(n_samples),
                                                               int(n_batch), int(n_predict), C.byref(sampler), sd.ctypes.data, int(eos_id), out.ctypes.data,
                                                               ol.ctypes.data, C.byref(secs))
        elif sampler is not None:
            got = lib().biogpt_hip_generate_sample_wide(self._h, flat.ctypes.data, lens.ctypes.data, len(prompts), int(n_samples), int(n_batch), int(n_predict),
                                                        C.byref(sampler), sd.ctypes.data, int(eos_id), out.ctypes.data, ol.ctypes.data, C.byref(secs))
        elif prefix is not None:
            pre = _flat_ids([prefix])
            got = lib().biogpt_hip_generate_sample_prefix(self._h, pre.ctypes.data, len(prefix), flat.ctypes.data, lens.ctypes.data, len(prompts), int(n_samples),
                                                          int(n_batch), int(n_predict), int(top_k), float(top_p), float(temp), sd.ctypes.data, int(eos_id),
                                                          out.ctypes.data, ol.ctypes.data, C.byref(secs))
        elif trie is not None:
            _no_rules_with_trie(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)
            got = lib().biogpt_hip_generate_sample_trie(self._h, flat.ctypes.data, lens.ctypes.data, len(prompts), int(n_samples), int(n_batch), int(n_predict),
                                                        int(top_k), float(top_p), float(temp), sd.ctypes.data, int(eos_id), _trie_handle(trie), out.ctypes.data,
                                                        ol.ctypes.data, C.byref(secs))
        else:
            got = lib().biogpt_hip_generate_sample_rules(self._h, flat.ctypes.data, lens.ctypes.data, len(prompts), int(n_samples), int(n_batch), int(n_predict),
                                                         int(top_k), float(top_p), float(temp), sd.ctypes.data, int(eos_id), out.ctypes.data, ol.ctypes.data,
                                                         C.byref(secs), C.byref(rules))
        if got < 0:
            raise BiogptError(_err())
        if got == 0:
            return [], secs.value
        rows = out.reshape(-1)      # rows are [n][n_predict as clamped]
        return [rows[r * got:r * got + int(ol[r])].copy() for r in range(n)], secs.value

    # -- sequence scoring (no reference counterpart): teacher-forced causal log-probabilities --
    def score(self, tokens, n_past=0, targets=None):
        """Row i sees tokens[0..i] (after n_past cached positions).  Returns (logprobs float32[n], argmax int32[n], target_logits float32[n]):
        log P(targets[i] | ...) (natural log; targets=None: the next token, the last row unscored), each row's arg-max, and the target's
        logit.  Rows with a negative target get 0 in logprobs and target_logits."""
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32)
        if tg is not None and tg.size != toks.size:
            raise BiogptError("targets must have one entry per token (%d != %d)" % (tg.size, toks.size))
        lp = np.zeros(toks.size, dtype=np.float32)
        am = np.zeros(toks.size, dtype=np.int32)
        lg = np.zeros(toks.size, dtype=np.float32)
        if lib().biogpt_hip_score(self._h, toks.ctypes.data, toks.size, int(n_past), None if tg is None else tg.ctypes.data,
                                  lp.ctypes.data, am.ctypes.data, lg.ctypes.data) != 0:
            raise BiogptError(_err())
        return lp, am, lg

    def score_batch(self, seqs, targets=None):
        """score() of several independent sequences (each from position 0, in its own K / V cache) in common passes.  targets: None, or one
        entry per sequence -- None (next-token scoring) or that sequence's targets.  Returns a list of (logprobs, argmax, target_logits)."""
        lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]) if len(seqs) else np.zeros(0, np.int32))
        tg = None
        if targets is not None:
            if len(targets) != len(seqs):
                raise BiogptError("targets must have one entry per sequence")
            parts = []
            for s, t in zip(seqs, targets):
                if t is None:
                    t = list(s[1:]) + [-1]
                if len(t) != len(s):
                    raise BiogptError("targets must have one entry per token")
                parts.append(np.asarray(t, dtype=np.int32))
            tg = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, np.int32))
        n = max(int(flat.size), 1)
        lp, am, lg = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        if lib().biogpt_hip_score_batch(self._h, flat.ctypes.data, lens.ctypes.data, len(seqs), None if tg is None else tg.ctypes.data,
                                        lp.ctypes.data, am.ctypes.data, lg.ctypes.data) != 0:
            raise BiogptError(_err())
        out, off = [], 0
        for k in lens:
            out.append((lp[off:off + k].copy(), am[off:off + k].copy(), lg[off:off + k].copy()))
            off += int(k)
        return out

    def score_continuations(self, prefix, continuations):
        """Many continuations of ONE prefix (lists of ids): the prefix is evaluated once and read in place by every continuation.  Returns one
        (logprobs, argmax, logits) triple per continuation, each array of the continuation's length: entry i is log P(cont[i] | prefix,
        cont[:i]), the arg-max of that row and cont[i]'s logit -- rows len(prefix) - 1 + i of score(prefix + cont), bit for bit."""
        pre = np.ascontiguousarray(prefix, dtype=np.int32).reshape(-1)
        lens = np.asarray([len(c) for c in continuations], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.int32).reshape(-1) for c in continuations])
                                    if len(continuations) else np.zeros(0, np.int32))
        n = max(int(flat.size), 1)
        lp, am, lg = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        secs = C.c_double(0.0)
        if lib().biogpt_hip_score_continuations(self._h, pre.ctypes.data, int(pre.size), flat.ctypes.data, lens.ctypes.data, len(continuations),
                                                lp.ctypes.data, am.ctypes.data, lg.ctypes.data, C.byref(secs)) != 0:
            raise BiogptError(_err())
        self.score_seconds = secs.value
        out, off = [], 0
        for k in lens:
            out.append((lp[off:off + k].copy(), am[off:off + k].copy(), lg[off:off + k].copy()))
            off += int(k)
        return out

    def rank_continuations(self, prefix, continuations, normalize=False):
        """(order, sums): the indices of `continuations` from the most to the least likely after `prefix`, and every continuation's summed
        log-probability (float64 sums on the host; normalize: divided by the continuation's length).  Ties keep the order given."""
        rows = self.score_continuations(prefix, continuations)
        sums = np.asarray([lp.astype(np.float64).sum() / (len(lp) if normalize else 1) for lp, _, _ in rows], dtype=np.float64)
        return np.argsort(-sums, kind="stable"), sums

    def score_continuations_batch(self, prefixes, continuations):
        """score_continuations for a dataset: prefixes a list of id lists, continuations a list (one entry per prefix) of lists of id lists.  Returns one list
        per group of (logprobs, argmax, logits) triples, as score_continuations(prefixes[g], continuations[g]) does.  The groups travel through common passes
        (biogpt_hip_score_continuations_batch); a dataset that needs more than 512 slots (one per prefix, one per continuation) is cut into several calls,
        greedily and in order (prefix_batch_chunks).  BIOGPT_HIP_RUN_ATTN=0: bit for bit the per-group calls; see include/biogpt_hip.h for the other settings."""
        if len(prefixes) != len(continuations):
            raise BiogptError("continuations must have one entry per prefix (%d != %d)" % (len(continuations), len(prefixes)))
        out, secs_all, self.prefix_batch_calls = [], 0.0, 0
        for g0, g1 in prefix_batch_chunks([len(c) for c in continuations]):
            pres = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in prefixes[g0:g1]]
            flat_p = np.ascontiguousarray(np.concatenate(pres)) if sum(p.size for p in pres) else np.zeros(1, np.int32)
            plens = np.asarray([p.size for p in pres], dtype=np.int32)
            ncs = np.asarray([len(c) for c in continuations[g0:g1]], dtype=np.int32)
            cs = [np.asarray(c, dtype=np.int32).reshape(-1) for grp in continuations[g0:g1] for c in grp]
            clens = np.asarray([c.size for c in cs] or [0], dtype=np.int32)
            flat_c = np.ascontiguousarray(np.concatenate(cs)) if sum(c.size for c in cs) else np.zeros(1, np.int32)
            n = max(int(clens.sum()), 1)
            lp, am, lg = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
            secs = C.c_double(0.0)
            if lib().biogpt_hip_score_continuations_batch(self._h, flat_p.ctypes.data, plens.ctypes.data, g1 - g0, flat_c.ctypes.data, clens.ctypes.data,
                                                          ncs.ctypes.data, lp.ctypes.data, am.ctypes.data, lg.ctypes.data, C.byref(secs)) != 0:
                raise BiogptError(_err())
            secs_all += secs.value
            self.prefix_batch_calls += 1
            off, at = 0, 0
            for nc in ncs:
                rows = []
                for k in clens[at:at + nc]:
                    rows.append((lp[off:off + k].copy(), am[off:off + k].copy(), lg[off:off + k].copy()))
                    off += int(k)
                at += int(nc)
                out.append(rows)
        self.score_seconds = secs_all
        return out

    def rank_continuations_batch(self, prefixes, continuations, normalize=False):
        """rank_continuations for a dataset: a list of (order, sums) per group -- float64 sums on the host, ties keep the order given."""
        res = []
        for rows in self.score_continuations_batch(prefixes, continuations):
            sums = np.asarray([lp.astype(np.float64).sum() / (len(lp) if normalize else 1) for lp, _, _ in rows], dtype=np.float64)
            res.append((np.argsort(-sums, kind="stable"), sums))
        return res

    def prefix_batch_stats(self):
        """Of the last successful biogpt_hip_score_continuations_batch call on this model: prefix_columns, continuation_columns, passes, run_passes (the
        passes whose attention ran on attn_runs_kernel)."""
        out = np.zeros(4, dtype=np.int32)
        if lib().biogpt_hip_prefix_batch_stats(self._h, out.ctypes.data) != 0:
            raise BiogptError(_err())
        return dict(prefix_columns=int(out[0]), continuation_columns=int(out[1]), passes=int(out[2]), run_passes=int(out[3]))

    # -- hidden states, pooled embeddings, classification heads (no reference counterpart) --
    def hidden(self, tokens, n_past=0):
        """The final hidden state (after the last LayerNorm) of every token, float32 [n, d_model]; row i sees tokens[0..i] (after n_past
        cached positions).  Leaves the K / V rows of eval_prompt(tokens, n_past, 1); the context's logits row is undefined afterwards."""
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.zeros((toks.size, self.hparams.d_model), dtype=np.float32)
        if lib().biogpt_hip_hidden(self._h, toks.ctypes.data, toks.size, int(n_past), out.ctypes.data) != 0:
            raise BiogptError(_err())
        return out

    def embed_batch(self, seqs, layer=-1, pooling="last", normalize=False, head=None):
        """Embeddings of several independent sequences (list of id lists, each from position 0 in its own K / V cache) in common causal passes.
        layer: transformers' hidden_states index (0 embeddings ... n_layer = -1 after the final LayerNorm); pooling "last" / "mean": one row per
        sequence, float32 [n_seqs, width]; "none": a list of per-sequence arrays [len, width].  normalize: L2-normalised rows.  head: W
        [n_out, d_model] or (W, b), applied on the device to the pooled rows (or to every token's row): width = n_out, else d_model."""
        o, keep = embed_opts(layer, pooling, normalize, head)
        if keep[0] is not None and keep[0].shape[1] != self.hparams.d_model:
            raise BiogptError("head: W must have d_model = %d columns (got %d)" % (self.hparams.d_model, keep[0].shape[1]))
        lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]) if len(seqs) else np.zeros(0, np.int32))
        width = int(o.n_out) if o.n_out > 0 else self.hparams.d_model
        rows = len(seqs) if o.pooling else int(flat.size)
        out = np.zeros((max(rows, 1), max(width, 1)), dtype=np.float32)
        secs = C.c_double(0.0)
        if lib().biogpt_hip_embed_batch(self._h, flat.ctypes.data, lens.ctypes.data, len(seqs), C.byref(o), out.ctypes.data, C.byref(secs)) != 0:
            raise BiogptError(_err())
        self.embed_seconds = secs.value
        if o.pooling:
            return out[:rows]
        res, off = [], 0
        for k in lens:
            res.append(out[off:off + k].copy())
            off += int(k)
        return res

    def read_kv(self, which, offset, count):
        out = np.empty(int(count), dtype=np.float32)
        if lib().biogpt_hip_read_kv(self._h, int(which), int(offset), int(count), out.ctypes.data) != 0:
            raise BiogptError(_err())
        return out

    def debug_stamps(self, offset, count):
        """Profiling builds: `count` raw stage stamps (100 MHz ticks) from word `offset` of the context's stamp buffer."""
        out = (C.c_ulonglong * count)()
        if lib().biogpt_hip_debug_stamps(self._h, offset, count, out) != 0:
            raise BiogptError(_err())
        return np.frombuffer(out, dtype=np.uint64).copy()

    def bench_matvec(self, which, layer=0, reps=200):
        secs, nbytes = C.c_double(0.0), C.c_double(0.0)
        if lib().biogpt_hip_bench_matvec(self._h, int(which), int(layer), int(reps), C.byref(secs), C.byref(nbytes)) != 0:
            raise BiogptError(_err())
        return secs.value, nbytes.value

    def bench_stream(self, rows=1 << 19, reps=20, steps=8):
        secs, nbytes = C.c_double(0.0), C.c_double(0.0)
        if lib().biogpt_hip_bench_stream(self._h, int(rows), int(reps), int(steps), C.byref(secs), C.byref(nbytes)) != 0:
            raise BiogptError(_err())
        return secs.value, nbytes.value

    def bench_api_loop(self, prompt, n_predict, mode):
        """The reference's greedy host loop in C++ on this library (mode 0: full logits row per token, 1: device top-40)."""
        pr = np.ascontiguousarray(prompt, dtype=np.int32)
        out = np.zeros(int(n_predict), dtype=np.int32)
        secs = C.c_double(0.0)
        got = lib().biogpt_hip_bench_api_loop(self._h, pr.ctypes.data, pr.size, int(n_predict), int(mode), out.ctypes.data, C.byref(secs))
        if got < 0:
            raise BiogptError(_err())
        return out[:got], secs.value

    def generate_launches(self):
        """Tokens of each multi-token pipelined launch of the last generate_greedy call (biogpt_hip_generate_launches)."""
        buf = (C.c_int32 * 16)()
        n = int(lib().biogpt_hip_generate_launches(self._h, buf, 16))
        return [int(buf[i]) for i in range(max(0, min(n, 16)))]

    def fpipe_launches(self):
        """Single-token steps through the float-weight persistent launch (biogpt_hip_fpipe_launches); -1: not available to this context."""
        return int(lib().biogpt_hip_fpipe_launches(self._h))

    def fpipe_stamps(self):
        """Stage-border times of the last float-weight persistent launch (BIOGPT_HIP_FPIPE_STAMPS=1): numpy uint64 [3 workgroups][32 layers][32], 10 ns units; None when inactive."""
        import numpy as np
        buf = (C.c_uint64 * 3072)()
        n = int(lib().biogpt_hip_fpipe_stamps(self._h, buf, 3072))
        return None if n != 3072 else np.frombuffer(buf, dtype=np.uint64).reshape(3, 32, 32).copy()

    def mfma_launches(self):
        """Launches of the many-column chain that went to the matrix-core kernels (biogpt_hip_mfma_launches)."""
        return int(lib().biogpt_hip_mfma_launches(self._h))

    def chain_kind(self):
        """Which many-column layer chain the file has (biogpt_hip_chain_kind): 0 none, 1 the BioGPT-base chain, 2 the wide chain (any other block-quantized file
        with head size 64, d_model a multiple of 64 and d_ff of 32), 3 the float chain (an F32 / F16 file of those widths while float_chain() is on), 4 the SIMD chain (a context in
        the "simd" association while assoc_chain is on; such a context is 0 otherwise)."""
        k = int(lib().biogpt_hip_chain_kind(self._h))
        if k < 0:
            raise BiogptError(_err())
        return k

    def float_chain(self, on=True):
        """The float chain's switch (biogpt_hip_float_chain): on, the batched calls the wide chain serves serve this F32 / F16 file, chain_kind() is 3; off (the
        default of a load), the file has the single-sequence calls only.  Raises BiogptError with the reason where the file cannot have it."""
        if lib().biogpt_hip_float_chain(self._h, 1 if on else 0) != 0:
            raise BiogptError(_err())

    def set_assoc(self, mode):
        """The association's switch (biogpt_hip_assoc): "scalar" (ggml's scalar summation order, the default) or "simd" (the order of an AVX2 build of the
        reference: the oracle's assoc = 3).  In "simd" the context serves the single-sequence calls on five launches per layer and refuses the calls over
        column states.  Raises BiogptError with the reason where the file cannot have the mode (an F32 / F16 file, a head size other than 64)."""
        if mode not in ASSOC_MODES:
            raise ValueError("assoc must be 'scalar' or 'simd' (got %r)" % (mode,))
        if lib().biogpt_hip_assoc(self._h, ASSOC_MODES[mode]) != 0:
            raise BiogptError(_err())

    @property
    def assoc(self):
        """The context's association: "scalar" or "simd" (biogpt_hip_get_assoc)."""
        k = int(lib().biogpt_hip_get_assoc(self._h))
        if k < 0:
            raise BiogptError(_err())
        return "simd" if k == 1 else "scalar"

    def set_assoc_chain(self, on=True):
        """The SIMD chain's switch (biogpt_hip_assoc_chain): on, a context in the "simd" association serves the batched calls the wide chain serves (score_batch,
        embed_batch, score_continuations, generate_greedy_batch, generate_sample, generate_beam(_batch), the plain generate_queue) in that association, and
        chain_kind() is 4; in the "scalar" association the switch changes nothing.  Raises BiogptError with the reason where the file cannot have it."""
        if lib().biogpt_hip_assoc_chain(self._h, 1 if on else 0) != 0:
            raise BiogptError(_err())

    @property
    def assoc_chain(self):
        """Whether the SIMD chain's switch is on (biogpt_hip_get_assoc_chain)."""
        k = int(lib().biogpt_hip_get_assoc_chain(self._h))
        if k < 0:
            raise BiogptError(_err())
        return k == 1

    def simd_chain_launches(self):
        """Linear-stage launches of the SIMD chain (biogpt_hip_simd_chain_launches); 0 while the switch is off."""
        return int(lib().biogpt_hip_simd_chain_launches(self._h))

    def float_launches(self):
        """Linear-stage launches of the float chain (biogpt_hip_float_launches); 0 while the switch is off."""
        return int(lib().biogpt_hip_float_launches(self._h))

    def wide_launches(self):
        """Linear-stage launches of the wide chain (biogpt_hip_wide_launches); 0 on a BioGPT-base file."""
        return int(lib().biogpt_hip_wide_launches(self._h))

    def chunk_launches(self):
        """Evals of 2 .. 8 tokens that went through the column-per-XCD launch (biogpt_hip_chunk_launches)."""
        return int(lib().biogpt_hip_chunk_launches(self._h))

    def xpipe_state(self):
        """1: single-token decode steps of this context run as the XCD-pipelined persistent launch; 0: off / path held by
        another context of the device; -1: unavailable or abandoned after a disturbed launch."""
        return int(lib().biogpt_hip_xpipe_state(self._h))

    def refresh_options(self):
        """Re-read the BIOGPT_HIP_* switches (they are cached at load time) and drop the captured graphs."""
        if lib().biogpt_hip_refresh_options(self._h) != 0:
            raise BiogptError(_err())

    def bench_sweep(self, reps=20, which=0):
        """(seconds per launch, algorithmic bytes per launch, max |device - host| over sampled rows) of the all-matrices mat-vec launch (biogpt_hip_bench_sweep)."""
        secs, nbytes, chk = C.c_double(0.0), C.c_double(0.0), C.c_double(-1.0)
        if lib().biogpt_hip_bench_sweep(self._h, int(which), int(reps), C.byref(secs), C.byref(nbytes), C.byref(chk)) != 0:
            raise BiogptError(_err())
        return secs.value, nbytes.value, chk.value

    def bench_sweep_rows(self, which=0, reps=4):
        """The sweep launch's output rows and the two Q8 activation vectors they were computed with (biogpt_hip_bench_sweep_ex): (rows float32 [sum of the selected
        matrices' rows], xq int8 [1024 + 4096], xd float32 [32 + 128])."""
        hp = self.hparams
        per_layer = {0: 3 * hp.d_model + hp.d_model + hp.d_ff + hp.d_model, 2: 4 * hp.d_model, 3: hp.d_model, 4: hp.d_ff, 1: 0}[int(which)]
        n = per_layer * hp.n_layer + (hp.n_vocab if which in (0, 1) else 0)
        rows = np.zeros(n, np.float32); xq = np.zeros(1024 + 4096, np.int8); xd = np.zeros(32 + 128, np.float32)
        secs, nbytes, chk = C.c_double(0.0), C.c_double(0.0), C.c_double(-1.0)
        if lib().biogpt_hip_bench_sweep_ex(self._h, int(which), int(reps), C.byref(secs), C.byref(nbytes), C.byref(chk), rows.ctypes.data_as(C.POINTER(C.c_float)), n,
                                           xq.ctypes.data_as(C.POINTER(C.c_int8)), xd.ctypes.data_as(C.POINTER(C.c_float))) != 0:
            raise BiogptError(_err())
        return rows, xq, xd

    def bench_decode(self, n_past, reps=50):
        secs = C.c_double(0.0)
        if lib().biogpt_hip_bench_decode(self._h, int(n_past), int(reps), C.byref(secs)) != 0:
            raise BiogptError(_err())
        return secs.value

    def vocab_token(self, i):
        p, n = C.c_char_p(), C.c_int32()
        if lib().biogpt_hip_vocab_token(self._h, int(i), C.byref(p), C.byref(n)) != 0:
            raise IndexError(i)
        return C.string_at(p, n.value)

    @property
    def vocab(self):
        """The context's vocabulary handle (borrowed: valid until close()); None for an attached context."""
        h = lib().biogpt_hip_ctx_vocab(self._h)
        return Vocab(h, False) if h else None

    @property
    def arena(self):
        return lib().biogpt_hip_arena_ptr(self._h), int(lib().biogpt_hip_arena_bytes(self._h))

    def close(self):
        if self._h:
            lib().biogpt_hip_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Replicas:
    """biogpt_hip_replicas_*: one process, one context per device, weights loaded once and RCCL-broadcast."""

    def __init__(self, fname, devices, verbosity=0):
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        self._h = lib().biogpt_hip_replicas_load(_bytes(fname), devs.ctypes.data, int(devs.size), int(verbosity))
        if not self._h:
            raise BiogptError(_err())

    @property
    def count(self):
        return lib().biogpt_hip_replicas_count(self._h)

    @property
    def broadcast_seconds(self):
        return lib().biogpt_hip_replicas_broadcast_seconds(self._h)

    def vocab_of(self, i):
        """The tokenizer handle of replica i (attached replicas share the root's tables)."""
        ctx = lib().biogpt_hip_replicas_ctx(self._h, int(i))
        h = lib().biogpt_hip_ctx_vocab(ctx)
        return Vocab(h, False) if h else None

    def generate_greedy(self, prompts, n_predict, n_batch=8):
        flat = np.ascontiguousarray([t for p in prompts for t in p], dtype=np.int32)
        lens = np.ascontiguousarray([len(p) for p in prompts], dtype=np.int32)
        out = np.zeros((len(prompts), int(n_predict)), dtype=np.int32)
        counts = np.zeros(len(prompts), dtype=np.int32)
        secs = C.c_double(0.0)
        rc = lib().biogpt_hip_replicas_generate_greedy(self._h, flat.ctypes.data, lens.ctypes.data, len(prompts), int(n_batch), int(n_predict),
                                                       out.ctypes.data, counts.ctypes.data, C.byref(secs))
        if rc < 0:
            raise BiogptError(_err())
        return [out[g, :counts[g]].copy() for g in range(len(prompts))], secs.value

    def close(self):
        if self._h:
            lib().biogpt_hip_replicas_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_bytes_per_token(hp, T):
    """Algorithmic HBM bytes of one decoded token at context T:
    W(type) + 2*L*T*D*4 (KV read) + 2*L*D*4 (KV write) + V*4 (logits)."""
    D, F, V, L = hp.d_model, hp.d_ff, hp.n_vocab, hp.n_layer
    bb = FILE_BLOCK_BYTES[hp.ftype] / 32.0
    mats = L * (4 * D * D + 2 * D * F) * bb + V * D * bb
    vecs = (L * (4 * D + 4 * D + F + D) + 2 * D) * 4
    rows = 2 * D * bb
    return mats + vecs + rows + 2 * L * T * D * 4 + 2 * L * D * 4 + V * 4
