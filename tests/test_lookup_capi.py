"""Prompt-lookup decoding (biogpt_hip_generate_lookup, biogpt_hip_lookup_draft_device, biogpt_hip_lookup_accept_device) without a GPU: the C-ABI is
exported and bound with the declared signature, and every argument error returns -1 and names its field before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = ctypes.c_void_p
NAMES = ("biogpt_hip_generate_lookup", "biogpt_hip_lookup_draft_device", "biogpt_hip_lookup_accept_device")


def test_lookup_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name: (res, args) for name, res, args in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert name in bound
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    i32 = ctypes.c_int32
    assert bound["biogpt_hip_generate_lookup"][1] == [_P, _P, _P, i32, _P, _P, i32, i32, i32, i32, i32, _P, _P, _P, ctypes.POINTER(ctypes.c_double)]
    decl = re.search(r"int biogpt_hip_generate_lookup\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "prompts", "prompt_lens", "n_prompts", "corpus", "corpus_lens", "n_batch", "n_predict",
                                                                     "max_draft", "max_ngram", "eos_id", "out_ids", "out_lens", "out_stats", "seconds_out"]
    for name, n_args in (("biogpt_hip_lookup_draft_device", 13), ("biogpt_hip_lookup_accept_device", 16)):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == n_args == len(bound[name][1])
    assert hasattr(pkg.BiogptModel, "generate_lookup") and callable(pkg.lookup_draft) and callable(pkg.lookup_accept)


def call(pkg, ctx=None, prompts=True, lens=True, n_prompts=2, corpus=False, corpus_lens=False, clens=(2, 1), n_batch=8, n_predict=8, max_draft=7, max_ngram=3,
         eos_id=-1, ids=True, ol=True):
    pr = np.array([2, 5, 7, 2, 9], dtype=np.int32)
    ln = np.array([3, 2], dtype=np.int32)
    co = np.array([4, 5, 6], dtype=np.int32)
    cl = np.zeros(max(n_prompts, 2), dtype=np.int32)
    cl[:2] = clens
    out = np.zeros((max(n_prompts, 1), 8), dtype=np.int32)
    lens_out = np.zeros(max(n_prompts, 1), dtype=np.int32)
    secs = ctypes.c_double(0.0)
    rc = pkg.lib().biogpt_hip_generate_lookup(ctx, pr.ctypes.data if prompts else None, ln.ctypes.data if lens else None, n_prompts,
                                              co.ctypes.data if corpus else None, cl.ctypes.data if corpus_lens else None, n_batch, n_predict, max_draft,
                                              max_ngram, eos_id, out.ctypes.data if ids else None, lens_out.ctypes.data if ol else None, None, ctypes.byref(secs))
    return rc, pkg._err()


@pytest.mark.parametrize("kw, field", [
    (dict(), "null context"),
    (dict(corpus=True, corpus_lens=True), "null context"),
    (dict(prompts=False), "prompts"), (dict(lens=False), "prompt_lens"), (dict(ids=False), "out_ids"), (dict(ol=False), "out_lens"),
    (dict(corpus=True), "corpus and corpus_lens"), (dict(corpus_lens=True), "corpus and corpus_lens"),
    (dict(n_prompts=0), "n_prompts"), (dict(n_prompts=-3), "n_prompts"),
    (dict(max_draft=-1), "max_draft must be in [0, 15]"), (dict(max_draft=16), "max_draft must be in [0, 15]"),
    (dict(max_ngram=0), "max_ngram must be in [1, 8]"), (dict(max_ngram=9), "max_ngram must be in [1, 8]"),
    (dict(n_prompts=65, max_draft=7), "n_prompts x (1 + max_draft)"), (dict(n_prompts=513, max_draft=0), "n_prompts x (1 + max_draft)"),
    (dict(n_batch=0), "n_batch"),
    (dict(eos_id=-2), "eos_id"),
    (dict(corpus=True, corpus_lens=True, clens=(2, -1)), "corpus_lens[1]"),
])
def test_lookup_argument_errors_come_before_any_device_call(pkg, kw, field):
    """No device on this machine: a call that reached HIP would return -2, not -1."""
    rc, msg = call(pkg, **kw)
    assert rc == -1, (rc, msg)
    assert field in msg, msg


def draft_call(pkg, texts=True, n_seqs=2, tl=(3, 2), ng=(1, 0), npast=(2, 1), n_predict=8, max_draft=7, max_ngram=3, outs=True):
    tx = np.array([2, 5, 7, 2, 9], dtype=np.int32)
    a = [np.zeros(max(n_seqs, 2), np.int32) for _ in range(3)]
    a[0][:2], a[1][:2], a[2][:2] = tl, ng, npast
    dr, d, cols = np.zeros((max(n_seqs, 1), 16), np.int32), np.zeros(max(n_seqs, 1), np.int32), np.zeros((max(n_seqs, 1), 16, 4), np.int32)
    rc = pkg.lib().biogpt_hip_lookup_draft_device(0, tx.ctypes.data if texts else None, a[0].ctypes.data, n_seqs, a[1].ctypes.data, a[2].ctypes.data, None, n_predict,
                                                  max_draft, max_ngram, dr.ctypes.data, d.ctypes.data if outs else None, cols.ctypes.data)
    return rc, pkg._err()


@pytest.mark.parametrize("kw, field", [
    (dict(texts=False), "NULL"), (dict(outs=False), "NULL"), (dict(n_seqs=0), "n_seqs"),
    (dict(max_draft=16), "max_draft"), (dict(max_ngram=0), "max_ngram"), (dict(n_seqs=513, max_draft=0), "n_prompts x (1 + max_draft)"),
    (dict(n_predict=0), "n_predict"), (dict(tl=(3, 0)), "text_lens[1]"), (dict(ng=(3, 0)), "n_gen[0]"), (dict(npast=(2, -1)), "n_past[1]"),
])
def test_draft_entry_argument_errors(pkg, kw, field):
    rc, msg = draft_call(pkg, **kw)
    assert rc == -1 and field in msg, (rc, msg)


def accept_call(pkg, rows=True, n_seqs=2, n_vocab=8, max_draft=1, d=(1, 0), ng=(0, 0), npast=(2, 1), n_predict=8, eos_id=-1, outs=True):
    lg = np.zeros((max(n_seqs, 1) * 16, 8), dtype=np.float32)
    a = [np.zeros(max(n_seqs, 2), np.int32) for _ in range(3)]
    a[0][:2], a[1][:2], a[2][:2] = d, ng, npast
    dr = np.zeros((max(n_seqs, 1), 16), np.int32)
    o = [np.zeros((max(n_seqs, 1), 16), np.int32) for _ in range(4)]
    rc = pkg.lib().biogpt_hip_lookup_accept_device(0, lg.ctypes.data if rows else None, n_seqs, n_vocab, max_draft, dr.ctypes.data, a[0].ctypes.data, a[1].ctypes.data,
                                                   a[2].ctypes.data, None, n_predict, eos_id, o[0].ctypes.data, o[1].ctypes.data, o[2].ctypes.data,
                                                   o[3].ctypes.data if outs else None)
    return rc, pkg._err()


@pytest.mark.parametrize("kw, field", [
    (dict(rows=False), "rows is NULL"), (dict(outs=False), "NULL"), (dict(n_seqs=0), "n_seqs"), (dict(max_draft=16), "max_draft"),
    (dict(n_seqs=257, max_draft=1), "n_prompts x (1 + max_draft)"), (dict(n_vocab=0), "n_vocab"), (dict(n_predict=0), "n_predict"),
    (dict(eos_id=8), "eos_id"), (dict(d=(2, 0)), "d[0]"), (dict(ng=(0, 9)), "n_gen[1]"), (dict(npast=(-1, 0)), "n_past[0]"),
])
def test_accept_entry_argument_errors(pkg, kw, field):
    rc, msg = accept_call(pkg, **kw)
    assert rc == -1 and field in msg, (rc, msg)
