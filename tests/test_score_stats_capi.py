"""Scoring statistics and the comparison of two files (biogpt_hip_score_stats, biogpt_hip_score_batch_stats, biogpt_hip_score_compare,
biogpt_hip_score_stats_device) without a GPU: the C-ABI is declared, exported and bound, the structs' fields are in the documented order, and the
argument checks come before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest

HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "biogpt_hip.h")).read()
TOKS, LENS = np.array([2, 5, 7], dtype=np.int32), np.array([3], dtype=np.int32)
F, I = np.zeros(64, dtype=np.float32), np.zeros(64, dtype=np.int32)


def test_symbols_declared_exported_and_bound(pkg):
    bound, raw = {name for name, _, _ in pkg.SYMBOLS}, ctypes.CDLL(pkg.LIB_PATH)
    for name in ("biogpt_hip_score_stats", "biogpt_hip_score_batch_stats", "biogpt_hip_score_compare", "biogpt_hip_score_stats_device"):
        assert re.search(r"\bint %s\s*\(" % name, HDR) and name in bound and getattr(raw, name) is not None, name
        assert getattr(pkg.lib(), name).restype is ctypes.c_int


@pytest.mark.parametrize("tag, cls, fields", [
    ("biogpt_hip_score_stats", "ScoreStats", ["n_top", "rank", "entropy", "top_ids", "top_lp"]),
    ("biogpt_hip_score_cmp", "ScoreCmp", ["kl_pq", "kl_qp", "lp_p", "lp_q", "argmax_p", "argmax_q"]),
])
def test_struct_fields_in_order(pkg, tag, cls, fields):
    body = re.search(r"struct %s \{(.*?)\}" % tag, HDR, flags=re.S).group(1)
    assert re.findall(r"\*?(\w+);", body) == fields and [f[0] for f in getattr(pkg, cls)._fields_] == fields


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("n_top, top_ids, top_lp, message", [
    (None, 1, 1, "stats"), (-1, 1, 1, "stats.n_top"), (9, 1, 1, "stats.n_top"), (3, 0, 1, "stats.top_ids"), (3, 1, 0, "stats.top_lp"),
    (8, 1, 1, "null context"), (0, 0, 0, "null context"),
])
def test_stats_argument_errors_come_first(pkg, batch, n_top, top_ids, top_lp, message):
    st = None if n_top is None else ctypes.byref(pkg.ScoreStats(n_top, I.ctypes.data, F.ctypes.data, top_ids and I.ctypes.data, top_lp and F.ctypes.data))
    if batch:
        rc = pkg.lib().biogpt_hip_score_batch_stats(None, TOKS.ctypes.data, LENS.ctypes.data, 1, None, F.ctypes.data, None, None, st)
    else:
        rc = pkg.lib().biogpt_hip_score_stats(None, TOKS.ctypes.data, 3, 0, None, F.ctypes.data, None, None, st)
    assert rc == -1 and message in pkg._err(), pkg._err()


def test_compare_argument_errors_come_first(pkg):
    full = ctypes.byref(pkg.ScoreCmp(F.ctypes.data, F.ctypes.data, F.ctypes.data, F.ctypes.data, I.ctypes.data, I.ctypes.data))
    same = F.ctypes.data      # never read: two equal context pointers are refused by comparing them
    for ctx_p, ctx_q, out, message in [(None, None, None, "out"), (None, None, ctypes.byref(pkg.ScoreCmp()), "out.kl_pq"), (None, same, full, "null context: ctx_p"),
                                       (same, None, full, "null context: ctx_q"), (same, same, full, "same context")]:
        assert pkg.lib().biogpt_hip_score_compare(ctx_p, ctx_q, TOKS.ctypes.data, 3, 0, None, out) == -1
        assert message in pkg._err(), (message, pkg._err())
