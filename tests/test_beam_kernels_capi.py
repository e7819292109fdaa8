"""The kernel-alone entries of the scoring and beam-step kernels (biogpt_hip_logprob_rows_device, biogpt_hip_beam_rows_device,
biogpt_hip_beam_table_device) without a GPU: the C-ABI is exported and bound, argument errors come before any HIP call and name the argument; the
fixtures of test_gpu_beam_kernels.py do test what they are there for (ties, EOS, early stops, evictions, forks); and the two references that
module uses agree with each other."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import beam_kernels_ref as bk
import beam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("biogpt_hip_logprob_rows_device", "biogpt_hip_beam_rows_device", "biogpt_hip_beam_table_device")


def test_symbols_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    bound = {name for name, _, _ in pkg.SYMBOLS}
    raw = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in bound, name
        assert getattr(raw, name) is not None
        assert getattr(pkg.lib(), name).restype is ctypes.c_int
    for fn in ("logprob_rows", "beam_rows", "beam_table"):
        assert hasattr(pkg, fn)


# ---- argument errors: -1 and a message naming the argument, with no device on this machine (a call that reached HIP would return -2) ----

def call_logprob(pkg, rows=True, targets=True, out=True, n_rows=2, n_vocab=8, tgt=(1, -1)):
    a = np.zeros((2, 8), dtype=np.float32)
    t = np.array(tgt, dtype=np.int32)
    o = np.zeros(2, dtype=np.float32)
    return pkg.lib().biogpt_hip_logprob_rows_device(0, a.ctypes.data if rows else None, n_rows, n_vocab, t.ctypes.data if targets else None,
                                                    o.ctypes.data if out else None, o.ctypes.data, o.ctypes.data)


@pytest.mark.parametrize("kw,word", [(dict(rows=False), "rows"), (dict(targets=False), "targets"), (dict(out=False), "lp_out"), (dict(n_rows=0), "n_rows"),
                                     (dict(n_rows=4097), "n_rows"), (dict(n_vocab=0), "n_vocab"), (dict(tgt=(1, 8)), "targets"), (dict(tgt=(-2, 0)), "targets")])
def test_logprob_rows_argument_errors(pkg, kw, word):
    assert call_logprob(pkg, **kw) == -1
    assert word in pkg._err(), pkg._err()


def call_beam_rows(pkg, rows=True, run_score=True, out=True, n_rows=4, n_vocab=40, given=0, n_beams=2, first_step=0, fill=0.0):
    a = np.full((4, 40), fill, dtype=np.float32)
    rs = np.zeros(4, dtype=np.float32)
    o = np.zeros(4 * 32, dtype=np.float32)
    return pkg.lib().biogpt_hip_beam_rows_device(0, a.ctypes.data if rows else None, n_rows, n_vocab, given, n_beams, rs.ctypes.data if run_score else None,
                                                 first_step, o.ctypes.data if out else None, o.ctypes.data, o.ctypes.data)


@pytest.mark.parametrize("kw,word", [(dict(rows=False), "rows"), (dict(run_score=False), "run_score"), (dict(out=False), "cand_score"),
                                     (dict(n_beams=0), "n_beams"), (dict(n_beams=17), "n_beams"), (dict(n_beams=3), "n_rows"), (dict(n_rows=0), "n_rows"),
                                     (dict(n_beams=4, n_vocab=7), "n_vocab"), (dict(given=2), "given"), (dict(first_step=-1), "first_step"),
                                     (dict(given=1, fill=-math.inf), "rows")])
def test_beam_rows_argument_errors(pkg, kw, word):
    assert call_beam_rows(pkg, **kw) == -1
    assert word in pkg._err(), pkg._err()


def call_beam_table(pkg, table=True, starts=True, out=True, state=True, R=4, n_vocab=40, given=1, start=(1, 2), plen=(3, 1), n_groups=2, n_beams=2, n_predict=4,
                    eos_id=3, lpen=1.0, es=1, max_steps=4, fill=-1.0):
    t = np.full((4, 40), fill, dtype=np.float32)
    st, pl = np.array(start, dtype=np.int32), np.array(plen, dtype=np.int32)
    o = np.zeros(2 * 2 * 16 * 2 * 8 * 4 + 64, dtype=np.float32)
    p = o.ctypes.data
    return pkg.lib().biogpt_hip_beam_table_device(0, t.ctypes.data if table else None, R, n_vocab, given, st.ctypes.data if starts else None, pl.ctypes.data, n_groups,
                                                  n_beams, n_predict, eos_id, lpen, es, max_steps, p if out else None, p, p, p, p, p, p, p, p, p, p, p if state else None)


@pytest.mark.parametrize("kw,word", [(dict(table=False), "table"), (dict(starts=False), "start_tokens"), (dict(out=False), "out_ids"), (dict(state=False), "kv_out"),
                                     (dict(n_beams=0), "n_beams"), (dict(n_beams=17), "n_beams"), (dict(n_groups=0), "n_groups"), (dict(n_beams=16, n_vocab=31), "n_vocab"),
                                     (dict(R=0), "n_table_rows"), (dict(n_predict=0), "n_predict"), (dict(max_steps=0), "max_steps"), (dict(eos_id=40), "eos_id"),
                                     (dict(eos_id=-2), "eos_id"), (dict(lpen=math.nan), "length_penalty"), (dict(lpen=math.inf), "length_penalty"),
                                     (dict(es=2), "early_stopping"), (dict(given=-1), "given"), (dict(plen=(0, 1)), "prompt_lens"), (dict(start=(1, 40)), "start_tokens"),
                                     (dict(fill=-math.inf), "table")])
def test_beam_table_argument_errors(pkg, kw, word):
    assert call_beam_table(pkg, **kw) == -1
    assert word in pkg._err(), pkg._err()


# ---- the fixtures of the tied searches test what they are there for (the restatement alone) ----

@pytest.fixture(scope="module")
def tied_runs():
    """{(V, B, early_stopping, length_penalty): (hyps, margins, trace)} of the first group of every tied case."""
    out = {}
    start = bk.GROUPS[0][0]
    for V, R, B in bk.tied_cases():
        for es in (True, False):
            for lpen in bk.TIED_PENALTIES:
                trace = []
                hyps, margins = bk.tied_reference(V, R, B, start, es, lpen, trace)
                out[(V, B, es, lpen)] = (hyps, margins, trace)
    return out


def test_tied_fixtures_have_ties_at_most_steps(tied_runs):
    steps = sum(len(m) for _, m, _ in tied_runs.values())
    zero = sum(sum(1 for g in m if g == 0.0) for _, m, _ in tied_runs.values())
    print("tied fixtures: %d of %d steps decide on a zero margin" % (zero, steps))
    assert 2 * zero >= steps, (zero, steps)


def test_tied_fixtures_finish_hypotheses_with_eos_and_stop_early(tied_runs):
    for V, R in bk.TIED_VOCABS:
        for B in bk.TIED_BEAMS:
            if B < 2:
                continue
            eos = bk.eos_of(V)
            assert any(len(ids) < bk.N_PREDICT and ids[-1] == eos for (v, b, _, _), (hyps, _, _) in tied_runs.items() if (v, b) == (V, B) for ids, _ in hyps), (V, B)
    assert any(len(m) < bk.N_PREDICT for _, m, _ in tied_runs.values())


def test_tied_fixtures_evict_from_the_pool(tied_runs):
    assert any(st["evicted"] for (_, _, es, _), (_, _, trace) in tied_runs.items() if not es for st in trace)


def test_tied_fixtures_fork_and_drop_parents(tied_runs):
    for (V, B, es, lpen), (_, _, trace) in tied_runs.items():
        if B < 2:
            continue
        twice = any(max(np.bincount(st["parents"], minlength=B)) >= 2 for st in trace[1:] if st["parents"])
        none = any(min(np.bincount(st["parents"], minlength=B)) == 0 for st in trace[1:] if st["parents"])
        assert twice and none, (V, B, es, lpen)


# ---- the references agree with each other ----

@pytest.mark.parametrize("V,R,B", [(33, 33, 16), (96, 96, 5), (1001, 1001, 8)])
def test_row_candidates_merged_are_the_restatements_candidates(V, R, B):
    """row_candidates over all rows of a step, merged and sorted by (score, parent rank, id), is the candidate list beam_search forms there."""
    table = bk.tied_table(V, R, bk.TIED_SEED)
    start = bk.GROUPS[1][0]
    trace = []
    beam_ref.running_beams(bk.table_logprobs(table, start), B, bk.N_PREDICT, 6, -1, 1.0, True, trace)
    assert len(trace) == 6
    running = [([], np.float32(0.0))]
    for st in trace:
        merged = []
        for rank, (hist, score) in enumerate(running):
            ids, sc = bk.row_candidates(table[(hist[-1] if hist else start) % R], 2 * B, score, True)
            merged += [(float(s), rank, int(i)) for i, s in zip(ids, sc)]
        merged.sort(key=lambda c: (-c[0], c[1], c[2]))
        assert [(float(s), p, i) for s, p, i in st["cand"]] == merged[:2 * B]
        running = [(running[p][0] + [i], np.float32(s)) for s, p, i in st["cand"][:B]]     # (no EOS: the first B candidates run on)


def test_log_softmax64_is_the_restatements_log_softmax():
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((4, 333)) * 2.5).astype(np.float32)
    want = beam_ref.log_softmax_rows(rows)
    for r in range(4):
        lp, am = bk.log_softmax64(rows[r])
        assert am == int(np.argmax(rows[r]))
        assert np.max(np.abs(lp - want[r].astype(np.float64))) <= 2e-6
