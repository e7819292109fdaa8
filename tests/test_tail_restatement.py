"""The restatement of the token tail (tests/tail_ref.py), its case list (tests/tail_cases.py) and the probe (biogpt_hip_tail_device), without a GPU: the rule on
rows written out by hand; every named mistake, committed in the restatement, changes an expected output of a case; the cases are what their text says -- the
ties lie where the kernels combine, the edited rows are NaN / +inf / -inf, each NaN part's true maximum sits beside the NaN -- and every TOPK case takes the
outcome (an answer, or a refusal) written down for it; the probe's symbol is declared, exported and bound and refuses bad arguments by name before any HIP call;
the three host selections of biogpt_hip_eval_topk, through the probe, give the restatement's pairs on every TOPK case."""
import ctypes
import os
import re

import numpy as np
import pytest

import chain_ref as R
import tail_cases as C
import tail_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAN, INF = np.nan, np.inf


# ---- the rule ----

def test_rule_by_hand():
    row = np.array([1.0, NAN, 3.0, 3.0, -INF, INF, NAN, INF], F32)
    assert T.order(row).tolist() == [5, 7, 2, 3, 0, 4]
    assert T.argmax(row) == 5 and T.argmax([NAN, NAN]) == 0 and T.argmax([-INF, -INF]) == 0 and T.argmax([NAN, -INF]) == 1
    pv, pi = T.partials(row, 2)
    assert pi.tolist() == [0, 2, 5, 7] and pv.tolist()[1:] == [3.0, INF, INF]
    pv, pi = T.partials([NAN, NAN, -INF, -INF, 5.0], 2)
    assert pi.tolist() == [T.NONE_IDX, 2, 4] and pv.tolist() == [-INF, -INF, 5.0]
    v, i = T.topk(row, 3)
    assert i.tolist() == [5, 7, 2] and v.tolist() == [INF, INF, 3.0]
    assert T.topk([NAN, 1.0], 2)[1].tolist() == [1] and T.full_row([NAN, 1.0, NAN], 3)[1].tolist() == [1, 0, 2]
    assert T.finish([1.0, 1.0, NAN], [70, 3, 1], 100) == 3 and T.finish([NAN], [3], 100) == 0 and T.finish([-INF], [T.NONE_IDX], 100) == 0
    assert T.finish([2.0], [100], 100) == 0 and T.finish([2.0], [-1], 100) == 0
    assert T.block_maxima(np.r_[np.zeros(64), np.full(64, NAN), [NAN, 2.0]]).tolist() == [0.0, -INF, 2.0]


def test_threshold_by_hand():
    pm = np.arange(24, dtype=F32)                                   # groups of 8: maxima 7, 15, 23
    assert T.topk_threshold(pm, 24, 1) == (23.0, False) and T.topk_threshold(pm, 24, 3) == (7.0, False)
    assert T.topk_threshold(pm, 24, 4) == (-INF, False)              # more than the groups
    assert T.topk_threshold(np.zeros(1025, F32), 1025, 1) == (-INF, False)
    pm[3] = NAN
    assert T.topk_threshold(pm, 24, 3) == (7.0, False)               # fmaxf passes a NaN over
    pm[0:8] = NAN
    assert T.topk_threshold(pm, 24, 2) == (15.0, False) and T.topk_threshold(pm, 24, 1)[1]


# ---- every named mistake is seen ----

def _partials_rows():
    for wtype, M, edits in ((R.Q8_0, 1045, True), (R.Q4_0, 129, False), (R.Q8_0, 65, False)):
        c = C.partials_case(wtype, M, edits)
        yield "%s M%d" % (R.NAMES[wtype], M), c["want"], c["rpp"]
    row = np.r_[np.zeros(64, F32), [NAN, 5.0], np.zeros(62, F32), np.zeros(16, F32)].astype(F32)
    row[-1] = 1.0
    yield "by hand", row, 64


def _differs(a, b):
    return any(not np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b)) if isinstance(a, tuple) else a != b


def _seen_in(mistake):
    hits = []
    for name, row, rpp in _partials_rows():
        want = T.partials(row, rpp)
        if len(want[0]) != len(T.partials(row, rpp, mistake)[0]) or _differs(want, T.partials(row, rpp, mistake)):
            hits.append("PARTIALS " + name)
    for name, v, i in C.finish_cases():
        if T.finish(v, i, C.N_VOCAB) != T.finish(v, i, C.N_VOCAB, mistake):
            hits.append("FINISH " + name)
    for c in C.topk_cases():
        if c["row"].size > 9000 and c["row"].size not in (43009, 44100) and "candidates" not in c["name"]:
            continue
        a, b = T.topk_kernel(c["row"], c["pmax"], c["pmax"].size, c["k"]), T.topk_kernel(c["row"], c["pmax"], c["pmax"].size, c["k"], mistake)
        if a[0] != b[0] or (a[0] > 0 and _differs(a[1:], b[1:])):
            hits.append("TOPK " + c["name"])
        if c["row"].size <= 9000:
            if _differs(T.host_topk(c["row"], c["k"])[1:], T.host_topk(c["row"], c["k"], mistake)[1:]):
                hits.append("HOST_TOPK " + c["name"])
            if c["true_max"] and _differs(T.host_topk_blocks(c["row"], c["k"], c["pmax"])[1:], T.host_topk_blocks(c["row"], c["k"], c["pmax"], mistake)[1:]):
                hits.append("HOST_BLOCKS " + c["name"])
    return hits


# (topk_kernel's and host_topk's restatements state their tie rule through their own steps: rank_by_slot and host_ge are their tie mistakes)
WHERE = {"tie_higher_id": ("PARTIALS", "FINISH"), "tie_within_wave_only": ("PARTIALS", "FINISH"), "nan_seed": ("PARTIALS", "FINISH"),
         "last_block_dropped": ("PARTIALS",), "unclamped_empty": ("FINISH",), "candidates_gt": ("TOPK",), "cap_off_by_one": ("TOPK",), "rank_by_slot": ("TOPK",),
         "beyond_regs_dropped": ("TOPK",), "host_ge": ("HOST_TOPK",), "blocks_select_gt": ("HOST_BLOCKS",)}


@pytest.mark.parametrize("mistake", sorted(T.MISTAKES))
def test_every_mistake_changes_an_expected_output(mistake):
    assert set(WHERE) == set(T.MISTAKES)
    hits = _seen_in(mistake)
    for stage in WHERE[mistake]:
        assert any(h.startswith(stage + " ") for h in hits), (mistake, stage, hits[:5])


# ---- the cases are what they say ----

def test_the_column_is_not_fragile():
    """The lm_head kernels sum the LayerNorm's doubles in their own association: the row's bits are owed to chain_ref only while that cannot decide a float32."""
    assert not R.ln_fragile(C.column()[0])


@pytest.mark.parametrize("wtype", (C.F32_TYPE,) + R.TYPES, ids=("f32",) + tuple(R.NAMES[t] for t in R.TYPES))
def test_partials_cases_hold_their_ties(wtype):
    kinds = set()
    for M in C.PARTIAL_M:
        c = C.partials_case(wtype, M)
        row, rpp = c["want"], c["rpp"]
        assert row.shape == (M,) and np.isfinite(row).all()
        pv, pi = T.partials(row, rpp)
        for kind, (p, rows) in c["ties"].items():
            kinds.add(kind)
            assert len(set(row[rows].view(np.uint32).tolist())) == 1, (M, kind)
            if kind == "across parts":
                assert row[rows[0]] == row.max() and T.argmax(row) == rows[0] and len({r // rpp for r in rows}) >= 2, (M, kind)
                lo = [r for r in rows if r // rpp == p][-1]
                assert lo % rpp == rpp - 1 and any(r % rpp == 0 and r > lo for r in rows)        # the winner's part holds it in its LAST row, a later part in its first
            else:
                assert all(r // rpp == p for r in rows) and pi[p] == rows[0] and row[rows[0]] == row[p * rpp:(p + 1) * rpp].max(), (M, kind)
                if kind == "same wave":
                    assert rows[1] - rows[0] == 1 and rows[0] % 2 == 0
                if kind == "across waves":
                    assert (rows[0] % rpp) // max(rpp // 4, 1) != (rows[1] % rpp) // max(rpp // 4, 1)
                if kind == "last part":
                    assert p == len(pi) - 1 and (M % rpp != 0 or M < 64 or wtype == C.F32_TYPE or M in (64, 128, 1040))
    assert kinds == ({"same wave", "across waves", "last part", "across parts"} if wtype != C.F32_TYPE else kinds) and "across parts" in kinds


@pytest.mark.parametrize("M,lm_stream", ((1045, True), (C.FULL_M, True), (C.FULL_M, False)))
def test_q8_edit_cases_hold_their_rows(M, lm_stream):
    c = C.partials_case(R.Q8_0, M, True, lm_stream)
    row, rpp, made = c["want"], c["rpp"], c["edits"]
    assert rpp == (64 if M == C.FULL_M else 8) and C.expected_kernel(R.Q8_0, M, lm_stream) == (0 if (lm_stream and M == C.FULL_M) else 1)
    pv, pi = T.partials(row, rpp)
    assert len(pv) == -(-M // rpp) and (M != C.FULL_M or (len(pv) == 663 and M - 662 * 64 == 16))
    for at, mx in (C.NAN_PAIRS_64 if rpp == 64 else C.NAN_PAIRS_8):
        p = made["nan %d max %d" % (at, mx)]
        part = row[p * rpp:(p + 1) * rpp]
        assert np.isnan(part[at]) and np.isnan(part).sum() == 1 and pi[p] == p * rpp + mx and part[mx] > np.nanmax(np.delete(part, mx))
    p = made["all nan"]
    assert np.isnan(row[p * rpp:(p + 1) * rpp]).all() and pv[p] == -INF and pi[p] == T.NONE_IDX
    p = made["all -inf"]
    assert (row[p * rpp:(p + 1) * rpp] == -INF).all() and pv[p] == -INF and pi[p] == p * rpp
    p = made["one -inf"]
    assert row[p * rpp + 1] == -INF and np.isfinite(pv[p])
    p = made["+inf tied in a part"]
    assert (row[p * rpp:(p + 1) * rpp] == INF).sum() == 2 and pi[p] == p * rpp + 3 and pv[p] == INF
    p2 = made["+inf in a later part"]
    assert pv[p2] == INF and T.finish(pv, pi, M) == p * rpp + 3
    assert len(c["ties"]) == 4


def test_finish_cases():
    names = [n for n, _, _ in C.finish_cases()]
    assert len(set(names)) == len(names) and {v.size for _, v, _ in C.finish_cases()} >= set(C.FINISH_NPARTS)
    for name, v, i in C.finish_cases():
        tok = T.finish(v, i, C.N_VOCAB)
        assert 0 <= tok < C.N_VOCAB
        if "all nan" in name or "never written" in name or "past the vocabulary" in name or "negative" in name:
            assert tok == 0 and T.finish(v, i, C.N_VOCAB, "unclamped_empty") != 0, name
        if "all -inf" in name:
            assert tok == int(i.min()), name
        if "one comparable" in name:
            assert tok == int(i[v.size // 2]), name
        if "top tied" in name and v.size > 1:
            tied = np.flatnonzero(v == v.max())
            assert len(tied) >= 2 and tok == int(i[tied].min()), name
            if "lowest id last" in name:
                assert int(np.argmin(i[tied])) == len(tied) - 1, name


# what each TOPK case must take: an answer (k) or a refusal (-1), by what its text says
# (V 4097 with k 40 / 64: k exceeds the 9 groups of 65 maxima, so there is no threshold and the whole row -- 4097 logits -- is a candidate; V 4096 is answered)
REFUSED = ("4097 candidates", "too high", "below the whole row", "three comparable, k 7", "V4097 k40 normal", "V4097 k64 normal")
ANSWERED = ("4096 candidates", "too low", "tie straddles", "nan among the maxima", "a group of nan maxima", "+-inf and nan", "three comparable, k 2", "all -inf but a nan",
            "normal", "nparts 1024")


def test_topk_cases_take_the_outcome_written_down():
    cases = C.topk_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    assert {c["row"].size for c in cases} >= set(C.TOPK_V) | set(C.TOPK_K) and {c["k"] for c in cases} == set(C.TOPK_K)
    refused = answered = 0
    for c in cases:
        row, k, pm = c["row"], c["k"], c["pmax"]
        n, v, i = T.topk_kernel(row, pm, pm.size, k)
        want_v, want_i = T.topk(row, k)
        assert n in (k, -1), c["name"]
        if n == k:      # never another answer
            assert np.array_equal(i, want_i) and v.tobytes() == want_v.tobytes(), c["name"]
        with np.errstate(invalid="ignore"):
            over = int((row >= T.topk_threshold(pm, pm.size, k)[0]).sum())
        assert (n == -1) == (over > T.TOPK_CAP or over < k), c["name"]
        if any(t in c["name"] for t in REFUSED):
            assert n == -1, c["name"]
        elif any(t in c["name"] for t in ANSWERED):
            assert n == k, c["name"]
        refused, answered = refused + (n == -1), answered + (n == k)
        if c["true_max"]:
            assert np.array_equal(pm, T.block_maxima(row)), c["name"]
        if row.size >= 43009 and "normal" in c["name"]:
            assert (want_i >= 43008).any(), c["name"]
    assert refused >= 12 and answered >= 60
    by = {c["name"]: c for c in cases}
    for k in (2, 7, 40, 64):
        c = by["k%d tie straddles place k" % k]
        v, i = T.topk(c["row"], k + 2)
        assert v[k - 2] > v[k - 1] == v[k] == v[k + 1] and i[k - 1] == 77
    assert by["nparts 10 < k 40"]["pmax"].size == 10 and by["nparts 1025"]["pmax"].size == 1025
    assert T.topk_kernel(by["nparts 1025"]["row"], by["nparts 1025"]["pmax"], 1025, 7)[0] == -1      # no threshold beyond 1024 partials: the whole row is a candidate


# ---- the probe ----

def test_symbol_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "biogpt_hip.h")).read()
    name = "biogpt_hip_tail_device"
    assert re.search(r"\b%s\s*\(" % name, hdr)
    assert name in {n for n, _, _ in pkg.SYMBOLS}
    assert getattr(ctypes.CDLL(pkg.LIB_PATH), name) is not None
    assert getattr(pkg.lib(), name).restype is ctypes.c_int
    assert callable(pkg.tail_device)


_Z = np.zeros(1024, F32)
REFUSALS = [
    ("an unknown type", dict(stage="PARTIALS", wtype=1, w_rows=np.zeros((1, 2048), np.uint8), M=1, x=_Z, ln_w=_Z, ln_b=_Z), "type 1 is neither F32 nor a block format"),
    ("M 0", dict(stage="PARTIALS", wtype=0, w_rows=np.zeros((1, 1024), F32), M=0, x=_Z, ln_w=_Z, ln_b=_Z), r"M must be in \[1, 131072\]"),
    ("ln_b missing", dict(stage="PARTIALS", wtype=0, w_rows=np.zeros((1, 1024), F32), x=_Z, ln_w=_Z), "w_rows, x, ln_w or ln_b is NULL"),
    ("no partials", dict(stage="FINISH", pmax_val=np.zeros(0, F32), pmax_idx=np.zeros(0, np.int32)), r"nparts must be in \[1, 4096\]"),
    ("4097 partials", dict(stage="FINISH", pmax_val=np.zeros(4097, F32), pmax_idx=np.zeros(4097, np.int32)), r"nparts must be in \[1, 4096\]"),
    ("n_positions 0", dict(stage="FINISH", pmax_val=np.zeros(1, F32), pmax_idx=np.zeros(1, np.int32), n_positions=0), r"n_positions must be in \[1, 4096\]"),
    ("n_gen negative", dict(stage="FINISH", pmax_val=np.zeros(1, F32), pmax_idx=np.zeros(1, np.int32), state=(0, -1, 0, 0)), "n_gen -1 is negative"),
    ("n_vocab 0", dict(stage="FINISH", pmax_val=np.zeros(1, F32), pmax_idx=np.zeros(1, np.int32), n_vocab=0), "n_vocab must be at least 1"),
    ("k 0", dict(stage="TOPK", row=np.zeros(8, F32), pmax_val=np.zeros(1, F32), k=0), r"k must be in \[1, min\(64, V\)\]"),
    ("k 65", dict(stage="HOST_TOPK", row=np.zeros(100, F32), k=65), r"k must be in \[1, min\(64, V\)\]"),
    ("k over V", dict(stage="HOST_FULL", row=np.zeros(3, F32), k=4), r"k must be in \[1, min\(64, V\)\]"),
    ("no maxima", dict(stage="TOPK", row=np.zeros(8, F32), k=1), "part_in_val is NULL"),
    ("4097 maxima", dict(stage="TOPK", row=np.zeros(8, F32), pmax_val=np.zeros(4097, F32), k=1), r"nparts must be in \[1, 4096\]"),
    ("maxima of other blocks", dict(stage="HOST_BLOCKS", row=np.zeros(130, F32), pmax_val=np.zeros(2, F32), k=1), "walks the row's 3 64-row blocks"),
    ("no row", dict(stage="HOST_TOPK", k=1), r"V must be in \[1, 1048576\]"),
]


@pytest.mark.parametrize("what,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_probe_refuses_before_any_hip_call(pkg, what, kw, text):
    with pytest.raises(pkg.BiogptError, match=text):      # (there is no device here: a HIP call would make it -2 with HIP's message)
        pkg.tail_device(**kw)


def test_refusal_returns_minus_one(pkg):
    rc = pkg.lib().biogpt_hip_tail_device(0, 6, 0, 1, None, None, None, None, None, None, None, 0, 0, None, 0, 0, 0, None, None, None, None, None)
    assert rc == -1 and b"no stage" in pkg.lib().biogpt_hip_last_error()


# ---- the host selections, through the probe ----

def _whole(got, n, v, i, name):
    """The first n pairs are (v, i); every entry behind them keeps its 0xff preset."""
    assert got["n"] == n, (name, got["n"], n)
    assert got["vals"][:n].tobytes() == np.asarray(v, F32)[:n].tobytes() and got["ids"][:n].tolist() == np.asarray(i)[:n].tolist(), name
    assert (got["vals"][n:].view(np.uint32) == 0xFFFFFFFF).all() and (got["ids"][n:] == -1).all() and (got["count"][1:] == -1).all(), name


def test_host_selections_on_every_case(pkg):
    ran = 0
    for c in C.topk_cases():
        row, k, pm, name = c["row"], c["k"], c["pmax"], c["name"]
        want_v, want_i = T.topk(row, k)
        n, v, i = T.host_topk(row, k)
        assert n == len(want_i) and np.array_equal(i, want_i), name              # the restatement of the walk is the rule
        _whole(pkg.tail_device("HOST_TOPK", row=row, k=k), n, v, i, name)
        fv, fi = T.full_row(row, k)
        _whole(pkg.tail_device("HOST_FULL", row=row, k=k), k, fv, fi, name)
        assert np.array_equal(fi[:len(want_i)], want_i), name
        if c["true_max"] or (np.isnan(pm).any() and pm.size == -(-row.size // 64)):      # true maxima (or a NaN among them: the walk hands over to host_topk)
            n, v, i = T.host_topk_blocks(row, k, pm)
            assert n == len(want_i) and np.array_equal(i, want_i), name
            _whole(pkg.tail_device("HOST_BLOCKS", row=row, pmax_val=pm, k=k), n, v, i, name)
            ran += 1
    assert ran >= 80


def test_host_blocks_needs_true_maxima(pkg):
    """Why the stale-maxima cases stop at topk_kernel and host_topk: the block walk never looks into a block whose maximum says no, so a maximum that is too low
    costs it the block's members -- another answer.  The engine hands it the maxima the resident launch wrote behind the very row it selects from."""
    c = {c["name"]: c for c in C.topk_cases()}["stale maxima, another row's"]
    n, v, i = T.host_topk_blocks(c["row"], c["k"], c["pmax"])
    got = pkg.tail_device("HOST_BLOCKS", row=c["row"], pmax_val=c["pmax"], k=c["k"])
    _whole(got, n, v, i, c["name"])
    assert not np.array_equal(i, T.topk(c["row"], c["k"])[1])
