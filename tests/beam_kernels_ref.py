"""References and fixtures for the tests of the scoring and beam-step kernels on their own (test_gpu_beam_kernels.py, test_beam_kernels_capi.py):
logprob_rows_kernel / lp_row_stats (kernels_score.hip.h) and beam_group_rows_kernel, beam_group_select_kernel, kv_group_fork_kernel
(kernels_beam.hip.h), reached through biogpt_hip_logprob_rows_device, biogpt_hip_beam_rows_device and biogpt_hip_beam_table_device.  Plain numpy,
float64 where arithmetic is involved.

Not a test module: a helper the tests import."""
import math

import numpy as np

import beam_ref

WIDTHS = (42384, 42383, 1021, 320, 70, 33)     # 33 = 2 * BEAM_MAX + 1: with 16 beams fewer threads than K hold an element
BEAMS = (1, 2, 4, 5, 8, 12, 16)                # 2B <= 8, <= 16, <= 32: the three instantiations of the row kernel
LP_THREADS = 256


# ---- one row ----

def log_softmax64(row):
    """(float64 log-softmax of an f32 row, its first arg-max)."""
    r = np.asarray(row, dtype=np.float32).astype(np.float64)
    m = r.max()
    return (r - m) - math.log(np.exp(r - m).sum()), int(np.argmax(r))


def lp_tolerance(n_vocab, ref):
    """The bound on |lp - ref| for logprob_rows_kernel: lp = (l - m) - log(S) in double, rounded once.  S is a sum of f32 per-lane sums (each of at
    most ceil(V / 256) + 4 terms: one f32 rounding per addition, relative to a partial sum no larger than the whole) of expf values good to 2 ulp;
    the lanes are combined in double.  So S is off by at most (ceil(V / 256) + 8) * 2^-23 relatively, which is the absolute error of log(S); the
    rounding of the result adds half an ulp of it."""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return (math.ceil(n_vocab / LP_THREADS) + 8) * 2.0 ** -23 + 0.5 * np.spacing(ref.astype(np.float32)).astype(np.float64)


def row_candidates(row, K, run_score, given):
    """What beam_group_rows_kernel writes for a row: (ids, scores) of its K best entries, equal values: lower id first.  score =
    f32(run_score + lp) with lp the row value itself (given) or f32(log_softmax64)."""
    r = np.asarray(row, dtype=np.float32)
    ids = np.argsort(-r.astype(np.float64), kind="stable")[:K]
    lp = r[ids] if given else log_softmax64(r)[0][ids].astype(np.float32)
    return ids.astype(np.int64), (np.float32(run_score) + lp).astype(np.float32)


# ---- hostile rows ----

def _gauss(rng, n, V):
    return (rng.standard_normal((n, V)) * 2.5).astype(np.float32)


def dominant_places(V):
    return [0, 1, 2, 3, V - 1, V - 2, V - 3, V - 4, V // 2]


def wave_first_places(V):
    """An index among the first elements each of the four waves reads (thread 0, 64, 128, 192: float4 number t of an aligned row), and the last."""
    return sorted(set(min(4 * t, V - 1) for t in (0, 64, 128, 192)) | {V - 1})


def row_kinds(V, B, given, seed):
    """{kind: float32 [n >= 4][V]} -- at least four rows per kind, so that with an odd V every 16-byte alignment occurs in every kind."""
    rng = np.random.default_rng([seed, V, B, int(given)])
    K = 2 * B
    out = {}
    out["gauss"] = _gauss(rng, 4, V)
    out["quantised"] = (np.round(_gauss(rng, 4, V) * 2.0) / 2.0).astype(np.float32)
    out["equal"] = np.repeat(np.array([[0.0], [-7.25], [3.5], [1e4]], dtype=np.float32), V, axis=1)
    dom = _gauss(rng, len(dominant_places(V)), V)
    for r, at in enumerate(dominant_places(V)):
        dom[r, at] = dom[r].max() + np.float32(60.0)
    out["dominant"] = dom
    dup = _gauss(rng, 4, V)
    for r in range(4):
        dup[r, wave_first_places(V)] = np.float32(np.ceil(dup[r].max()) + 1.0 + r)
    out["max_in_every_wave"] = dup
    out["huge"] = (rng.uniform(-1e4, 1e4, (4, V))).astype(np.float32)
    # the best 2B values in one thread's float4 stride (indices congruent modulo 4 * 256), or as many of them as the row has
    stride = _gauss(rng, 4, V)
    for r in range(4):
        at = np.arange((r * 5) % min(V, 1024), V, 1024)[:K]
        stride[r, at] = stride[r].max() + np.float32(1.0) + rng.permutation(at.size).astype(np.float32) * np.float32(0.25)
    out["one_stride"] = stride
    if given:
        for kind in ("gauss", "quantised", "dominant", "max_in_every_wave", "huge", "one_stride"):      # log-probabilities are <= 0
            out[kind] = (out[kind] - out[kind].max(axis=1, keepdims=True)).astype(np.float32)
        out["equal"] = -np.abs(out["equal"])
        for name, n_inf in (("inf_30", int(0.3 * V)), ("inf_90", int(0.9 * V)), ("inf_all_but_2B", V - K)):
            rows = out["quantised"].copy() if name == "inf_90" else (_gauss(rng, 4, V) - np.float32(12.0)).clip(max=0.0).astype(np.float32)
            n_inf = min(n_inf, V - K)      # never fewer than 2B finite values: the call's own precondition
            for r in range(4):
                rows[r, rng.permutation(V)[:n_inf]] = -np.inf
            out[name] = rows
    return out


# ---- tied searches ----

TIED_VOCABS = ((33, 33), (96, 96), (1001, 1001), (42384, 64))     # (n_vocab, table rows)
TIED_BEAMS = (1, 2, 5, 8, 16)
TIED_PENALTIES = (0.0, 1.0, 2.0)
N_PREDICT = 16
GROUPS = ((5, 3), (17, 9), (30, 1))      # (start token, n_prompt) of the three groups; a search of one group is the first


def eos_of(V):
    return 7 if V > 33 else 4


def tied_table(V, R, seed):
    """Log-probability rows whose finite entries are negative multiples of 1/8 in [-3, -1/8] (every f32 sum of 16 of them is exact: ties are true
    ties on the device and in the restatement), 30 % of the entries -inf (none at V = 33, where a row must keep 2 * 16 finite ones), and the EOS
    column at -1/8 in a quarter of the rows and -2 elsewhere."""
    rng = np.random.default_rng([seed, V, R])
    t = (-rng.integers(1, 25, (R, V)) / 8.0).astype(np.float32)
    if V > 33:
        t[rng.random((R, V)) < 0.3] = -np.inf
    t[:, eos_of(V)] = np.where(rng.random(R) < 0.25, np.float32(-0.125), np.float32(-2.0))
    return t


def table_logprobs(table, start, given=True):
    """The callback of beam_ref.beam_search for a table: the row of a prefix is the row of its last token (of the start token at first)."""
    t = np.asarray(table, dtype=np.float32)
    lp = t if given else np.stack([log_softmax64(r)[0].astype(np.float32) for r in t])
    return lambda prefixes: np.stack([lp[(p[-1] if len(p) else start) % lp.shape[0]] for p in prefixes])


TIED_SEED = 3      # the first seed whose tables meet every fixture condition of test_beam_kernels_capi.py


def tied_cases():
    for V, R in TIED_VOCABS:
        for B in TIED_BEAMS:
            yield V, R, B


def tied_reference(V, R, B, start, es, lpen, trace=None):
    """(hyps, margins) of the restatement for one group of a tied case."""
    cb = table_logprobs(tied_table(V, R, TIED_SEED), start)
    if trace is None:
        return beam_ref.beam_search(cb, B, N_PREDICT, eos_of(V), lpen, es)
    hyps, margins, _ = beam_ref._search(cb, B, N_PREDICT, eos_of(V), lpen, es, None, trace)
    return hyps, margins


def stamp(token, pos, head, kv):
    """The K (kv = 0) or V (kv = 1) row biogpt_hip_beam_table_device leaves for a token at a position (include/biogpt_hip.h)."""
    return np.array([token, pos, 2 * head + kv, (token + 7 * pos + 3 * head + kv) & 0xffff], dtype=np.float32)
