"""The rows of tests/test_gpu_pv_context.py, stated once: which files, which tokens, which oracle rows -- so that tests/test_pv_context_rows.py can look at
exactly those rows on the CPU (how many of them have a top-two gap too small to ask for the arg-max).

The walk: teacher-forced single tokens at every n_past from 0 to 272 on three wide files of tests/wide_models.py.  In the attention stage of the pipelined
decode launch (csrc/kernels_xpipe.hip.h, stage B of xp_run) wave w of a head's workgroup holds the value rows of keys w + 8 k; the walk meets every count of
old keys per wave of the 64- / 128- / 192- / 256-key variants (0 .. 8 / 16 / 24 / 32), the token's own key in every wave (0 .. 7) and in slots of both
parities, the first and the last key of each variant, and from 256 keys on the second workgroup of a head from its first key on (0 .. 2 old keys per wave
there, all 32 in the first).  rawq8 and the combined files have peaked attention (layers 0 and 1): many softmax weights are exactly 0."""
import numpy as np

import wide_models as wm

FILES = ["combined.q4_0", "combined.q5_1", "rawq8"]
N_ROWS = 273                     # n_past 0 .. 272
GAP = 2e-3                       # the arg-max is asserted where the oracle's top-two gap is at least twice the 1e-3 bar on logits
CAP = 1.0 / 20.0                 # ... and at most this share of a walk's rows may fall below it
SEEDS = {}                       # token seed per file, default 1 (tests/test_pv_context_rows.py holds them to CAP on the CPU)
PROMPTS = (4, 66, 130, 194, 258) # the ordinary multi-token launches: one prompt per variant (64 / 128 / 192 / 256 keys, two workgroups per head)
N_GEN = 58


def walk_tokens(name):
    return wm.tokens(SEEDS.get(name, 1), N_ROWS)


def prompt_tokens(name, n):
    return wm.tokens(1000 + SEEDS.get(name, 1), n)


def oracle_walk(O, path, name, n_threads):
    """(tokens, float32 [N_ROWS, n_vocab]): the oracle's logits row of every step of the walk."""
    o = O.OracleModel(path, n_threads=n_threads)
    toks = walk_tokens(name)
    rows = np.stack([o.eval([toks[n_past]], n_past) for n_past in range(N_ROWS)])
    o.close()
    return toks, rows


def close_rows(rows):
    """n_past of the rows whose top-two gap is below GAP."""
    return [n_past for n_past in range(len(rows)) if wm.top_two_gap(rows[n_past]) < GAP]
