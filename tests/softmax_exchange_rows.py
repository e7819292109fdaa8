"""The rows of tests/test_gpu_softmax_exchange.py, stated once: which files, which tokens, which oracle rows -- so that tests/test_softmax_exchange_rows.py can
look at exactly those rows on the CPU (how many of them have a top-two gap too small to ask for the arg-max).

The softmax of the pipelined decode launch's attention stage (csrc/kernels_xpipe.hip.h, stage B of xp_run): up to 128 keys every wave works the whole softmax
out for itself behind one exchange -- lane j holds the numerators of keys j and j + 64 in two registers, their sum is one unsigned sum of numerator * 2^24
(128 numerators of 1.0: 2^31), and wave w takes the weights of its keys w + 8 k from lane w + 8 (k mod 8) of register k / 8; beyond 128 keys the stage makes
two exchanges.  The compared contexts:
  n_past 0, 1, 63                    64-key variant: first key, last key
  64 .. 72, 127                      128-key variant: both registers, the token's own key in slots 8 and 9 of a wave (64 .. 71: slot 8 of waves 0 .. 7; 72:
                                     slot 9 of wave 0), in every wave, and (63 / 127) in the last slot of a register
  128, 129, 191 / 192, 255           192- / 256-key variants: first and last key
  256, 257                           two workgroups per head
The context between them is filled by chunk evals (up to 8 tokens), fed to the oracle in the same calls.

Files: peaked.q4_0 (tests/wide_models.py: scores x 16 and x 144 in layers 0 and 1 -- most numerators exactly 0, the maximum's exactly 1.0) and two "uniform"
files (q_proj weight and bias 0 in layers 0 and 1: every score is 0, every numerator exactly 1.0 -- the largest sum a context can have), Q4_0 and Q5_1 (the
second with Q8_1 activations: the attention output leaves with its block sums)."""
import os

import numpy as np

import wide_models as wm

FILES = ["peaked.q4_0", "uniform.q4_0", "uniform.q5_1"]
CONTEXTS = (0, 1, 63) + tuple(range(64, 73)) + (127, 128, 129, 191, 192, 255, 256, 257)
GAP = 2e-3                       # the arg-max is asserted where the oracle's top-two gap is at least twice the 1e-3 bar on logits
CAP = 1.0 / 20.0                 # ... and at most this share of a file's compared rows may fall below it
SEEDS = {}                       # token seed per file, default 1 (tests/test_softmax_exchange_rows.py holds them to CAP on the CPU)
GEN_FILES = ["peaked.q4_0", "uniform.q4_0"]
N_PROMPT, N_GEN = 60, 140        # generate_greedy over 60 .. 199 keys: the 64-, 128-, 192- and 256-key variants in one call


def uniform(W):
    """q_proj weight and bias x 0 in layers 0 and 1: q = 0, every score exactly 0.  Layer 2 is the control."""
    for l in (0, 1):
        for part in ("weight", "bias"):
            wm._own(W, wm.lname(l, "self_attn.q_proj.%s" % part))[...] = 0.0


def build(pkg, d):
    """Write FILES into directory d; returns {name: path}."""
    out = wm.build(pkg, d, ["peaked.q4_0", "plain.f32"])
    hp, vocab, merges, order, W = wm.load_arrays(out.pop("plain.f32"))
    T = dict(W)
    uniform(T)
    f32 = os.path.join(str(d), "uniform.f32.bin")
    wm.save_arrays(f32, hp, vocab, merges, order, T)
    for typ in ("q4_0", "q5_1"):
        out["uniform." + typ] = os.path.join(str(d), "uniform.%s.bin" % typ)
        pkg.quantize_file(f32, out["uniform." + typ], typ)
    os.remove(f32)
    return out


def plan(name):
    """[(tokens, n_past, compared)]: single tokens at CONTEXTS, chunks of up to 8 tokens between them."""
    t = wm.tokens(SEEDS.get(name, 1), CONTEXTS[-1] + 1)
    steps, at = [], 0
    for c in CONTEXTS:
        while at < c:
            n = min(8, c - at)
            steps.append((t[at:at + n], at, False))
            at += n
        steps.append((t[c:c + 1], c, True))
        at = c + 1
    return steps


def prompt_tokens(name):
    return wm.tokens(1000 + SEEDS.get(name, 1), N_PROMPT)


def oracle_rows(O, path, name, n_threads):
    """{n_past: float32 [n_vocab]}: the oracle's logits row of every compared step of the plan."""
    o = O.OracleModel(path, n_threads=n_threads)
    rows = {}
    for toks, n_past, compared in plan(name):
        lo = o.eval(toks, n_past)
        if compared:
            rows[n_past] = np.array(lo, dtype=np.float32)
            rows[n_past].setflags(write=False)
    o.close()
    return rows


def close_rows(rows):
    """n_past of the rows whose top-two gap is below GAP."""
    return [n_past for n_past in sorted(rows) if wm.top_two_gap(rows[n_past]) < GAP]
