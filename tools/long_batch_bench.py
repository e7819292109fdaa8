#!/usr/bin/env python3
"""The batched calls of a wide file at 1025 .. 2048 keys (csrc/kernels_attn_long_cols.hip.h) on a synthetic file at BioGPT-Large's sizes (d_model 1600, d_ff 6400,
25 heads, n_vocab 57717, 2048 positions): host wall clock around calls that return after their stream has drained, warm-up 2, median of 9 (min - max), the two
routes of a row alternating in one process.  Every yardstick is an unchanged route of the same build -- the loop of single-context calls with long_context on;
the parent commit has none, it refuses these calls.  A row the batched call loses says LOSS.  Prints one JSON line.

  kernels                  by device events through the probe's timing loop (a repeated stand-alone launch finds its K / V rows in cache), 25 heads: the run
                           form against the column form on the same packed pass (2048 columns of one sequence; 64 runs of 8 behind 1500 shared rows), and the
                           column form at 64 / 256 decode columns at 1100 / 2048 keys
  score_batch_4x2048       score_batch of 4 x 2048 tokens against the loop of score
  greedy_batch_8 / _64     generate_greedy_batch of 8 / 64 prompts of 1400 + 200 tokens against loops of generate_greedy
  continuations_64x8       score_continuations of 64 x 8 tokens behind 1500 against score of the concatenations
  (BIOGPT_HIP_LONG_RUNS=0 / 1 in the environment gives the form rule's A/B arms on the call rows)

  python tools/long_batch_bench.py [--layers 48] [--types q4_0] [--reps 9] [--warmup 2] [--skip-kernels] [--skip-calls]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.join(ROOT, "tools"))
from wide_decode_bench import LARGE, SEED, alternating, stats      # noqa: E402

LARGE_2048 = dict(LARGE, n_positions=2048)
H = 25


def row(new, old, names=("batched", "loop")):
    r = {names[0]: stats(new), names[1]: stats(old)}
    r["ratio"] = round(r[names[0]]["ms"] / r[names[1]]["ms"], 3)
    r["verdict"] = "win" if r["ratio"] < 1.0 else "LOSS"
    return r


def calls(m, path, a):
    rng = np.random.default_rng(5)
    toks = [[2] + [int(v) for v in rng.integers(4, LARGE["n_vocab"], 2047)] for _ in range(64)]
    g, one = m.BiogptModel.load(path), m.BiogptModel.load(path, long_context=True)
    both = lambda f_new, f_old: alternating([f_new, f_old], a.reps, a.warmup)
    res = {}
    res["score_batch_4x2048"] = row(*both(lambda: g.score_batch(toks[:4]), lambda: [one.score(t) for t in toks[:4]]))
    for n in (8, 64):
        prompts = [t[:1400] for t in toks[:n]]
        res["greedy_batch_%d" % n] = row(*both(lambda: g.generate_greedy_batch(prompts, 200), lambda: [one.generate_greedy(p, 200) for p in prompts]))
    prefix, conts = toks[0][:1500], [t[1500:1508] for t in toks]
    res["continuations_64x8"] = row(*both(lambda: g.score_continuations(prefix, conts), lambda: [one.score(prefix + c) for c in conts]))
    res["long_cols_launches"] = g.long_cols_launches()
    g.close(); one.close()
    return res


def kernels(m, a):
    rng = np.random.default_rng(7)
    out = {}

    def us(form, P, t_max, n_slots, states, K, V, **kw):
        q = (rng.standard_normal((len(states), H * 64)) * 0.125).astype(np.float32)
        r = m.attn_long_cols_device(form, H, P, t_max, n_slots, q, K, V, states, q8=0, reps=a.reps, **kw)
        if r[0] != 0:
            raise m.BiogptError(m._err())
        return round(float(np.median(r[6])), 2)

    def pair(name, states, n_slots, t_max, shared):
        K, V = (rng.standard_normal((n_slots, H, 2048, 64)).astype(np.float32) for _ in range(2))
        r = dict(runs_us=us(1, 2048, t_max, n_slots, states, K, V), columns_us=us(0, 2048, t_max, n_slots, states, K, V, shared=shared))
        r["runs_over_columns"] = round(r["runs_us"] / r["columns_us"], 3)
        r["verdict"] = "win" if r["runs_over_columns"] < 1.0 else "LOSS"
        out[name] = r

    pair("packed_2048_of_one_sequence", [[i, 0, 0, 0, i + 1, 0, 0, 0] for i in range(2048)], 1, 2048, False)
    # 64 continuations of 8 tokens in slots 1 .. 8 (eight continuations share a slot's rows: the launch is the same, the image stays small) behind 1500 rows of slot 0
    pair("64_runs_of_8_behind_1500", [[1499 + i, 0, 0, 1 + c % 8, 1500 + i, 1499, 0, 0] for c in range(64) for i in range(8)], 9, 1507, True)
    for N in (64, 256):
        K, V = (rng.standard_normal((8, H, 2048, 64)).astype(np.float32) for _ in range(2))
        for T in (1100, 2048):      # (decode columns: packed states that name one of 8 slots, every column at T keys)
            out["columns_N%d_T%d_us" % (N, T)] = us(0, 2048, T, 8, [[T - 1, 0, 0, i % 8, T, 0, 0, 0] for i in range(N)], K, V)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--types", default="q4_0")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.lib()
    res = {"metric": "long_batch_bench", "model": "synthetic BioGPT-Large sizes, %d layers, %d positions" % (a.layers, LARGE_2048["n_positions"]), "reps": a.reps,
           "warmup": a.warmup, "long_runs": os.environ.get("BIOGPT_HIP_LONG_RUNS", "-1")}
    if not a.skip_kernels:
        res["kernels"] = kernels(m, a)
    with tempfile.TemporaryDirectory() as td:
        f32 = os.path.join(td, "f32.bin")
        if not a.skip_calls:
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **LARGE_2048)
        for name in a.types.split(","):
            if a.skip_calls:
                break
            print("long_batch_bench: %s" % name, file=sys.stderr, flush=True)
            path = os.path.join(td, name + ".bin")
            m.quantize_file(f32, path, name)
            res[name] = calls(m, path, a)
            os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
