#!/usr/bin/env python3
"""Log-probabilities of generated tokens on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per call by host wall clock
(every call returns after its stream has drained).  16-token prompts, 64 new tokens, n_batch 8, no EOS; sampling with top_k 40, top_p 0.9, temp 0.9.
The routes of one (mode, sequence count) run in turn, round after round -- `--warmup` rounds thrown away, then `--reps` rounds (median, min, max) -- so a
drift of the machine meets every route alike.  Prints one JSON line with, per mode (greedy, sample) and sequence count (8, 64, 256):

  plain         generate_greedy_batch / generate_sample as before
  lp0, lp5      the same call with logprobs=0 / logprobs=5
  plain_score   the route logprobs=0 replaces: the plain call, then score_batch of every prompt ++ continuation
  and the ratios lp0 / plain, lp5 / plain, lp0 / plain_score

  python tools/genlp_bench.py [--reps 9] [--warmup 2] [--routes plain,lp0,lp5,plain_score] [--counts 8,64,256] [--modes greedy,sample]

--routes plain uses nothing this tool's commit added: the file runs unchanged in a checkout of the parent commit, for the plain call's before / after.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 0x42494F47
N_PROMPT, N_PREDICT = 16, 64
TOP_K, TOP_P, TEMP = 40, 0.9, 0.9


def summary(ts):
    return dict(ms=round(float(np.median(ts)), 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4), n=len(ts))


def timed_in_turn(routes, reps, warmup):
    """{name: summary}: every round runs each route once, in the order given."""
    ts = {name: [] for name in routes}
    for rd in range(warmup + reps):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            if rd >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: summary(v) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--routes", default="plain,lp0,lp5,plain_score")
    ap.add_argument("--counts", default="8,64,256")
    ap.add_argument("--modes", default="greedy,sample")
    a = ap.parse_args()
    want = a.routes.split(",")
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "genlp_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_prompt": N_PROMPT, "n_predict": N_PREDICT, "n_batch": 8,
           "top_k": TOP_K, "top_p": TOP_P, "temp": TEMP, "eos_id": -1, "reps": a.reps, "warmup": a.warmup, "routes": want}
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prompts = [[2] + [int(v) for v in rng.integers(4, g.n_vocab, N_PROMPT - 1)] for _ in range(256)]
        skw = dict(top_k=TOP_K, top_p=TOP_P, temp=TEMP, seed=1, eos_id=-1, n_batch=8)
        for mode in a.modes.split(","):
            for n in [int(v) for v in a.counts.split(",")]:
                ps = prompts[:n]
                if mode == "greedy":
                    gen = lambda **kw: g.generate_greedy_batch(ps, N_PREDICT, n_batch=8, **kw)
                else:
                    gen = lambda **kw: g.generate_sample(ps, N_PREDICT, **skw, **kw)

                def plain_score():
                    ids = gen()[0]
                    return g.score_batch([p + [int(t) for t in s] for p, s in zip(ps, ids)])

                table = dict(plain=lambda: gen(), lp0=lambda: gen(logprobs=0), lp5=lambda: gen(logprobs=5), plain_score=plain_score)
                r = timed_in_turn({name: table[name] for name in want}, a.reps, a.warmup)
                for num, den in (("lp0", "plain"), ("lp5", "plain"), ("lp0", "plain_score")):
                    if num in r and den in r:
                        r["%s/%s" % (num, den)] = round(r[num]["ms"] / r[den]["ms"], 4)
                res["%s_%d" % (mode, n)] = r
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
