#!/usr/bin/env python3
"""Prompt-lookup decoding on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): biogpt_hip_generate_lookup against the greedy calls that give
the same ids -- biogpt_hip_generate_greedy for one prompt, biogpt_hip_generate_greedy_batch for eight.  Milliseconds per call by host wall clock (every
call returns after its stream has drained), warm-up 2, median of 9, spread = (max - min) / median.  16-token random prompts, 64 tokens, max_draft 7,
max_ngram 3, at the two ends of acceptance:

  copy   corpus = the prompt's own greedy continuation: nearly every draft is right (about 8 tokens per pass)
  none   no corpus, random prompt: nothing to copy but what the model repeats of itself -- what a caller pays when speculation never helps

The yardstick functions are unchanged on the parent commit, so the same script times them there (--greedy-only works on a build without prompt-lookup
decoding).  One JSON line per case: the medians and spreads, ratio = lookup / greedy, the mean tokens per pass, and per prompt count the tokens per pass at
which lookup breaks even with greedy: the line through the two ends, time per pass taken as constant (t_none / passes_none).

  python tools/lookup_bench.py [--reps 9] [--warmup 2] [--only 1] [--greedy-only] [--max-draft 7] [--max-ngram 3]
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


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def stats(ts):
    med = float(np.median(ts))
    return {"median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "spread": round((max(ts) - min(ts)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--greedy-only", action="store_true")
    ap.add_argument("--max-draft", type=int, default=7)
    ap.add_argument("--max-ngram", type=int, default=3)
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.lib()
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED, **{k: v for k, v in m.BIOGPT_BASE.items() if k != "ftype"})
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40, device=0)
        for G in (1, 8):
            if a.only and G != a.only:
                continue
            rng = np.random.default_rng(G * 100 + 7)
            prompts = [[2] + [int(v) for v in rng.integers(4, g.hparams.n_vocab, N_PROMPT - 1)] for _ in range(G)]
            out = {"n_prompts": G, "prompt_tokens": N_PROMPT, "n_predict": N_PREDICT, "max_draft": a.max_draft, "max_ngram": a.max_ngram}
            if G == 1:
                want = [[int(t) for t in g.generate_greedy(prompts[0], N_PREDICT)[0]]]
                out["greedy"] = stats(timed(lambda: g.generate_greedy(prompts[0], N_PREDICT), a.reps, a.warmup))
            else:
                want = [[int(t) for t in row] for row in g.generate_greedy_batch(prompts, N_PREDICT)[0]]
            out["greedy_batch"] = stats(timed(lambda: g.generate_greedy_batch(prompts, N_PREDICT), a.reps, a.warmup))
            base = out["greedy" if G == 1 else "greedy_batch"]["median_ms"]
            if not a.greedy_only:
                ends = {}
                for end, corpus in (("copy", want), ("none", None)):
                    kw = dict(max_draft=a.max_draft, max_ngram=a.max_ngram, corpus=corpus)
                    ids, st, _ = g.generate_lookup(prompts, N_PREDICT, **kw)
                    assert [list(i) for i in ids] == want, "lookup ids differ from the greedy ids"
                    r = stats(timed(lambda: g.generate_lookup(prompts, N_PREDICT, **kw), a.reps, a.warmup))
                    r["ratio"] = round(r["median_ms"] / base, 4)
                    r["passes"] = max(s["passes"] for s in st)      # the call runs until its slowest prompt is done
                    r["tokens_per_pass"] = round(sum(s["passes"] + s["accepted"] for s in st) / sum(s["passes"] for s in st), 3)
                    out["lookup_" + end] = ends[end] = r
                per_pass = ends["none"]["median_ms"] / ends["none"]["passes"]
                out["ms_per_pass_none"] = round(per_pass, 4)
                out["ms_per_pass_copy"] = round(ends["copy"]["median_ms"] / ends["copy"]["passes"], 4)
                out["break_even_tokens_per_pass"] = round(N_PREDICT * per_pass / base, 3)      # N_PREDICT / tpp passes of per_pass ms each = the greedy call
            print(json.dumps(out), flush=True)
        g.close()


if __name__ == "__main__":
    main()
