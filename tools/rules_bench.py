#!/usr/bin/env python3
"""Cost of the generation rules on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per call by host wall clock (every
call returns after its stream has drained), after a warm-up, `--reps` repeats (median, min, max, and the spread (max - min) / median).  A 40-token
prompt, n_predict 64, EOS id 2 with min_new_tokens 64 where rules are on (every call runs its 64 steps; the line says so: full_length).

  beam_5        biogpt_hip_generate_beam, 5 beams
  sample_N      biogpt_hip_generate_sample, N prompts, one sample each (top_k 40, top_p 0.9, temp 0.9)

  python tools/rules_bench.py --rules 0     no rule: only arguments every commit with the two entry points has, so the same file measures a parent commit
  python tools/rules_bench.py --rules 1     all four rules active

Prints one JSON line.  Compare `--rules 0` of two commits for the neutral path, and `--rules 1` against `--rules 0` for the cost of the rules."""
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
N_PROMPT, N_PREDICT, EOS = 40, 64, 2
RULES = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=N_PREDICT, suppress_tokens=[11, 12, 13])


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ts))
    return dict(ms=round(med, 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4), spread=round((max(ts) - min(ts)) / med, 4), n=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rules", type=int, default=1)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="one shape, e.g. beam_5 or sample_64 (under a kernel trace)")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    rules = dict(RULES) if a.rules else {}
    res = {"metric": "rules_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_prompt": N_PROMPT, "n_predict": N_PREDICT, "eos_id": EOS,
           "rules": rules, "reps": a.reps, "warmup": a.warmup}
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prompts = [[2] + [int(v) for v in rng.integers(4, g.n_vocab, N_PROMPT - 1)] for _ in range(256)]
        if a.only in ("", "beam_5"):
            call = lambda: g.generate_beam(prompts[0], N_PREDICT, n_beams=5, eos_id=EOS, length_penalty=1.0, early_stopping=True, n_batch=8, **rules)
            r = timed(call, a.reps, a.warmup)
            r["full_length"] = bool(max(len(i) for i, _ in call()[0]) == N_PREDICT)
            res["beam_5"] = r
        for n in (8, 64, 256):
            if a.only not in ("", "sample_%d" % n):
                continue
            call = lambda: g.generate_sample(prompts[:n], N_PREDICT, top_k=40, top_p=0.9, temp=0.9, seed=1, eos_id=EOS, n_batch=8, **rules)
            r = timed(call, a.reps, a.warmup)
            r["full_length"] = bool(all(len(i) == N_PREDICT for i in call()[0]))
            r["tok_per_s"] = round(n * N_PREDICT / r["ms"] * 1e3, 1)
            res["sample_%d" % n] = r
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
