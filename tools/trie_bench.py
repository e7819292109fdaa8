#!/usr/bin/env python3
"""Cost of trie-constrained beam search on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): 8 prompts of 40 tokens x 5 beams, 16 tokens.

  calls     generate_beam_batch(trie=...) against generate_beam_batch without a trie, in one process, the two ALTERNATING repeat by repeat (other
            work shares the machine): milliseconds per call by host wall clock (every call returns after its stream has drained), after a warm-up;
            median, min, max and the spread (max - min) / median of each, and the median of the per-repeat differences.  Tries of 10^3 and 10^5
            random entries of 34 tokens over a pool of 4096 ids: no entry can finish within 16 tokens, so every call runs its 16 steps (the line
            says so: full_length).
  kernel    trie_rows_kernel alone (mode 1, 40 rows of 42384 logits), histories 1 / 8 / 32 tokens deep inside the trie: microseconds per launch
            between two device events (biogpt_hip_trie_rows_bench); depth 0 is the kernel without a walk.

Prints one JSON line."""
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
N_PROMPT, N_PREDICT, EOS, G, B = 40, 16, 2, 8, 5
ENTRY_LEN, POOL = 34, 4096


def stats(ts):
    med = float(np.median(ts))
    return dict(ms=round(med, 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4), spread=round((max(ts) - min(ts)) / med, 4), n=len(ts))


def alternate(fa, fb, reps, warmup):
    for _ in range(warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--layers", type=int, default=24, help="fewer layers: a rehearsal, not a measurement")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "trie_bench", "model": "synthetic BioGPT-base, %d layers, q4_0" % a.layers, "n_prompt": N_PROMPT, "n_predict": N_PREDICT, "eos_id": EOS,
           "prompts": G, "beams": B, "reps": a.reps, "warmup": a.warmup}
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED, **dict(m.BIOGPT_BASE, n_layer=a.layers))
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        V = g.n_vocab
        prompts = [[2] + [int(v) for v in rng.integers(4, V, N_PROMPT - 1)] for _ in range(G)]
        pool = rng.choice(np.arange(4, V), POOL, replace=False)
        kw = dict(n_beams=B, eos_id=EOS, length_penalty=1.0, early_stopping=True, n_batch=8)
        free = lambda: g.generate_beam_batch(prompts, N_PREDICT, **kw)
        for n_entries in (1000, 100000):
            entries = rng.choice(pool, (n_entries, ENTRY_LEN))
            t0 = time.perf_counter()
            trie = m.Trie.build(entries, V)
            build_ms = (time.perf_counter() - t0) * 1e3
            held = lambda: g.generate_beam_batch(prompts, N_PREDICT, trie=trie, **kw)
            tf, tt = alternate(free, held, a.reps, a.warmup)
            r = dict(free=stats(tf), trie=stats(tt), diff_ms=round(float(np.median(np.array(tt) - np.array(tf))), 4), info=trie.info(), build_ms=round(build_ms, 1))
            r["full_length"] = bool(all(max(len(i) for i, _ in h) == N_PREDICT for h in free()[0]) and all(max(len(i) for i, _ in h) == N_PREDICT for h in held()[0]))
            # the kernel alone: 40 rows, histories inside the trie
            rows = (rng.standard_normal((G * B, V)) * 3.0).astype(np.float32)
            for depth in (0, 1, 8, 32):
                hs = [[int(t) for t in entries[int(i)][:depth]] for i in rng.integers(0, n_entries, G * B)]
                _, us = m.trie_rows(rows, trie, hs, mode=1, eos_id=EOS, reps=a.kernel_reps)
                us = us[a.kernel_reps // 10:]
                r["kernel_us_depth_%d" % depth] = dict(us=round(float(np.median(us)), 2), min=round(float(us.min()), 2), max=round(float(us.max()), 2), n=int(us.size))
            res["entries_%d" % n_entries] = r
            trie.close()
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
