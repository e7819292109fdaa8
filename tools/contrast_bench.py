#!/usr/bin/env python3
"""Contrastive search on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): biogpt_hip_generate_contrastive against
biogpt_hip_generate_greedy_batch with the same number of columns (n_prompts x top_k sequences) and n_predict + 1 steps -- the forward passes
of a contrastive call without its penalty, selection and K / V row copies.  Milliseconds per call by host wall clock (every call returns
after its stream has drained), warm-up 2, median of 9, spread = (max - min) / median.  Cases (n_prompts, top_k, prompt tokens, n_predict):

  1x4x16x64  8x4x16x64  64x4x16x64  1x8x16x64  8x8x16x64  64x8x16x64      short contexts
  1x4x512x64                                                                 one long context: 512 - 575 context rows per step

The yardstick function is unchanged on the parent commit, so the same script times it there (--greedy-only works on a build without
contrastive search).  One JSON line per case: both medians and spreads, and ratio = contrastive / greedy.

  python tools/contrast_bench.py [--reps 9] [--warmup 2] [--only 64x4x16x64] [--greedy-only] [--contrastive-only]
                                 (--only with --contrastive-only: one case in this process, e.g. under a kernel trace)
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
CASES = [(1, 4, 16, 64), (8, 4, 16, 64), (64, 4, 16, 64), (1, 8, 16, 64), (8, 8, 16, 64), (64, 8, 16, 64), (1, 4, 512, 64)]
ALPHA = 0.6


def key(case):
    return "%dx%dx%dx%d" % case


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
    ap.add_argument("--only", default="")
    ap.add_argument("--greedy-only", action="store_true")
    ap.add_argument("--contrastive-only", action="store_true")
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
        for case in CASES:
            if a.only and key(case) != a.only:
                continue
            G, k, n_prompt, n = case
            rng = np.random.default_rng(G * 100 + k)
            prompts = [[2] + [int(v) for v in rng.integers(4, g.hparams.n_vocab, n_prompt - 1)] for _ in range(G)]
            out = {"case": key(case), "n_prompts": G, "top_k": k, "prompt_tokens": n_prompt, "n_predict": n, "columns": G * k}
            if not a.greedy_only:
                ts = timed(lambda: g.generate_contrastive(prompts, n, top_k=k, penalty_alpha=ALPHA), a.reps, a.warmup)
                out["contrastive"] = stats(ts)
            if not a.contrastive_only:
                cols = [p for p in prompts for _ in range(k)]      # the same columns: every prompt k times
                ts = timed(lambda: g.generate_greedy_batch(cols, n + 1), a.reps, a.warmup)
                out["greedy_batch"] = stats(ts)
            if "contrastive" in out and "greedy_batch" in out:
                out["ratio"] = round(out["contrastive"]["median_ms"] / out["greedy_batch"]["median_ms"], 4)
            print(json.dumps(out), flush=True)
        g.close()


if __name__ == "__main__":
    main()
