#!/usr/bin/env python3
"""Beam search on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per call by host wall clock (every
call returns after its stream has drained), after a warm-up, `--reps` repeats (median, min, max).  Prints one JSON line:

  beam_B      biogpt_hip_generate_beam, a 40-token prompt, n_predict 64, no EOS (every call runs 64 steps), B beams; ms per call and
              per step (call / 64), against biogpt_hip_generate_greedy_batch of B copies of the prompt (same column count, same
              decode path) in the same process, and the ratio beam / greedy_batch

  python tools/beam_bench.py [--reps 10] [--warmup 2] [--only 5]    (--only: one beam count, beam calls only, e.g. under a kernel trace)
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
N_PROMPT, N_PREDICT = 40, 64


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(float(np.median(ts)), 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4), n=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, default=0)
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "beam_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_prompt": N_PROMPT, "n_predict": N_PREDICT,
           "eos_id": -1, "reps": a.reps, "warmup": a.warmup}
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prompt = [2] + [int(v) for v in rng.integers(4, g.n_vocab, N_PROMPT - 1)]
        for B in ([a.only] if a.only else [1, 4, 5, 8]):
            bm = timed(lambda: g.generate_beam(prompt, N_PREDICT, n_beams=B, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8),
                       a.reps, a.warmup)
            r = dict(beam=bm, beam_ms_per_step=round(bm["ms"] / N_PREDICT, 4))
            if not a.only:
                gb = timed(lambda: g.generate_greedy_batch([prompt] * B, N_PREDICT, n_batch=8), a.reps, a.warmup)
                r.update(greedy_batch=gb, greedy_batch_ms_per_step=round(gb["ms"] / N_PREDICT, 4), ratio=round(bm["ms"] / gb["ms"], 4))
            res["beam_%d" % B] = r
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
