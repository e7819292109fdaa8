#!/usr/bin/env python3
"""Cost of whole-vocabulary sampling on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): 16-token prompts, 64 new tokens, 8 / 64 / 256
sequences.

  calls     generate_sample(sampler=...) for the nucleus (0, 0.9, 0.9), ancestral (0, 1, 1) and min-p (0, 1, 1.5, min_p 0.05) samplers against the unchanged
            plain call generate_sample(top_k=64, top_p=0.9, temp=0.9), in one process, the routes ALTERNATING repeat by repeat (other work shares the
            machine): milliseconds per call by host wall clock (every call returns after its stream has drained), after a warm-up; median, min, max
            of each and the ratio of the medians to the plain call's.
  kernel    sample_wide_rows_kernel alone on 256 rows of 42384 logits -- a flat N(0, 0.5) set and a peaked N(0, 3) set -- for the same three samplers,
            against sample_rows_kernel at k = 64: microseconds per launch between two device events (biogpt_hip_sample_wide_rows_bench).

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
N_PROMPT, N_PREDICT = 16, 64
PLAIN = dict(top_k=64, top_p=0.9, temp=0.9)
SAMPLERS = {"nucleus": (0, 0.9, 0.0, 0.9), "ancestral": (0, 1.0, 0.0, 1.0), "min_p": (0, 1.0, 0.05, 1.5)}      # (top_k, top_p, min_p, temp)


def stats(ts):
    return dict(ms=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3), n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--seqs", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--layers", type=int, default=24, help="fewer layers: a rehearsal, not a measurement")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "wide_sample_bench", "model": "synthetic BioGPT-base, %d layers, q4_0" % a.layers, "n_prompt": N_PROMPT, "n_predict": N_PREDICT, "plain": PLAIN,
           "samplers": SAMPLERS, "reps": a.reps, "warmup": a.warmup}
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED, **dict(m.BIOGPT_BASE, n_layer=a.layers))
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        V = g.n_vocab
        for n in a.seqs:
            prompts = [[2] + [int(v) for v in rng.integers(4, V, N_PROMPT - 1)] for _ in range(n)]
            routes = {"plain": lambda: g.generate_sample(prompts, N_PREDICT, seed=1, **PLAIN)}
            for name, sp in SAMPLERS.items():
                routes[name] = (lambda sp: lambda: g.generate_sample(prompts, N_PREDICT, seed=1, sampler=sp))(sp)
            for _ in range(a.warmup):
                for f in routes.values():
                    f()
            ts = {name: [] for name in routes}
            for _ in range(a.reps):
                for name, f in routes.items():
                    t0 = time.perf_counter()
                    f()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            r = {name: stats(t) for name, t in ts.items()}
            for name in SAMPLERS:
                r[name]["ratio"] = round(r[name]["ms"] / r["plain"]["ms"], 4)
            res["seqs_%d" % n] = r
        g.close()
    # the kernels alone
    n_rows = 256
    states = np.zeros((n_rows, 625), dtype=np.uint32)
    for r in range(n_rows):
        assert m.lib().biogpt_hip_mt19937_seed(100 + r, states[r].ctypes.data) == 0
    for label, sigma in (("flat", 0.5), ("peaked", 3.0)):
        rows = (rng.standard_normal((n_rows, 42384)) * sigma).astype(np.float32)
        k = {}
        cut = a.kernel_reps // 10
        us = m.sample_wide_rows_bench(rows, (64, 0.9, 0.0, 0.9), states, which=1, reps=a.kernel_reps)[cut:] * 1e6
        k["sample_rows_kernel_k64"] = dict(us=round(float(np.median(us)), 1), min=round(float(us.min()), 1), max=round(float(us.max()), 1))
        for name, sp in SAMPLERS.items():
            us = m.sample_wide_rows_bench(rows, sp, states, which=0, reps=a.kernel_reps)[cut:] * 1e6
            k[name] = dict(us=round(float(np.median(us)), 1), min=round(float(us.min()), 1), max=round(float(us.max()), 1))
        res["kernel_256_rows_" + label] = k
    print(json.dumps(res))


if __name__ == "__main__":
    main()
