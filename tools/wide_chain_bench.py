#!/usr/bin/env python3
"""The wide chain on a synthetic Q4_0 file at BioGPT-Large's sizes (48 layers, d_model 1600, d_ff 6400, 25 heads, n_vocab 57717): milliseconds per call by
host wall clock (every call returns after its stream has drained), warm-up 2, median of 9, the two routes of a row alternating.  Prints one JSON line:

  score_batch_64x64      biogpt_hip_score_batch of 64 sequences x 64 tokens        against the loop of 64 biogpt_hip_score calls a caller had before
  greedy_batch_8x64      biogpt_hip_generate_greedy_batch, 8 prompts x 64 tokens   against the loop of 8 biogpt_hip_generate_greedy calls
  greedy_batch_64x64     the same with 64 prompts                                  against the loop of 64 calls (--loop64-reps repeats: 4096 single-token passes each)
  kernel                 matmul_wide_kernel alone (device events) at (K 1600, M 4800) and (K 6400, M 1600), N = 16 / 64 / 512, and the BioGPT-base
                         matmul_mfma_kernel at out_proj (K 1024) / fc2 (K 4096) with the same N: microseconds, and `per_mac_vs_base` = (base us per block
                         MAC) / (wide us per block MAC) -- what a pipelined wide kernel could still win is 1 / that.

The loops run on the generic kernels of the same build: nothing of theirs changed.  A row where the batched route loses shows ratio > 1.

  python tools/wide_chain_bench.py [--layers 48] [--reps 9] [--warmup 2] [--loop64-reps 3] [--skip-calls] [--skip-kernel]
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
LARGE = dict(n_vocab=57717, n_head=25, n_positions=1024, d_ff=6400, d_model=1600, n_merges=40000)
Q4_0 = 2


def alternating(fa, fb, reps, warmup):
    """a, b, a, b, ...: (ms of a, ms of b) as dicts of median / min / max."""
    ta, tb = [], []
    for i in range(warmup + reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
    d = lambda ts: dict(ms=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3), n=len(ts))
    return d(ta), d(tb)


def row(batched, loop, tokens):
    return dict(batched=batched, loop=loop, ratio=round(batched["ms"] / loop["ms"], 4), batched_tok_s=round(tokens / batched["ms"] * 1e3), loop_tok_s=round(tokens / loop["ms"] * 1e3))


def calls(m, path, a):
    g = m.BiogptModel.load(path)
    rng = np.random.default_rng(5)
    V = LARGE["n_vocab"]
    seqs = [[2] + [int(v) for v in rng.integers(4, V, 63)] for _ in range(64)]
    prompts = [[2] + [int(v) for v in rng.integers(4, V, 7)] for _ in range(64)]
    res = {}
    b, l = alternating(lambda: g.score_batch(seqs), lambda: [g.score(s) for s in seqs], a.reps, a.warmup)
    res["score_batch_64x64"] = row(b, l, 64 * 64)
    b, l = alternating(lambda: g.generate_greedy_batch(prompts[:8], 64), lambda: [g.generate_greedy(p, 64) for p in prompts[:8]], a.reps, a.warmup)
    res["greedy_batch_8x64"] = row(b, l, 8 * 64)
    b, l = alternating(lambda: g.generate_greedy_batch(prompts, 64), lambda: [g.generate_greedy(p, 64) for p in prompts], a.loop64_reps, 1)
    res["greedy_batch_64x64"] = row(b, l, 64 * 64)
    res["chain_kind"], res["wide_launches"] = g.chain_kind(), g.wide_launches()
    g.close()
    return res


def kernel(m, a):
    out = {}
    for K, M, KB in ((1600, 4800, 1024), (6400, 1600, 4096)):
        for N in (16, 64, 512):
            w = float(np.median(m.wide_chain_bench("wide", Q4_0, M, K, N, a.reps)))
            b = float(np.median(m.wide_chain_bench("base", Q4_0, 1024, KB, N, a.reps)))
            macs_w, macs_b = M * (K // 32) * N, 1024 * (KB // 32) * N
            out["K%d_M%d_N%d" % (K, M, N)] = dict(wide_us=round(w, 2), base_us=round(b, 2), base_shape="K%d_M1024" % KB,
                                                  per_mac_vs_base=round((b / macs_b) / (w / macs_w), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop64-reps", type=int, default=3)
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "wide_chain_bench", "model": "synthetic BioGPT-Large sizes, %d layers, q4_0" % a.layers, "reps": a.reps, "warmup": a.warmup, "loop64_reps": a.loop64_reps}
    if not a.skip_kernel:
        res["kernel"] = kernel(m, a)
    if not a.skip_calls:
        with tempfile.TemporaryDirectory() as td:
            f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **LARGE)
            m.quantize_file(f32, q40, "q4_0")
            os.remove(f32)
            res.update(calls(m, q40, a))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
