#!/usr/bin/env python3
"""The SIMD chain (biogpt_hip_assoc_chain) on synthetic 24-layer BioGPT-base files, Q4_0 / Q5_1 / Q8_0 (d_model 1024, d_ff 4096, 16 heads, n_vocab 42384, 512
positions): host wall clock around calls that return after their stream has drained, warm-up 2, median of 9 (min - max), the routes of a row alternating in one
process.  The yardstick of every row is an UNCHANGED route of the same build in mode 1 -- the single-sequence call in a loop -- never the code under test.
Prints one JSON line.

  score_64x64     score_batch of 64 sequences of 64 tokens                 against the loop of score
  score_1x512     score_batch of one 512-token sequence                    against score of it
  greedy_Nx64     generate_greedy_batch of N = 8 / 64 / 256 prompts of 16 tokens + 64 new ones
                                                                           against loops of generate_greedy (above --loop-cap prompts the loop runs over the
                                                                           first --loop-cap of them and is scaled by N / cap: "loop_scaled_from" says so)
  kernels         the stage alone per site at N = 8, 64, 512 (device events): schain_kernel at the launch's own tile shape and at each forced one, its
                  producer, matvec_simd_kernel at N = 8 times N / 8 (the yardstick), and -- for scale only -- the mode-0 matrix-core stage

  python tools/simd_chain_bench.py [--layers 24] [--types q4_0,q5_1,q8_0] [--reps 9] [--warmup 2] [--loop-cap 32] [--skip-kernels] [--skip-calls]
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
BASE = dict(n_vocab=42384, n_head=16, n_positions=512, d_ff=4096, d_model=1024, n_merges=40000)
WTYPES = {"q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8}
SITES = (("qkv", 1024, 3072), ("out_proj", 1024, 1024), ("fc1", 1024, 4096), ("fc2", 4096, 1024), ("lm_head", 1024, 42384))
N_PROMPT, N_GEN = 16, 64


def stats(ts, tokens):
    ts = np.asarray(ts)
    return dict(ms=round(float(np.median(ts)), 3), min=round(float(ts.min()), 3), max=round(float(ts.max()), 3), n=int(ts.size),
                tok_s=round(tokens / float(np.median(ts)) * 1e3, 1))


def alternating(fns, reps, warmup):
    """fns[0], fns[1], ..., fns[0], ...: the milliseconds of each."""
    ts = [[] for _ in fns]
    for i in range(warmup + reps):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                t.append((time.perf_counter() - t0) * 1e3)
    return ts


def row(batched, loop, tokens, scale=1.0, scaled_from=None):
    loop = [t * scale for t in loop]
    r = dict(batched=stats(batched, tokens), loop=stats(loop, tokens))
    r["batched_over_loop"] = round(r["batched"]["ms"] / r["loop"]["ms"], 3)
    r["verdict"] = "win" if r["batched_over_loop"] < 1.0 else "LOSS"
    if scaled_from is not None:
        r["loop_scaled_from"] = scaled_from
    return r


def calls(m, path, a):
    rng = np.random.default_rng(5)
    V = BASE["n_vocab"]
    seq = lambda n: [2] + [int(v) for v in rng.integers(4, V, n - 1)]
    chain = m.BiogptModel.load(path, assoc="simd", assoc_chain=True)      # the batched calls
    alone = m.BiogptModel.load(path, assoc="simd")                        # the yardstick: a context in mode 1 as it was
    res = {}
    seqs = [seq(64) for _ in range(64)]
    tb, tl = alternating([lambda: chain.score_batch(seqs), lambda: [alone.score(s) for s in seqs]], a.reps, a.warmup)
    res["score_64x64"] = row(tb, tl, 64 * 64)
    long_seq = seq(512)
    tb, tl = alternating([lambda: chain.score_batch([long_seq]), lambda: alone.score(long_seq)], a.reps, a.warmup)
    res["score_1x512"] = row(tb, tl, 512)
    for n in (8, 64, 256):
        prompts = [seq(N_PROMPT) for _ in range(n)]
        cap = min(n, a.loop_cap)
        reps = a.reps if n <= 64 else max(3, a.reps // 3)
        tb, tl = alternating([lambda: chain.generate_greedy_batch(prompts, N_GEN), lambda: [alone.generate_greedy(p, N_GEN) for p in prompts[:cap]]], reps, a.warmup)
        res["greedy_%dx%d" % (n, N_GEN)] = row(tb, tl, n * N_GEN, n / cap, cap if cap < n else None)
    res["stage_launches"] = chain.simd_chain_launches()
    chain.close(); alone.close()
    return res


def kernels(m, wtype, a):
    out = {}
    med = lambda us: round(float(np.median(us)), 2)
    for site, K, M in SITES:
        mv8 = med(m.schain_bench("matvec", wtype, M, K, 8, reps=a.reps))
        for N in (8, 64, 512):
            r = dict(stage_us=med(m.schain_bench("stage", wtype, M, K, N, -1, a.reps)), q8_us=med(m.schain_bench("q8", wtype, M, K, N, reps=a.reps)),
                     matvec8_scaled_us=round(mv8 * N / 8, 2))
            for cfg in (0, 1, 2):
                r["stage_cfg%d_us" % cfg] = med(m.schain_bench("stage", wtype, M, K, N, cfg, a.reps))
            if M % 16 == 0:
                r["mode0_mfma_us"] = med(m.schain_bench("wide", wtype, M, K, N, reps=a.reps))
            r["stage_and_q8_over_matvec8"] = round((r["stage_us"] + r["q8_us"]) / r["matvec8_scaled_us"], 3)
            out["%s_N%d" % (site, N)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--types", default="q4_0,q5_1,q8_0")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-cap", type=int, default=32)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "simd_chain_bench", "model": "synthetic BioGPT-base sizes, %d layers, %d positions" % (a.layers, BASE["n_positions"]), "reps": a.reps,
           "warmup": a.warmup}
    with tempfile.TemporaryDirectory() as td:
        f32 = os.path.join(td, "f32.bin")
        if not a.skip_calls:
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **BASE)
        for name in a.types.split(","):
            res[name] = {}
            if not a.skip_kernels:
                res[name]["kernels"] = kernels(m, WTYPES[name], a)
            if not a.skip_calls:
                path = os.path.join(td, name + ".bin")
                m.quantize_file(f32, path, name)
                res[name].update(calls(m, path, a))
                os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
