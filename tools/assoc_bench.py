#!/usr/bin/env python3
"""The SIMD association (biogpt_hip_assoc, mode 1) on synthetic 24-layer BioGPT-base files, Q4_0 / Q5_1 / Q8_0 (d_model 1024, d_ff 4096, 16 heads, n_vocab 42384):
host wall clock around calls that return after their stream has drained, warm-up 2, median of 9 (min - max), the routes of a row alternating.  Prints one JSON line.

  decode      biogpt_hip_generate_greedy, a 16-token prompt + 200 tokens, tokens per second:
                (a) simd         the context in mode 1
                (b) scalar_five  mode 0 of the same build on its own five launches per layer (BIOGPT_HIP_XPIPE=0, BIOGPT_HIP_NO_FUSED_DECODE=1): the
                                 like-for-like launch structure, the yardstick of the kernels
                (c) scalar       mode 0 as shipped
                (d) oracle_avx2  OracleModel(assoc = 7) on 16 threads: the only other thing that computes mode 1's bits
  prompt      a 512-token prompt through biogpt_hip_eval_prompt in chunks of 8, tokens per second, (a) / (b) / (c)
  kernels     each new kernel alone per site (device events): matvec_simd_kernel against the scalar association's mat-vec of the five-launch route at the
              shapes of q/k/v, out_proj, fc1, fc2 and the lm_head, one column and eight; attn_simd_kernel at 64 / 256 / 1024 keys, 16 heads
  diverge     for 8 prompts, the index of the first of 200 greedy ids at which modes 0 and 1 part (-1: none) -- recorded, not asserted

  python tools/assoc_bench.py [--layers 24] [--types q4_0,q5_1,q8_0] [--reps 9] [--warmup 2] [--skip-oracle] [--skip-kernels] [--skip-calls]
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
BASE = dict(n_vocab=42384, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
WTYPES = {"q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8}
SITES = (("qkv", 1024, 3072), ("out_proj", 1024, 1024), ("fc1", 1024, 4096), ("fc2", 4096, 1024), ("lm_head", 1024, 42384))
N_PROMPT, N_GEN = 16, 200


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


def load_five_launch(m, path):
    """Mode 0 on five launches per layer: the options are read when the context is created."""
    keep = {k: os.environ.get(k) for k in ("BIOGPT_HIP_XPIPE", "BIOGPT_HIP_NO_FUSED_DECODE")}
    os.environ["BIOGPT_HIP_XPIPE"], os.environ["BIOGPT_HIP_NO_FUSED_DECODE"] = "0", "1"
    try:
        return m.BiogptModel.load(path)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def calls(m, path, a):
    rng = np.random.default_rng(5)
    V = BASE["n_vocab"]
    prompts = [[2] + [int(v) for v in rng.integers(4, V, N_PROMPT - 1)] for _ in range(8)]
    long_prompt = [2] + [int(v) for v in rng.integers(4, V, 511)]
    simd, five, shipped = m.BiogptModel.load(path, assoc="simd"), load_five_launch(m, path), m.BiogptModel.load(path)
    ctxs = (("simd", simd), ("scalar_five", five), ("scalar", shipped))
    res = {"decode": {}, "prompt": {}}
    ts = alternating([lambda g=g: g.generate_greedy(prompts[0], N_GEN) for _, g in ctxs], a.reps, a.warmup)
    for (name, _), t in zip(ctxs, ts):
        res["decode"][name] = stats(t, N_GEN)
    ts = alternating([lambda g=g: g.eval_prompt(long_prompt, 0, 8) for _, g in ctxs], a.reps, a.warmup)
    for (name, _), t in zip(ctxs, ts):
        res["prompt"][name] = stats(t, 512)
    res["decode"]["simd_over_scalar_five"] = round(res["decode"]["simd"]["ms"] / res["decode"]["scalar_five"]["ms"], 3)
    res["prompt"]["simd_over_scalar_five"] = round(res["prompt"]["simd"]["ms"] / res["prompt"]["scalar_five"]["ms"], 3)
    div = []
    for p in prompts:
        i0, i1 = shipped.generate_greedy(p, N_GEN)[0], simd.generate_greedy(p, N_GEN)[0]
        ne = np.nonzero(np.asarray(i0) != np.asarray(i1))[0]
        div.append(int(ne[0]) if ne.size else -1)
    res["diverge"] = div
    for _, g in ctxs:
        g.close()
    if not a.skip_oracle:
        from oracle import oracle as O
        O.build()
        o = O.OracleModel(path, n_threads=16, assoc=7 if O.have_avx2() else 3)
        t = []
        for i in range(1 + 3):
            t0 = time.perf_counter()
            o.generate_greedy(prompts[0], N_GEN)
            if i >= 1:
                t.append((time.perf_counter() - t0) * 1e3)
        res["decode"]["oracle_avx2" if O.have_avx2() else "oracle_simd_emulation"] = stats(t, N_GEN)
        o.close()
    return res


def kernels(m, wtype, a):
    out = {}
    med = lambda us: round(float(np.median(us)), 2)
    for site, K, M in SITES:
        for N in (1, 8):
            s, y = med(m.assoc_bench("simd", wtype, M, K, N, a.reps)), med(m.assoc_bench("scalar", wtype, M, K, N, a.reps))
            out["%s_N%d" % (site, N)] = dict(simd_us=s, scalar_us=y, ratio=round(s / y, 3))
    for T in (64, 256, 1024):
        out["attn_T%d" % T] = dict(simd_us=med(m.assoc_bench("attn", wtype, 16, T, 1, a.reps)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--types", default="q4_0,q5_1,q8_0")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-oracle", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "assoc_bench", "model": "synthetic BioGPT-base sizes, %d layers" % a.layers, "reps": a.reps, "warmup": a.warmup}
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
