#!/usr/bin/env python3
"""The float chain on synthetic 24-layer BioGPT-base files, F32 and F16 (d_model 1024, d_ff 4096, 16 heads, n_vocab 42384): milliseconds per call by host wall
clock (every call returns after its stream has drained), warm-up 2, median of 9 (min - max), the two routes of a row alternating.  Prints one JSON line:

  score_batch_64x64      biogpt_hip_score_batch of 64 sequences x 64 tokens, float chain on    against the loop of 64 biogpt_hip_score calls
  greedy_batch_Nx64      biogpt_hip_generate_greedy_batch, N = 8 / 64 / 256 prompts x 64 tokens against the loop of N biogpt_hip_generate_greedy calls
                         (256: --loop256-reps repeats behind one warm-up -- 16384 single-token passes each)
  stage                  fchain_kernel alone (device events, residual epilogue) per site -- q/k/v, out_proj, fc1, fc2, lm_head -- at N = 8 / 64 / 256: microseconds
                         at the launch's own tile shape and at each of the three (the sweep behind bg_fchain_cfg), and the generic matvec_kernel of a prompt pass
                         at the same shape; `floor_us` is the issue's derived floor, 26 us per column and 345 M MACs, scaled to the site's MACs.

The loops and the generic kernel are unchanged functions of the same build, on a context of the same file WITHOUT the switch.  A row where the batched route
loses shows ratio > 1.

  python tools/float_chain_bench.py [--layers 24] [--types f32,f16] [--reps 9] [--warmup 2] [--loop256-reps 3] [--skip-calls] [--skip-stage]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 0x42494F47
BASE = dict(n_vocab=42384, n_head=16, n_positions=1024, d_ff=4096, d_model=1024, n_merges=40000)
SITES = (("qkv", 1024, 3072), ("out_proj", 1024, 1024), ("fc1", 1024, 4096), ("fc2", 4096, 1024), ("lm_head", 1024, 42384))
FLOOR_US_PER_MAC = 26.0 / 345e6      # the issue's figure: 3 VALU operations a MAC on the whole chip at 2.4 GHz, f64 adds at full rate (not confirmed)


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


def f16_file(f32, f16):
    """convert.py --use-f16: the 2-D "*.weight" tensors as float16, ftype 1"""
    from modelfile_py import read_model, write_model
    hp, vocab, merges, tensors = read_model(f32)
    for t in tensors:
        if len(t["ne"]) == 2 and t["name"].endswith(".weight") and t["type"] == 0:
            t["raw"] = np.frombuffer(t["raw"], dtype=np.float32).astype(np.float16).tobytes()
            t["type"] = 1
    write_model(f16, dict(hp, ftype=1), vocab, merges, tensors)


def calls(m, path, a):
    g = m.BiogptModel.load(path, float_chain=True)      # the batched calls
    y = m.BiogptModel.load(path)                        # the yardstick: the same file without the switch
    rng = np.random.default_rng(5)
    V = BASE["n_vocab"]
    seqs = [[2] + [int(v) for v in rng.integers(4, V, 63)] for _ in range(64)]
    prompts = [[2] + [int(v) for v in rng.integers(4, V, 7)] for _ in range(256)]
    res = {}
    b, l = alternating(lambda: g.score_batch(seqs), lambda: [y.score(s) for s in seqs], a.reps, a.warmup)
    res["score_batch_64x64"] = row(b, l, 64 * 64)
    for n, reps, warm in ((8, a.reps, a.warmup), (64, a.reps, a.warmup), (256, a.loop256_reps, 1)):
        b, l = alternating(lambda: g.generate_greedy_batch(prompts[:n], 64), lambda: [y.generate_greedy(p, 64) for p in prompts[:n]], reps, warm)
        res["greedy_batch_%dx64" % n] = row(b, l, n * 64)
    res["chain_kind"], res["float_launches"], res["yardstick_chain_kind"] = g.chain_kind(), g.float_launches(), y.chain_kind()
    g.close()
    y.close()
    return res


def stage(m, wtype, a):
    out = {}
    for site, K, M in SITES:
        for N in (8, 64, 256):
            med = lambda us: round(float(np.median(us)), 2)
            r = dict(auto_us=med(m.fchain_bench("float", wtype, M, K, N, -1, a.reps)), generic_us=med(m.fchain_bench("generic", wtype, M, K, N, -1, a.reps)),
                     floor_us=round(FLOOR_US_PER_MAC * M * K * N, 2))
            for cfg in (0, 1, 2):
                r["cfg%d_us" % cfg] = med(m.fchain_bench("float", wtype, M, K, N, cfg, a.reps))
            out["%s_N%d" % (site, N)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--types", default="f32,f16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop256-reps", type=int, default=3)
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--skip-stage", action="store_true")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "float_chain_bench", "model": "synthetic BioGPT-base sizes, %d layers" % a.layers, "reps": a.reps, "warmup": a.warmup, "loop256_reps": a.loop256_reps}
    with tempfile.TemporaryDirectory() as td:
        f32, f16 = os.path.join(td, "f32.bin"), os.path.join(td, "f16.bin")
        if not a.skip_calls:
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **BASE)
        for name in a.types.split(","):
            wtype = {"f32": 0, "f16": 1}[name]
            res[name] = {}
            if not a.skip_stage:
                res[name]["stage"] = stage(m, wtype, a)
            if not a.skip_calls:
                if name == "f16":
                    f16_file(f32, f16)
                res[name].update(calls(m, f16 if name == "f16" else f32, a))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
