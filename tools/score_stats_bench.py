#!/usr/bin/env python3
"""Scoring statistics and the comparison of two files on the synthetic 24-layer BioGPT-base model (bench.py's seed), 512 tokens: milliseconds per call
by host wall clock (every call returns after its streams have drained), warm-up 2, median of 9 (min - max), the routes of a case taking turns.
Prints one JSON line:

  rank_entropy   score(top=0, rank, entropy) of the Q4_0 file    against the unchanged score() of the same build
  top5           score(top=5)                                    against the same
  compare        compare(Q4_0, F16)                              against score() on the Q4_0 file + score() on the F16 file

  python tools/score_stats_bench.py [--reps 9] [--warmup 2] [--tokens 512]
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


def f16_file(f32, f16):
    """convert.py --use-f16: the 2-D "*.weight" tensors as float16, ftype 1"""
    from modelfile_py import read_model, write_model
    hp, vocab, merges, tensors = read_model(f32)
    for t in tensors:
        if len(t["ne"]) == 2 and t["name"].endswith(".weight") and t["type"] == 0:
            t["raw"] = np.frombuffer(t["raw"], dtype=np.float32).astype(np.float16).tobytes()
            t["type"] = 1
    write_model(f16, dict(hp, ftype=1), vocab, merges, tensors)


def alternating(routes, reps, warmup):
    """{name: dict(ms, min, max)}: every round runs each route once, in order."""
    ts = {name: [] for name in routes}
    for r in range(warmup + reps):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: dict(ms=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4)) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=512)
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "score_stats_bench", "model": "synthetic BioGPT-base, 24 layers", "tokens": a.tokens, "reps": a.reps, "warmup": a.warmup}
    with tempfile.TemporaryDirectory() as td:
        f32, q40, f16 = (os.path.join(td, n) for n in ("f32.bin", "q4_0.bin", "f16.bin"))
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        f16_file(f32, f16)
        os.remove(f32)
        g, h = m.BiogptModel.load(q40), m.BiogptModel.load(f16)
        rng = np.random.default_rng(5)
        toks = [2] + [int(v) for v in rng.integers(4, g.n_vocab, a.tokens - 1)]
        t = alternating({"score": lambda: g.score(toks), "rank_entropy": lambda: g.score(toks, top=0, rank=True, entropy=True),
                         "top5": lambda: g.score(toks, top=5)}, a.reps, a.warmup)
        res.update(t)
        for name in ("rank_entropy", "top5"):
            res[name]["ratio_to_score"] = round(t[name]["ms"] / t["score"]["ms"], 4)
        c = alternating({"score_q4_0": lambda: g.score(toks), "score_f16": lambda: h.score(toks), "compare": lambda: g.compare(h, toks)}, a.reps, a.warmup)
        res.update(c)
        res["compare"]["ratio_to_two_scores"] = round(c["compare"]["ms"] / (c["score_q4_0"]["ms"] + c["score_f16"]["ms"]), 4)
        out = g.compare(h, toks)
        res["compare"].update(mean_kl=float(out["kl"].mean()), top1_agreement=float((out["argmax"] == out["argmax_other"]).mean()))
        g.close()
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
