#!/usr/bin/env python3
"""Sequence scoring on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per call by host wall clock
(every call below returns after its stream has drained), after a warm-up, `--reps` repeats (median, min, max).  Prints one JSON line:

  score_512 / score_1024      biogpt_hip_score of 512 / 1024 tokens, and eval_prompt(same tokens, 0, n_batch = 1) in the same process
  old_route_512              BIOGPT_HIP_CAUSAL=1 + eval_all + numpy log-softmax (what scoring took before biogpt_hip_score)
  score_batch_64x64          biogpt_hip_score_batch of 64 sequences x 64 tokens, against a loop of 64 score calls

  python tools/score_bench.py [--reps 20] [--warmup 3] [--only score_512]    (--only: one measurement, e.g. under a kernel trace)
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


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(float(np.median(ts)), 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4), n=reps)


def log_softmax_rows(rows, targets):
    r = rows.astype(np.float64)
    m = r.max(axis=1, keepdims=True)
    lse = np.log(np.exp(r - m).sum(axis=1)) + m[:, 0]
    return (r[np.arange(len(targets)), targets] - lse).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "score_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "reps": a.reps, "warmup": a.warmup}
    want = lambda k: not a.only or a.only == k
    rng = np.random.default_rng(5)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        for n in (512, 1024):
            key = "score_%d" % n
            if not want(key):
                continue
            toks = [2] + [int(v) for v in rng.integers(4, g.n_vocab, n - 1)]
            sc = timed(lambda: g.score(toks), a.reps, a.warmup)
            ep = timed(lambda: g.eval_prompt(toks, 0, 1), a.reps, a.warmup) if not a.only else None
            res[key] = dict(score=sc, tok_s=round(n / sc["ms"] * 1e3))
            if ep:
                res[key].update(eval_prompt_b1=ep, ratio=round(sc["ms"] / ep["ms"], 4))
        if want("score_batch_64x64"):
            seqs = [[2] + [int(v) for v in rng.integers(4, g.n_vocab, 63)] for _ in range(64)]
            sb = timed(lambda: g.score_batch(seqs), a.reps, a.warmup)
            lp = timed(lambda: [g.score(s) for s in seqs], max(3, a.reps // 4), 1) if not a.only else None
            res["score_batch_64x64"] = dict(score_batch=sb, tok_s=round(64 * 64 / sb["ms"] * 1e3))
            if lp:
                res["score_batch_64x64"].update(score_loop=lp, loop_tok_s=round(64 * 64 / lp["ms"] * 1e3), ratio=round(lp["ms"] / sb["ms"], 3))
        g.close()
        if want("old_route_512"):
            os.environ["BIOGPT_HIP_CAUSAL"] = "1"     # read when the context is created
            h = m.BiogptModel.load(q40)
            del os.environ["BIOGPT_HIP_CAUSAL"]
            toks = [2] + [int(v) for v in rng.integers(4, h.n_vocab, 511)]
            tg = np.asarray(toks[1:], dtype=np.int64)
            old = timed(lambda: log_softmax_rows(h.eval_all(toks, 0)[:-1], tg), max(5, a.reps // 2), 1)
            res["old_route_512"] = dict(eval_all_numpy=old)
            if "score_512" in res:
                res["old_route_512"]["score_speedup"] = round(old["ms"] / res["score_512"]["score"]["ms"], 2)
            h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
