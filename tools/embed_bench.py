#!/usr/bin/env python3
"""Hidden states and embeddings on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per call by host wall clock
(every call returns after its stream has drained), after a warm-up, `--reps` repeats (median, min, max).  Prints one JSON line:

  embed_mean_64x64      biogpt_hip_embed_batch(pooling = mean) of 64 sequences x 64 tokens       yardstick: biogpt_hip_score_batch of the same sequences
  hidden_512            biogpt_hip_hidden of one 512-token sequence                              yardstick: biogpt_hip_score of the same tokens
  embed_layer12_64x64   embed_batch(layer = 12, last token) of the 64 x 64 input                 against embed_layer24_64x64, the same call over all layers
  (embed_head7_64x64, embed_rows_64x64: mean + a 7-row head; no pooling -- what the head and a 16 MB copy back add)

The yardsticks are timed on ANOTHER build of the library (`--yardstick-lib`, e.g. the parent commit's libbiogpt_hip.so, loaded through
BIOGPT_HIP_LIB), not on the code under test.  Each side runs in a process of its own; `--rounds` rounds alternate the two, and the spread of
the per-round medians is reported beside each ratio.  Without --yardstick-lib the scoring calls of this build are timed instead and labelled so.

  python tools/embed_bench.py [--reps 15] [--warmup 3] [--rounds 3] [--yardstick-lib PATH] [--only embed_mean_64x64]
                              (--only: one measurement of this build in this process, e.g. under a kernel trace)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 0x42494F47
EMBED_KEYS = ["embed_mean_64x64", "hidden_512", "embed_layer12_64x64", "embed_layer24_64x64", "embed_head7_64x64", "embed_rows_64x64"]
PAIRS = {"embed_mean_64x64": "score_batch_64x64", "hidden_512": "score_512"}      # measurement -> its yardstick


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(float(np.median(ts)), 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4), n=reps)


def inputs(n_vocab):
    rng = np.random.default_rng(5)
    seqs = [[2] + [int(v) for v in rng.integers(4, n_vocab, 63)] for _ in range(64)]
    toks = [2] + [int(v) for v in rng.integers(4, n_vocab, 511)]
    return seqs, toks


def measure(role, model, reps, warmup, only=""):
    """One side's timings in THIS process, with whatever library BIOGPT_HIP_LIB names (default: this build's)."""
    import _pkg
    m = _pkg.load()
    raw = ctypes.CDLL(m.LIB_PATH)
    m.SYMBOLS[:] = [s for s in m.SYMBOLS if hasattr(raw, s[0])]      # (an older build exports fewer symbols)
    g = m.BiogptModel.load(model)
    seqs, toks = inputs(g.n_vocab)
    want = lambda k: not only or only == k
    res = {"lib": m.LIB_PATH}
    if role == "yardstick":
        if want("score_batch_64x64"):
            res["score_batch_64x64"] = timed(lambda: g.score_batch(seqs), reps, warmup)
        if want("score_512"):
            res["score_512"] = timed(lambda: g.score(toks), reps, warmup)
    else:
        W = np.random.default_rng(6).normal(0.0, 0.05, (7, 1024)).astype(np.float32)
        calls = {"embed_mean_64x64": lambda: g.embed_batch(seqs, pooling="mean"),
                 "hidden_512": lambda: g.hidden(toks),
                 "embed_layer12_64x64": lambda: g.embed_batch(seqs, layer=12),
                 "embed_layer24_64x64": lambda: g.embed_batch(seqs, layer=24),
                 "embed_head7_64x64": lambda: g.embed_batch(seqs, pooling="mean", head=W),
                 "embed_rows_64x64": lambda: g.embed_batch(seqs, pooling="none")}
        for k in EMBED_KEYS:
            if want(k):
                res[k] = timed(calls[k], reps, warmup)
    g.close()
    return res


def child(role, model, a, lib):
    env = dict(os.environ)
    if lib:
        env["BIOGPT_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("BIOGPT_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", role, "--model", model, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                         env=env, stdout=subprocess.PIPE, timeout=600, check=True).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def summary(rounds, key):
    meds = [r[key]["ms"] for r in rounds]
    return dict(ms=round(float(np.median(meds)), 4), round_medians=meds, min=min(r[key]["min"] for r in rounds), max=max(r[key]["max"] for r in rounds),
                spread=round((max(meds) - min(meds)) / float(np.median(meds)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--yardstick-lib", default="")
    ap.add_argument("--only", default="")
    ap.add_argument("--role", default="")      # internal: one side's timings of a given model file
    ap.add_argument("--model", default="")
    a = ap.parse_args()
    if a.role:
        print(json.dumps(measure(a.role, a.model, a.reps, a.warmup)))
        return
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "embed_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds,
           "yardstick": os.path.abspath(a.yardstick_lib) if a.yardstick_lib else "this build (not another build: no acceptance figure)"}
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        if a.only:
            res[a.only] = measure("embed", q40, a.reps, a.warmup, a.only)[a.only]
            print(json.dumps(res))
            return
        ys, es = [], []
        for _ in range(a.rounds):      # alternate the two builds
            ys.append(child("yardstick", q40, a, a.yardstick_lib))
            es.append(child("embed", q40, a, ""))
    for k in ("score_batch_64x64", "score_512"):
        res[k] = summary(ys, k)
    for k in EMBED_KEYS:
        res[k] = summary(es, k)
    for k, y in PAIRS.items():
        res[k]["yardstick"] = y
        res[k]["ratio"] = round(res[k]["ms"] / res[y]["ms"], 4)
        res[k]["ratio_by_round"] = [round(e[k]["ms"] / r[y]["ms"], 4) for e, r in zip(es, ys)]
    res["embed_mean_64x64"]["tok_s"] = round(64 * 64 / res["embed_mean_64x64"]["ms"] * 1e3)
    res["hidden_512"]["tok_s"] = round(512 / res["hidden_512"]["ms"] * 1e3)
    res["embed_layer12_64x64"]["ratio_to_layer24"] = round(res["embed_layer12_64x64"]["ms"] / res["embed_layer24_64x64"]["ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
