#!/usr/bin/env python3
"""Shared-prefix scoring on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): biogpt_hip_score_continuations against
biogpt_hip_score_batch of the concatenations [prefix + c for c in continuations], milliseconds per call by host wall clock (every call
returns after its stream has drained), warm-up 2, median of 7 with min - max.  Shapes (n_prefix, n_conts, len):

  384x3x2     a PubMedQA-shaped prompt with yes / no / maybe        384x64x8    reranking 64 hypotheses of one prompt
  64x64x8     the same behind a short prefix                         384x1x8     one candidate: only the prefix's lm_head rows are saved

The yardstick is timed on ANOTHER build of the library (`--yardstick-lib`, e.g. the parent commit's libbiogpt_hip.so, loaded through
BIOGPT_HIP_LIB), never on the code under test.  Each side runs in a process of its own; `--rounds` rounds alternate the two.  Per shape the
JSON line holds both sides' median / min / max over all rounds, the column counts of both routes, the ratio, and `beyond_spreads`: the
difference of the medians minus the two min - max spreads combined (positive: the new call is faster by more than both spreads).  Without
--yardstick-lib the score_batch of this build is timed instead and labelled so.

  python tools/prefix_bench.py [--reps 7] [--warmup 2] [--rounds 3] [--yardstick-lib PATH] [--only 384x64x8]
                               (--only: one shape of this build in this process, e.g. under a kernel trace)
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
SHAPES = [(384, 3, 2), (384, 64, 8), (64, 64, 8), (384, 1, 8)]


def key(shape):
    return "%dx%dx%d" % shape


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def inputs(shape, n_vocab):
    n_prefix, n_conts, n = shape
    rng = np.random.default_rng(n_prefix * 1000 + n_conts)
    prefix = [2] + [int(v) for v in rng.integers(4, n_vocab, n_prefix - 1)]
    conts = [[int(v) for v in rng.integers(4, n_vocab, n)] for _ in range(n_conts)]
    return prefix, conts


def measure(role, model, reps, warmup, only=""):
    """One side's timings in THIS process, with whatever library BIOGPT_HIP_LIB names (default: this build's)."""
    import _pkg
    m = _pkg.load()
    raw = ctypes.CDLL(m.LIB_PATH)
    m.SYMBOLS[:] = [s for s in m.SYMBOLS if hasattr(raw, s[0])]      # (an older build exports fewer symbols)
    g = m.BiogptModel.load(model)
    res = {"lib": m.LIB_PATH}
    for shape in SHAPES:
        if only and only != key(shape):
            continue
        prefix, conts = inputs(shape, g.n_vocab)
        if role == "yardstick":
            seqs = [prefix + c for c in conts]
            res[key(shape)] = timed(lambda: g.score_batch(seqs), reps, warmup)
        else:
            res[key(shape)] = timed(lambda: g.score_continuations(prefix, conts), reps, warmup)
    g.close()
    return res


def child(role, model, a, lib):
    env = dict(os.environ)
    if lib:
        env["BIOGPT_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("BIOGPT_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", role, "--model", model, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                         env=env, stdout=subprocess.PIPE, timeout=900, check=True).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def summary(rounds, k):
    meds = [round(float(np.median(r[k])), 4) for r in rounds]
    ts = [t for r in rounds for t in r[k]]
    return dict(ms=round(float(np.median(ts)), 4), min=round(min(ts), 4), max=round(max(ts), 4), round_medians=meds, n=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
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
    res = {"metric": "prefix_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds,
           "yardstick": os.path.abspath(a.yardstick_lib) if a.yardstick_lib else "this build (not another build: no acceptance figure)"}
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        if a.only:
            ts = measure("prefix", q40, a.reps, a.warmup, a.only)[a.only]
            res[a.only] = dict(ms=round(float(np.median(ts)), 4), min=round(min(ts), 4), max=round(max(ts), 4), n=len(ts))
            print(json.dumps(res))
            return
        ys, ps = [], []
        for _ in range(a.rounds):      # alternate the two builds
            ys.append(child("yardstick", q40, a, a.yardstick_lib))
            ps.append(child("prefix", q40, a, ""))
    for shape in SHAPES:
        n_prefix, n_conts, n = shape
        k = key(shape)
        new, old = summary(ps, k), summary(ys, k)
        res[k] = {"score_continuations": new, "score_batch_of_concatenations": old,
                  "columns": {"score_continuations": n_prefix - 1 + n_conts * n, "score_batch": n_conts * (n_prefix + n)},
                  "ratio": round(new["ms"] / old["ms"], 4),
                  "beyond_spreads": round((old["ms"] - new["ms"]) - ((old["max"] - old["min"]) + (new["max"] - new["min"])), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
