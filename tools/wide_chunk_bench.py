#!/usr/bin/env python3
"""The wide chunk layer (biogpt_hip_wide_chunk) on synthetic files at BioGPT-Large's sizes (d_model 1600, d_ff 6400, 25 heads, n_vocab 57717, 1024 positions),
Q4_0 / Q5_1 / Q8_0: host wall clock around calls that return after their stream has drained, warm-up 2, median of 9 (min - max), the two routes of a row
alternating in one process.  The yardstick of every row is the generic route of the same build: the same file in a context with the switch off (both contexts
have the wide decode layer on, as new contexts do; --generic-first loads that context first).  Prints one JSON line.

  eval8_at_T      one biogpt_eval of 8 tokens ending at T = 40, 230, 600, 1000 keys (behind a prompt evaluated once, outside the clock)
  eval2_at_230, eval5_at_230   likewise 2 and 5 tokens
  loop_512        the reference's prompt loop: 64 evals of 8 tokens from position 0
  greedy_64+64    generate_greedy of a 64-token prompt + 64 new tokens (its prompt travels as ONE pass of 64 columns: neither route's chunk launches)
  stages          each linear stage alone at 8 columns by device events through the probe's timing loop, at (K, M) = (1600, 4800) q/k/v, (1600, 1600)
                  out_proj, (1600, 6400) fc1, (6400, 1600) fc2 (the two LayerNorm + Q8 producer launches have no probe of their own: they are inside the calls)

  python tools/wide_chunk_bench.py [--layers 48] [--types q4_0,q5_1,q8_0] [--reps 9] [--warmup 2] [--skip-stages] [--skip-calls] [--generic-first]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.join(ROOT, "tools"))
from wide_decode_bench import BLOCK_BYTES, KEYS, LARGE, SEED, STAGES, WTYPES, alternating, stats      # noqa: E402


def row(chunk, generic, per=None):
    r = dict(chunk=stats(chunk), generic=stats(generic))
    r["chunk_over_generic"] = round(r["chunk"]["ms"] / r["generic"]["ms"], 3)
    r["verdict"] = "win" if r["chunk_over_generic"] < 1.0 else "LOSS"
    if per:
        r["chunk_us_per_layer"], r["generic_us_per_layer"] = (round(r[k]["ms"] * 1e3 / per, 2) for k in ("chunk", "generic"))
    return r


def calls(m, path, a):
    rng = np.random.default_rng(5)
    toks = [2] + [int(v) for v in rng.integers(4, LARGE["n_vocab"], 1023)]
    if a.generic_first:      # (which context is loaded first: a row whose two sides enqueue the same launches shows what the load order alone is worth)
        gen = m.BiogptModel.load(path, wide_chunk=False)
        new = m.BiogptModel.load(path, wide_chunk=True)
    else:
        new, gen = m.BiogptModel.load(path, wide_chunk=True), m.BiogptModel.load(path, wide_chunk=False)
    res = {}
    for n, T in [(8, T) for T in KEYS] + [(2, 230), (5, 230)]:
        for g in (new, gen):
            g.eval_prompt(toks[:T - n], 0, 8)
        tn, tg = alternating([lambda: new.eval(toks[T - n:T], T - n), lambda: gen.eval(toks[T - n:T], T - n)], a.reps, a.warmup)
        res["eval%d_at_%d" % (n, T)] = row(tn, tg, a.layers)      # (embedding, lm_head and the row's copy are inside: the same launches on both sides)

    def loop(g):
        for at in range(0, 512, 8):
            g.eval(toks[at:at + 8], at)
    tn, tg = alternating([lambda: loop(new), lambda: loop(gen)], a.reps, a.warmup)
    res["loop_512"] = row(tn, tg, 64 * a.layers)
    tn, tg = alternating([lambda: new.generate_greedy(toks[:64], 64), lambda: gen.generate_greedy(toks[:64], 64)], a.reps, a.warmup)
    res["greedy_64+64"] = row(tn, tg)
    res["chunk_launches"] = new.wide_chunk_launches()
    new.close(); gen.close()
    return res


def stages(m, wtype, a, N=8):
    out = {}
    for name, K, M in STAGES:
        z = dict(w_rows=np.full(M * (K // 32) * BLOCK_BYTES[wtype], 0x11, np.uint8), bias=np.zeros(M, np.float32), reps=a.reps,
                 aq=(np.ones((N, K), np.int8), np.ones((N, K // 32), np.float32), np.full((N, K // 32), 32, np.uint32)))
        if name in ("OPROJ", "FC2"):
            z.update(resid=np.zeros((N, M), np.float32))
        if name == "QKV":
            z.update(k_cache=np.zeros((K // 64, 16, 64), np.float32), v_cache=np.zeros((K // 64, 16, 64), np.float32), P=16, n_past=1)
        got = m.wchunk_device(name, wtype, M, K, N, **z)
        out[name] = dict(chunk_us=round(float(np.median(got["us"])), 2), threads=int(got["launched"][0]), grid=int(got["launched"][1]), lds=int(got["launched"][2]),
                         rows=int(got["launched"][3]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--types", default="q4_0,q5_1,q8_0")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-stages", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--generic-first", action="store_true")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.lib()
    res = {"metric": "wide_chunk_bench", "model": "synthetic BioGPT-Large sizes, %d layers, %d positions" % (a.layers, LARGE["n_positions"]), "reps": a.reps,
           "warmup": a.warmup}
    with tempfile.TemporaryDirectory() as td:
        f32 = os.path.join(td, "f32.bin")
        if not a.skip_calls:
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **LARGE)
        for name in a.types.split(","):
            print("wide_chunk_bench: %s" % name, file=sys.stderr, flush=True)
            res[name] = {}
            if not a.skip_stages:
                res[name]["stages_8_columns"] = stages(m, WTYPES[name], a)
            if not a.skip_calls:
                path = os.path.join(td, name + ".bin")
                m.quantize_file(f32, path, name)
                res[name].update(calls(m, path, a))
                os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
