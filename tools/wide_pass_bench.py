#!/usr/bin/env python3
"""The wide pass layer (biogpt_hip_wide_pass) on synthetic files at BioGPT-Large's sizes (d_model 1600, d_ff 6400, 25 heads, n_vocab 57717, 1024 positions),
Q4_0 / Q5_1 / Q8_0: host wall clock around calls that return after their stream has drained, warm-up 2, median of 9 (min - max), the two routes of a row
alternating in one process.  The yardstick of every row is the generic route of the same build: the same file in a context with the switch off (both contexts
have the wide decode and chunk layers on, as new contexts do).  Prints one JSON line.

  eval16 / eval64 / eval256 / eval512    one biogpt_eval of that many tokens at n_past 0
  eval64_at_448                          one biogpt_eval of 64 tokens behind 448 (evaluated once, outside the clock)
  score64 / score512                     one score call of that many tokens
  greedy_64+64                           generate_greedy of a 64-token prompt + 64 new tokens
  prompt512 / loop8_512                  eval_prompt of 512 tokens (both routes), and the reference's loop of 64 evals of 8 tokens in the switch-on context
  stages                                 each site of the new kernel alone against matmul_wide_kernel on the same image and columns, by device events through the
                                         probe's timing loop, at (K, M) = (1600, 4800) q/k/v, (1600, 1600) out_proj, (1600, 6400) fc1, (6400, 1600) fc2 and N = 16 /
                                         64 / 512 columns (the wide chain's fc1 is timed without the q8_rows_kernel launch it needs behind it)

  python tools/wide_pass_bench.py [--layers 48] [--types q4_0,q5_1,q8_0] [--reps 9] [--warmup 2] [--skip-stages] [--skip-calls]
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
from wide_decode_bench import BLOCK_BYTES, LARGE, SEED, STAGES, WTYPES, alternating, stats      # noqa: E402

SITES = {"QKV": "QKV", "OPROJ": "RESID", "FC1": "FC1", "FC2": "RESID"}


def row(new, generic):
    r = dict(wide_pass=stats(new), generic=stats(generic))
    r["pass_over_generic"] = round(r["wide_pass"]["ms"] / r["generic"]["ms"], 3)
    r["verdict"] = "win" if r["pass_over_generic"] < 1.0 else "LOSS"
    return r


def calls(m, path, a):
    rng = np.random.default_rng(5)
    toks = [2] + [int(v) for v in rng.integers(4, LARGE["n_vocab"], 1023)]
    new, gen = m.BiogptModel.load(path, wide_pass=True), m.BiogptModel.load(path, wide_pass=False)
    res = {}
    both = lambda f: alternating([lambda: f(new), lambda: f(gen)], a.reps, a.warmup)
    for n in (16, 64, 256, 512):
        res["eval%d" % n] = row(*both(lambda g: g.eval(toks[:n], 0)))
    for g in (new, gen):
        g.eval(toks[:448], 0)
    res["eval64_at_448"] = row(*both(lambda g: g.eval(toks[448:512], 448)))
    for n in (64, 512):
        res["score%d" % n] = row(*both(lambda g: g.score(toks[:n], 0)))
    res["greedy_64+64"] = row(*both(lambda g: g.generate_greedy(toks[:64], 64)))
    res["prompt512"] = row(*both(lambda g: g.eval_prompt(toks[:512], 0, 8)))

    def loop(g):
        for at in range(0, 512, 8):
            g.eval(toks[at:at + 8], at)
    res["loop8_512"] = stats(alternating([lambda: loop(new)], a.reps, a.warmup)[0])
    res["pass_launches"] = new.wide_pass_launches()
    new.close(); gen.close()
    return res


def stages(m, wtype, a):
    out = {}
    for name, K, M in STAGES:
        for N in (16, 64, 512):
            z = dict(w_rows=np.full(M * (K // 32) * BLOCK_BYTES[wtype], 0x11, np.uint8), bias=np.zeros(M, np.float32), reps=a.reps,
                     aq=(np.ones((N, K), np.int8), np.ones((N, K // 32), np.float32), np.full((N, K // 32), 32, np.uint32)))
            if SITES[name] == "RESID":
                z.update(resid=np.zeros((N, M), np.float32))
            if name == "QKV":
                z.update(k_cache=np.zeros((K // 64, N + 2, 64), np.float32), v_cache=np.zeros((K // 64, N + 2, 64), np.float32), P=N + 2, n_past=1)
            new, old = (m.wpass_device(SITES[name], wtype, M, K, N, which=w, **z) for w in (0, 1))
            r = dict(pass_us=round(float(np.median(new["us"])), 2), wide_chain_us=round(float(np.median(old["us"])), 2), launched=[int(v) for v in new["launched"][:5]])
            r["pass_over_wide_chain"] = round(r["pass_us"] / r["wide_chain_us"], 3)
            r["verdict"] = "win" if r["pass_over_wide_chain"] < 1.0 else "LOSS"
            out["%s_N%d" % (name, N)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--types", default="q4_0,q5_1,q8_0")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-stages", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.lib()
    res = {"metric": "wide_pass_bench", "model": "synthetic BioGPT-Large sizes, %d layers, %d positions" % (a.layers, LARGE["n_positions"]), "reps": a.reps,
           "warmup": a.warmup}
    with tempfile.TemporaryDirectory() as td:
        f32 = os.path.join(td, "f32.bin")
        if not a.skip_calls:
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **LARGE)
        for name in a.types.split(","):
            print("wide_pass_bench: %s" % name, file=sys.stderr, flush=True)
            res[name] = {}
            if not a.skip_stages:
                res[name]["stages"] = stages(m, WTYPES[name], a)
            if not a.skip_calls:
                path = os.path.join(td, name + ".bin")
                m.quantize_file(f32, path, name)
                res[name].update(calls(m, path, a))
                os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
