#!/usr/bin/env python3
"""The wide decode layer (biogpt_hip_wide_decode) on synthetic files at BioGPT-Large's sizes (d_model 1600, d_ff 6400, 25 heads, n_vocab 57717, 1024
positions), Q4_0 / Q5_1 / Q8_0: host wall clock around calls that return after their stream has drained, warm-up 2, median of 9 (min - max), the two routes
of a row alternating in one process.  The yardstick of every row is the generic route of the same build: the same file in a context with the switch off.
(Against another build: run the tool in both and compare the "generic" columns and the "wide" column across the two JSON lines.)  Prints one JSON line.

  greedy_16+200   generate_greedy of a 16-token prompt + 200 new tokens (captured steps)
  eval_loop       biogpt_eval per token: 64 single-token evals behind a 16-token prompt
  layer_at_T      one single-token eval at T = 40, 230, 600, 1000 keys (behind a prompt evaluated once, outside the clock), per layer
  stages          each kernel alone by device events through the probe's timing loop, at (K, M) = (1600, 4800) q/k/v, (1600, 1600) out_proj, (1600, 6400)
                  fc1, (6400, 1600) fc2, against matvec_kernel<PLAIN, RESID> at the same shape (which leaves out the LayerNorm and Q8 prologue the generic
                  route's q/k/v, fc1 and fc2 launches pay on top: the comparison flatters the yardstick)

  python tools/wide_decode_bench.py [--layers 48] [--types q4_0,q5_1,q8_0] [--reps 9] [--warmup 2] [--skip-stages] [--skip-calls]
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
WTYPES = {"q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8}
BLOCK_BYTES = {2: 18, 3: 20, 6: 22, 7: 24, 8: 34}
STAGES = (("QKV", 1600, 4800), ("OPROJ", 1600, 1600), ("FC1", 1600, 6400), ("FC2", 6400, 1600))
KEYS = (40, 230, 600, 1000)


def stats(ts):
    ts = np.asarray(ts)
    return dict(ms=round(float(np.median(ts)), 3), min=round(float(ts.min()), 3), max=round(float(ts.max()), 3), n=int(ts.size))


def alternating(fns, reps, warmup):
    ts = [[] for _ in fns]
    for i in range(warmup + reps):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                t.append((time.perf_counter() - t0) * 1e3)
    return ts


def row(wide, generic, per=None):
    r = dict(wide=stats(wide), generic=stats(generic))
    r["wide_over_generic"] = round(r["wide"]["ms"] / r["generic"]["ms"], 3)
    r["verdict"] = "win" if r["wide_over_generic"] < 1.0 else "LOSS"
    if per:
        r["wide_us_per_layer"], r["generic_us_per_layer"] = (round(r[k]["ms"] * 1e3 / per, 2) for k in ("wide", "generic"))
    return r


def calls(m, path, a):
    rng = np.random.default_rng(5)
    toks = [2] + [int(v) for v in rng.integers(4, LARGE["n_vocab"], 1023)]
    wide, gen = m.BiogptModel.load(path, wide_decode=True), m.BiogptModel.load(path, wide_decode=False)
    res = {}
    tw, tg = alternating([lambda: wide.generate_greedy(toks[:16], 200), lambda: gen.generate_greedy(toks[:16], 200)], a.reps, a.warmup)
    res["greedy_16+200"] = row(tw, tg, 200 * a.layers)

    def loop(g):
        g.eval(toks[:16], 0)
        for i in range(64):
            g.eval([toks[16 + i]], 16 + i)
    tw, tg = alternating([lambda: loop(wide), lambda: loop(gen)], a.reps, a.warmup)
    res["eval_loop_16+64"] = row(tw, tg, 64 * a.layers)      # (the prompt eval is inside: the same launches on both sides)
    for T in KEYS:
        for g in (wide, gen):
            g.eval_prompt(toks[:T - 1], 0, 8)
        tw, tg = alternating([lambda: wide.eval([toks[T - 1]], T - 1), lambda: gen.eval([toks[T - 1]], T - 1)], a.reps, a.warmup)
        res["layer_at_%d" % T] = row(tw, tg, a.layers)      # (embedding, lm_head and the row's copy are inside: the same launches on both sides)
    res["stage_launches"] = wide.wide_decode_launches()
    wide.close(); gen.close()
    return res


def stages(m, wtype, a):
    out = {}
    med = lambda us: round(float(np.median(us)), 2)
    for name, K, M in STAGES:
        z = dict(w_rows=np.full(M * (K // 32) * BLOCK_BYTES[wtype], 0x11, np.uint8), bias=np.zeros(M, np.float32), reps=a.reps)
        if name in ("QKV", "FC1"):
            z.update(x=np.linspace(-1, 1, K, dtype=np.float32), ln_w=np.ones(K, np.float32), ln_b=np.zeros(K, np.float32))
        else:
            z.update(aq=(np.ones(K, np.int8), np.ones(K // 32, np.float32), np.full(K // 32, 32, np.uint32)), resid=np.zeros(M, np.float32))
        if name == "QKV":
            z.update(k_cache=np.zeros((K // 64, 4, 64), np.float32), v_cache=np.zeros((K // 64, 4, 64), np.float32), P=4, n_past=1)
        got = m.wdecode_device(name, wtype, M, K, **z)
        r = dict(wide_us=med(got["us"]), threads=int(got["launched"][0]), grid=int(got["launched"][1]), lds=int(got["launched"][2]),
                 matvec_plain_resid_us=med(m.assoc_bench("scalar", wtype, M, K, 1, reps=a.reps)))
        r["wide_over_matvec"] = round(r["wide_us"] / r["matvec_plain_resid_us"], 3)
        out[name] = r
    for T in KEYS[:2]:
        H, P = 25, 1024
        got = m.wdecode_device("ATTN", wtype, H=H, P=P, n_past=T - 1, reps=a.reps, q=np.zeros(H * 64, np.float32), k_cache=np.zeros((H, P, 64), np.float32),
                               v_cache=np.zeros((H, P, 64), np.float32))
        out["ATTN_%d" % T] = dict(wide_us=med(got["us"]), lanes_per_key=int(got["launched"][2]))
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
    res = {"metric": "wide_decode_bench", "model": "synthetic BioGPT-Large sizes, %d layers, %d positions" % (a.layers, LARGE["n_positions"]), "reps": a.reps,
           "warmup": a.warmup}
    with tempfile.TemporaryDirectory() as td:
        f32 = os.path.join(td, "f32.bin")
        if not a.skip_calls:
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **LARGE)
        for name in a.types.split(","):
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
