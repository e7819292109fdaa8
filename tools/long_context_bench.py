#!/usr/bin/env python3
"""The long-context attention (biogpt_hip_long_context) on synthetic files at BioGPT-Large's sizes (d_model 1600, d_ff 6400, 25 heads, n_vocab 57717) with the
2048-row position table a real conversion has, Q4_0 / Q5_1 / Q8_0: host wall clock around calls that return after their stream has drained, warm-up 2, median of
9 (min - max), the two routes of a row alternating in one process.  The yardstick of every row is the switch-off route of the same build: the same file in a
context with the switch off (both contexts have the wide decode, chunk and pass layers on, as new contexts do).  A row the new route loses says LOSS.  Prints one
JSON line.

  prompt2048 / prompt2048_by8    eval_prompt of 2048 tokens as one pass, and in chunks of 8
  eval64_at_1984                 one biogpt_eval of 64 tokens behind 1984 keys (evaluated once, outside the clock)
  eval8_at_1500                  one biogpt_eval of 8 tokens behind 1500 keys
  token_at_1100 / token_at_2040  one biogpt_eval of one token at that many keys
  greedy_1400+200                generate_greedy of a 1400-token prompt + 200 new tokens
  kernels                        by device events through the probes' timing loops (a repeated stand-alone launch finds its K / V rows in cache): each of the two
                                 kernels against attn_kernel on the same K / V at 1025 / 1536 / 2048 keys (25 heads; the column kernel at 1 and 8 columns, the tile
                                 kernel at 128), and the tile kernel against attn_tile_kernel at 1024 keys on 512 columns

  python tools/long_context_bench.py [--layers 48] [--types q4_0,q5_1,q8_0] [--reps 9] [--warmup 2] [--skip-kernels] [--skip-calls]
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
from wide_decode_bench import LARGE, SEED, alternating, stats      # noqa: E402

LARGE_2048 = dict(LARGE, n_positions=2048)
H, TILE, GENERIC = 25, 12, 13      # heads of Large; biogpt_hip_attn_device's routes attn_tile_kernel<16, false> and attn_kernel


def row(new, old):
    r = dict(long_context=stats(new), off=stats(old))
    r["on_over_off"] = round(r["long_context"]["ms"] / r["off"]["ms"], 3)
    r["verdict"] = "win" if r["on_over_off"] < 1.0 else "LOSS"
    return r


def calls(m, path, a):
    rng = np.random.default_rng(5)
    toks = [2] + [int(v) for v in rng.integers(4, LARGE["n_vocab"], 2047)]
    new, old = m.BiogptModel.load(path, long_context=True), m.BiogptModel.load(path, long_context=False)
    res = {}
    both = lambda f: alternating([lambda: f(new), lambda: f(old)], a.reps, a.warmup)
    res["prompt2048"] = row(*both(lambda g: g.eval_prompt(toks, 0, 2048)))
    res["prompt2048_by8"] = row(*both(lambda g: g.eval_prompt(toks, 0, 8)))
    for g in (new, old):      # (the prompt above left 2048 keys in both caches: every row below reads keys that are there)
        g.eval_prompt(toks, 0, 2048)
    res["eval64_at_1984"] = row(*both(lambda g: g.eval(toks[1984:2048], 1984)))
    res["eval8_at_1500"] = row(*both(lambda g: g.eval(toks[1500:1508], 1500)))
    res["token_at_1100"] = row(*both(lambda g: g.eval(toks[1099:1100], 1099)))
    res["token_at_2040"] = row(*both(lambda g: g.eval(toks[2039:2040], 2039)))
    res["greedy_1400+200"] = row(*both(lambda g: g.generate_greedy(toks[:1400], 200)))
    res["long_attn_launches"] = new.long_attn_launches()
    new.close(); old.close()
    return res


def kernels(m, a):
    rng = np.random.default_rng(7)
    K, V = (rng.standard_normal((H, 2048, 64)).astype(np.float32) for _ in range(2))
    q = (rng.standard_normal((512, H * 64)) * 0.125).astype(np.float32)
    out = {}

    def generic_us(N, P, t_max, state):
        rows = (N + 15) // 16 * 16 + 1
        o, us = np.zeros((rows, H * 64), np.float32), np.zeros(a.reps, np.float32)
        rc = m.lib().biogpt_hip_attn_device_bench(0, GENERIC if t_max > 1024 else TILE, H, 64, N, P, t_max, 1, q.ctypes.data, K.ctypes.data, V.ctypes.data, state.ctypes.data, None, 0, 0,
                                                  o.ctypes.data, None, None, None, a.reps, us.ctypes.data)
        if rc != 0:
            raise m.BiogptError(m._err())
        return us

    def one(name, form, N, t_max, P=2048):
        state = np.array([t_max - N, 0, 0, 0], dtype=np.int32)
        new = m.attn_long_device(form, H, N, P, t_max, q, K, V, state, q8=1, reps=a.reps)
        if new[0] != 0:
            raise m.BiogptError(m._err())
        r = dict(long_us=round(float(np.median(new[6])), 2), existing_us=round(float(np.median(generic_us(N, P, t_max, state))), 2))
        r["long_over_existing"] = round(r["long_us"] / r["existing_us"], 3)
        r["verdict"] = "win" if r["long_over_existing"] < 1.0 else "LOSS"
        out[name] = r

    for T in (1025, 1536, 2048):
        one("col_N1_T%d" % T, 0, 1, T)
        one("col_N8_T%d" % T, 0, 8, T)
        one("tile_N128_T%d" % T, 1, 128, T)
    # the tile kernel below its own range is not launched by the engine or the probe: at 1025 keys on 512 columns against attn_tile_kernel at 1024 keys
    state = np.array([1025 - 512, 0, 0, 0], dtype=np.int32)
    new = m.attn_long_device(1, H, 512, 2048, 1025, q, K, V, state, q8=1, reps=a.reps)
    if new[0] != 0:
        raise m.BiogptError(m._err())
    old = generic_us(512, 2048, 1024, np.array([512, 0, 0, 0], dtype=np.int32))
    r = dict(long_us_at_1025=round(float(np.median(new[6])), 2), tile_us_at_1024=round(float(np.median(old)), 2))
    r["long_over_existing"] = round(r["long_us_at_1025"] / r["tile_us_at_1024"], 3)
    r["verdict"] = "win" if r["long_over_existing"] < 1.0 else "LOSS"
    out["tile_N512_T1025_vs_tile_kernel_T1024"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--types", default="q4_0,q5_1,q8_0")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.lib()
    res = {"metric": "long_context_bench", "model": "synthetic BioGPT-Large sizes, %d layers, %d positions" % (a.layers, LARGE_2048["n_positions"]), "reps": a.reps,
           "warmup": a.warmup}
    if not a.skip_kernels:
        res["kernels"] = kernels(m, a)
    with tempfile.TemporaryDirectory() as td:
        f32 = os.path.join(td, "f32.bin")
        if not a.skip_calls:
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **LARGE_2048)
        for name in a.types.split(","):
            if a.skip_calls:
                break
            print("long_context_bench: %s" % name, file=sys.stderr, flush=True)
            path = os.path.join(td, name + ".bin")
            m.quantize_file(f32, path, name)
            res[name] = calls(m, path, a)
            os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
