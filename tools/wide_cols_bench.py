#!/usr/bin/env python3
"""The wide column layer (biogpt_hip_wide_cols) on synthetic files at BioGPT-Large's sizes (d_model 1600, d_ff 6400, 25 heads, n_vocab 57717, 1024 positions),
Q4_0 / Q5_1 / Q8_0: host wall clock around calls that return after their stream has drained, warm-up 2, median of 9 (min - max), the two routes of a row
alternating in one process.  The yardstick of every row is the same build with the switch off: the same file in a second context.  Prints one JSON line.

  greedy_batch_N  generate_greedy_batch of N = 1, 2, 5, 8, 16 sequences: 16-token prompts + 64 new tokens
  beam_5          generate_beam of a 16-token prompt, five beams, 64 new tokens
  queue_16        generate_queue of 24 requests of 32 new tokens over max_columns = 16
  stages          each linear stage alone at N = 1, 2, 5, 8, 16 columns by device events through the probe's timing loop -- wcols_kernel against matmul_wide_kernel
                  on the same image and columns -- at (K, M) = (1600, 4800) q/k/v, (1600, 1600) out_proj, (1600, 6400) fc1, (6400, 1600) fc2

  python tools/wide_cols_bench.py [--layers 48] [--types q4_0,q5_1,q8_0] [--reps 9] [--warmup 2] [--skip-stages] [--skip-calls]
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

COLS = (1, 2, 5, 8, 16)
EPIS = {"QKV": "QKV", "OPROJ": "RESID", "FC1": "GELU", "FC2": "RESID"}


def row(on, off):
    r = dict(cols=stats(on), off=stats(off))
    r["cols_over_off"] = round(r["cols"]["ms"] / r["off"]["ms"], 3)
    r["verdict"] = "win" if r["cols_over_off"] < 1.0 else "LOSS"
    return r


def calls(m, path, a):
    rng = np.random.default_rng(5)
    prompts = [[2] + [int(v) for v in rng.integers(4, LARGE["n_vocab"], 15)] for _ in range(24)]
    on, off = m.BiogptModel.load(path, wide_cols=True), m.BiogptModel.load(path, wide_cols=False)
    res = {}
    for n in COLS:
        res["greedy_batch_%d" % n] = row(*alternating([lambda g=g: g.generate_greedy_batch(prompts[:n], 64) for g in (on, off)], a.reps, a.warmup))
    beam = dict(n_beams=5, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)
    res["beam_5"] = row(*alternating([lambda g=g: g.generate_beam(prompts[0], 64, **beam) for g in (on, off)], a.reps, a.warmup))
    queue = dict(max_columns=16, group=2, top_k=40, top_p=0.95, temp=1.0, seeds=list(range(1, 25)), eos_id=-1, n_batch=8)
    res["queue_16"] = row(*alternating([lambda g=g: g.generate_queue(prompts, 32, **queue) for g in (on, off)], a.reps, a.warmup))
    res["cols_launches"], res["off_cols_launches"] = on.wide_cols_launches(), off.wide_cols_launches()
    on.close(); off.close()
    return res


def stages(m, wtype, a):
    out = {}
    for name, K, M in STAGES:
        for N in COLS:
            z = dict(w_rows=np.full(M * (K // 32) * BLOCK_BYTES[wtype], 0x11, np.uint8), bias=np.zeros(M, np.float32), reps=a.reps, aq_q=np.ones((N, K), np.int8),
                     aq_d=np.ones((N, K // 32), np.float32), aq_s=np.full((N, K // 32), 32, np.uint32))
            if EPIS[name] == "RESID":
                z.update(resid=np.zeros((N, M), np.float32))
            if name == "QKV":
                z.update(k_slots=np.zeros((1, K // 64, 32, 64), np.float32), v_slots=np.zeros((1, K // 64, 32, 64), np.float32), P=32, dev_state=np.array([1, 0, 0, 0], np.int32))
            us = {w: float(np.median(m.wcols_device(EPIS[name], wtype, M, K, N, which=w, **z)["us"])) for w in ("cols", "wide")}
            out["%s_%d" % (name, N)] = dict(cols_us=round(us["cols"], 2), wide_us=round(us["wide"], 2), verdict="win" if us["cols"] < us["wide"] else "LOSS")
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
    res = {"metric": "wide_cols_bench", "model": "synthetic BioGPT-Large sizes, %d layers, %d positions" % (a.layers, LARGE["n_positions"]), "reps": a.reps,
           "warmup": a.warmup}
    with tempfile.TemporaryDirectory() as td:
        f32 = os.path.join(td, "f32.bin")
        if not a.skip_calls:
            m.write_synthetic(f32, seed=SEED, n_layer=a.layers, **LARGE)
        for name in a.types.split(","):
            print("wide_cols_bench: %s" % name, file=sys.stderr, flush=True)
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
