#!/usr/bin/env python3
"""Beam search over a batch of prompts on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per call by host wall
clock (every call returns after its stream has drained), after a warm-up, `--reps` repeats (median, min, max).  B = 5 beams, 40-token prompts,
n_predict 64, no EOS (every search runs all 64 steps), early_stopping.  Prints one JSON line:

  batch_G       biogpt_hip_generate_beam_batch of G prompts (G in --groups, default 1, 8, 51, 102), against
                  serial        a loop of G biogpt_hip_generate_beam calls with the library --yardstick-lib names (the commit before this
                                feature), in a process of its own; `--rounds` rounds alternate the two builds
                  greedy_batch  biogpt_hip_generate_greedy_batch of G * B sequences, in the batched call's process
  beam_single   biogpt_hip_generate_beam of one prompt on both builds

  python tools/beam_batch_bench.py [--yardstick-lib PATH] [--reps 7] [--warmup 2] [--rounds 2] [--groups 1,8,51,102]
  python tools/beam_batch_bench.py --only 51      (one batched call size alone in this process, e.g. under a kernel trace)

Without --yardstick-lib the serial loop runs on this build (then it is no acceptance figure, and the JSON says so)."""
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
N_PROMPT, N_PREDICT, N_BEAMS = 40, 64, 5
KW = dict(n_beams=N_BEAMS, eos_id=-1, length_penalty=1.0, early_stopping=True, n_batch=8)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(float(np.median(ts)), 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4), n=reps)


def prompts_of(n_vocab, n):
    rng = np.random.default_rng(7)
    return [[2] + [int(v) for v in rng.integers(4, n_vocab, N_PROMPT - 1)] for _ in range(n)]


def measure(role, model, groups, reps, warmup):
    """One side's timings in THIS process, with whatever library BIOGPT_HIP_LIB names (default: this build's)."""
    import _pkg
    m = _pkg.load()
    raw = ctypes.CDLL(m.LIB_PATH)
    m.SYMBOLS[:] = [s for s in m.SYMBOLS if hasattr(raw, s[0])]      # (an older build exports fewer symbols)
    g = m.BiogptModel.load(model)
    prompts = prompts_of(g.n_vocab, max(groups))
    res = {"lib": m.LIB_PATH, "beam_single": timed(lambda: g.generate_beam(prompts[0], N_PREDICT, **KW), reps, warmup)}
    for G in groups:
        if role == "serial":
            res["serial_%d" % G] = timed(lambda: [g.generate_beam(p, N_PREDICT, **KW) for p in prompts[:G]], reps, warmup)
        else:
            res["batch_%d" % G] = timed(lambda: g.generate_beam_batch(prompts[:G], N_PREDICT, **KW), reps, warmup)
            if role == "batch":
                res["greedy_batch_%d" % (G * N_BEAMS)] = timed(lambda: g.generate_greedy_batch([prompts[i // N_BEAMS] for i in range(G * N_BEAMS)], N_PREDICT,
                                                                                                n_batch=8), reps, warmup)
    g.close()
    return res


def child(role, model, a, lib):
    env = dict(os.environ)
    if lib:
        env["BIOGPT_HIP_LIB"] = os.path.abspath(lib)
    else:
        env.pop("BIOGPT_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", role, "--model", model, "--reps", str(a.reps), "--warmup", str(a.warmup),
                          "--groups", a.groups], env=env, stdout=subprocess.PIPE, timeout=900, check=True).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def summary(rounds, key):
    meds = [r[key]["ms"] for r in rounds]
    return dict(ms=round(float(np.median(meds)), 4), round_medians=meds, min=min(r[key]["min"] for r in rounds), max=max(r[key]["max"] for r in rounds),
                spread=round((max(r[key]["max"] for r in rounds) - min(r[key]["min"] for r in rounds)) / float(np.median(meds)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--groups", default="1,8,51,102")
    ap.add_argument("--yardstick-lib", default="")
    ap.add_argument("--only", type=int, default=0)
    ap.add_argument("--role", default="")      # internal: one side's timings of a given model file
    ap.add_argument("--model", default="")
    a = ap.parse_args()
    groups = [int(v) for v in a.groups.split(",")]
    if a.role:
        print(json.dumps(measure(a.role, a.model, groups, a.reps, a.warmup)))
        return
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "beam_batch_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_prompt": N_PROMPT, "n_predict": N_PREDICT, "n_beams": N_BEAMS,
           "eos_id": -1, "reps": a.reps, "warmup": a.warmup, "rounds": a.rounds,
           "yardstick": os.path.abspath(a.yardstick_lib) if a.yardstick_lib else "this build (not another build: no acceptance figure)"}
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        if a.only:
            res["batch_%d" % a.only] = measure("batch_only", q40, [a.only], a.reps, a.warmup)["batch_%d" % a.only]
            print(json.dumps(res))
            return
        ss, bs = [], []
        for _ in range(a.rounds):      # alternate the two builds
            ss.append(child("serial", q40, a, a.yardstick_lib))
            bs.append(child("batch", q40, a, ""))
    res["beam_single"] = dict(this=summary(bs, "beam_single"), yardstick=summary(ss, "beam_single"))
    res["beam_single"]["ratio"] = round(res["beam_single"]["this"]["ms"] / res["beam_single"]["yardstick"]["ms"], 4)
    for G in groups:
        b, s, gb = summary(bs, "batch_%d" % G), summary(ss, "serial_%d" % G), summary(bs, "greedy_batch_%d" % (G * N_BEAMS))
        res["batch_%d" % G] = dict(batch=b, serial=s, greedy_batch=gb, speedup_over_serial=round(s["ms"] / b["ms"], 3),
                                   ratio_to_greedy_batch=round(b["ms"] / gb["ms"], 4), hyp_tok_per_s=round(G * N_BEAMS * N_PREDICT / b["ms"] * 1e3, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
