#!/usr/bin/env python3
"""Sampled generation on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed): milliseconds per call by host wall clock (every call
returns after its stream has drained), after a warm-up, `--reps` repeats (median, min, max).  top_k 40, top_p 0.9, temp 0.9, a 40-token prompt,
n_predict 64, no EOS.  Prints one JSON line:

  sample_N      biogpt_hip_generate_sample with N sequences (N different prompts, one sample each) against biogpt_hip_generate_greedy_batch of
                the same prompts in the same process, and the ratio sample / greedy_batch
  shared_8      8 samples of ONE prompt as one call, against 8 serial runs of the host-sampling loop: per token one biogpt_hip_eval_topk and the
                draw on the host (biogpt_hip_sample_candidates_host) -- the route of the compat layer's biogpt_eval_sample_top_k_top_p

  python tools/sample_bench.py [--reps 7] [--warmup 2] [--only 64]    (--only: one sequence count, sample calls only, e.g. under a kernel trace)
"""
import argparse
import ctypes
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
N_PROMPT, N_PREDICT = 40, 64
TOP_K, TOP_P, TEMP = 40, 0.9, 0.9


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(float(np.median(ts)), 4), min=round(float(np.min(ts)), 4), max=round(float(np.max(ts)), 4), n=reps)


def host_loop(m, g, prompt, seed):
    """main.cpp's loop with the top-k selection on the device and the draw on the host."""
    L = m.lib()
    st = np.zeros(625, dtype=np.uint32)
    L.biogpt_hip_mt19937_seed(seed, st.ctypes.data)
    out = ctypes.c_int32(0)
    vals, ids = None, None
    for at in range(0, len(prompt), 8):
        vals, ids = g.eval_topk(prompt[at:at + 8], at, TOP_K)
    toks, n_past = [], len(prompt)
    for k in range(N_PREDICT):
        L.biogpt_hip_sample_candidates_host(vals.ctypes.data, ids.ctypes.data, vals.size, TOP_P, TEMP, st.ctypes.data, ctypes.byref(out))
        toks.append(int(out.value))
        if k + 1 < N_PREDICT:
            vals, ids = g.eval_topk([toks[-1]], n_past, TOP_K)
            n_past += 1
    return toks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, default=0)
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.build()
    res = {"metric": "sample_bench", "model": "synthetic BioGPT-base, 24 layers, q4_0", "n_prompt": N_PROMPT, "n_predict": N_PREDICT,
           "top_k": TOP_K, "top_p": TOP_P, "temp": TEMP, "eos_id": -1, "reps": a.reps, "warmup": a.warmup}
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED)
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        g = m.BiogptModel.load(q40)
        prompts = [[2] + [int(v) for v in rng.integers(4, g.n_vocab, N_PROMPT - 1)] for _ in range(256)]
        kw = dict(top_k=TOP_K, top_p=TOP_P, temp=TEMP, seed=1, eos_id=-1, n_batch=8)
        for n in ([a.only] if a.only else [8, 64, 256]):
            sm = timed(lambda: g.generate_sample(prompts[:n], N_PREDICT, **kw), a.reps, a.warmup)
            r = dict(sample=sm, sample_ms_per_step=round(sm["ms"] / N_PREDICT, 4), tok_per_s=round(n * N_PREDICT / sm["ms"] * 1e3, 1))
            if not a.only:
                gb = timed(lambda: g.generate_greedy_batch(prompts[:n], N_PREDICT, n_batch=8), a.reps, a.warmup)
                r.update(greedy_batch=gb, greedy_batch_ms_per_step=round(gb["ms"] / N_PREDICT, 4), ratio=round(sm["ms"] / gb["ms"], 4))
            res["sample_%d" % n] = r
        if not a.only:
            sh = timed(lambda: g.generate_sample([prompts[0]], N_PREDICT, n_samples=8, **kw), a.reps, a.warmup)
            hl = timed(lambda: [host_loop(m, g, prompts[0], 1 + j) for j in range(8)], a.reps, a.warmup)
            same = [list(s) for s in g.generate_sample([prompts[0]], N_PREDICT, n_samples=8, **kw)[0]] == [host_loop(m, g, prompts[0], 1 + j) for j in range(8)]
            res["shared_8"] = dict(sample=sh, host_loop_x8=hl, speedup=round(hl["ms"] / sh["ms"], 3), same_ids=bool(same))
        g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
