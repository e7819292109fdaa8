#!/usr/bin/env python3
"""Shared-prefix scoring of a dataset in one call (score_continuations_batch) on the synthetic 24-layer BioGPT-base model, Q4_0 (bench.py's seed), against the
yardstick: a loop of score_continuations over the groups -- an unchanged function of the same build, the code path of the parent commit.  Milliseconds per
dataset by host wall clock (every call returns after its stream has drained), warm-up 2, median of 9 with min - max; the two routes alternate call by call in
one process, so both see the same clocks.

  rows   16 / 64 / 128 groups of three one-token continuations behind 384 tokens (yes / no / maybe)
         8 groups of 32 eight-token continuations behind 384 tokens
         64 groups of three one-token continuations behind 64 tokens
         one group of 64 eight-token continuations behind 384 tokens, against the single call (no pass is saved: only the attention kernel can gain)

One JSON line per row: medians and ranges of both routes, ratio = batch / loop, prefix_batch_stats().  BIOGPT_HIP_RUN_ATTN is taken from the environment.
--ab: every row with BIOGPT_HIP_RUN_ATTN=0 and =1, each arm in a process of its own (the switch is read when a model is loaded; one context of 512 slots
is 96 GiB of K / V cache), then per row runs / fast = the ratio of the two batch medians.  --kernel: the attn_runs_kernel probe alone (16 heads, one layer;
a repeated stand-alone launch finds its K / V rows in cache, so these figures flatter a kernel that loads less).

  python tools/prefix_batch_bench.py [--ab | --kernel] [--reps 9] [--warmup 2] [--rows 0,1,2,3,4,5]
"""
import argparse
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
ROWS = [  # name, groups, n_prefix, candidates per group, tokens per candidate
    ("16 x 3 x 1 behind 384", 16, 384, 3, 1),
    ("64 x 3 x 1 behind 384", 64, 384, 3, 1),
    ("128 x 3 x 1 behind 384", 128, 384, 3, 1),
    ("8 x 32 x 8 behind 384", 8, 384, 32, 8),
    ("64 x 3 x 1 behind 64", 64, 64, 3, 1),
    ("1 x 64 x 8 behind 384", 1, 384, 64, 8),
    # one small example per call: a single pass of 386 / 66 / 18 columns (where the default routing has its threshold)
    ("1 x 3 x 1 behind 384", 1, 384, 3, 1),
    ("1 x 3 x 1 behind 64", 1, 64, 3, 1),
    ("1 x 3 x 1 behind 16", 1, 16, 3, 1),
    ("1 x 3 x 1 behind 128", 1, 128, 3, 1),
    ("1 x 3 x 1 behind 256", 1, 256, 3, 1),
    ("2 x 3 x 1 behind 64", 2, 64, 3, 1),
    ("6 x 3 x 1 behind 64", 6, 64, 3, 1),
]


def timed_pair(fa, fb, reps, warmup):
    ta, tb = [], []
    for r in range(warmup + reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
    return ta, tb


def stats(ts):
    med = float(np.median(ts))
    return {"median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def ints(s):
    return [int(v) for v in s.split(",") if v]


def dataset(V, row):
    _, n_groups, n_prefix, n_cand, n_tok = ROWS[row]
    rng = np.random.default_rng([row, n_groups])
    prefixes = [[2] + [int(v) for v in rng.integers(4, V, n_prefix - 1)] for _ in range(n_groups)]
    conts = [[[int(v) for v in rng.integers(4, V, n_tok)] for _ in range(n_cand)] for _ in range(n_groups)]
    return prefixes, conts


def call_level(m, path, a):
    g = m.BiogptModel.load(path, device=0)
    V = g.hparams.n_vocab
    run_attn = int(os.environ.get("BIOGPT_HIP_RUN_ATTN", "-1"))
    for row in a.rows:
        prefixes, conts = dataset(V, row)
        out = {"mode": "call", "row": ROWS[row][0], "run_attn": run_attn}
        try:
            got = g.score_continuations_batch(prefixes, conts)
        except m.BiogptError as e:
            out["not_measured"] = str(e)
            print(json.dumps(out), flush=True)
            continue
        out["stats"] = g.prefix_batch_stats()
        loop = lambda: [g.score_continuations(p, c) for p, c in zip(prefixes, conts)]
        want = loop()
        diff = sum(int((x != y).sum()) for gg, ww in zip(got, want) for t, u in zip(gg, ww) for x, y in zip(t, u))
        worst = max(float(np.abs(t[0] - u[0]).max()) for gg, ww in zip(got, want) for t, u in zip(gg, ww))
        out["values_differing_from_loop"], out["max_logprob_diff"] = diff, worst
        tb, tl = timed_pair(lambda: g.score_continuations_batch(prefixes, conts), loop, a.reps, a.warmup)
        out["batch"], out["loop"] = stats(tb), stats(tl)
        out["ratio"] = round(out["batch"]["median_ms"] / out["loop"]["median_ms"], 4)
        out["ms_per_group"] = round(out["batch"]["median_ms"] / len(prefixes), 4)
        print(json.dumps(out), flush=True)
    g.close()


def kernel_level(m, reps):
    """attn_runs_kernel alone: a pure prefix pass of 512 columns of one prompt at several depths, and 384 candidates of 128 groups behind 383 rows."""
    Hh = 16
    rng = np.random.default_rng(1)
    cases = [("512 prefix columns, rows %d .. %d" % (t0, t0 + 511), [(0, 0, t0 + k, 0, 0) for k in range(512)], 1) for t0 in (1, 257, 513)]
    cases.append(("128 groups x 3 candidates behind 383 rows", [(128 + 3 * g + c, 383, 384, 383, g) for g in range(128) for c in range(3)], 512))
    for name, cols, n_slots in cases:
        N, P = len(cols), 1024
        st = np.zeros((N, 8), dtype=np.int32)
        for i, (sid, _, tv, p0, p1) in enumerate(cols):
            st[i, 0], st[i, 3], st[i, 4], st[i, 5], st[i, 6] = tv - 1, sid, tv, p0, p1
        blk = rng.standard_normal((1, Hh, P, 64)).astype(np.float32)
        k = np.ascontiguousarray(np.broadcast_to(blk, (n_slots, Hh, P, 64)))
        v = np.ascontiguousarray(k[:, :, ::-1])
        q = rng.standard_normal((N, Hh * 64)).astype(np.float32)
        rc, _, _, _, _, launched, us = m.attn_runs_device(Hh, P, int(st[:, 4].max()), n_slots, q, k, v, st, q8=1, reps=reps)
        assert rc == 0, m._err()
        us = us[2:]
        print(json.dumps({"mode": "kernel", "case": name, "columns": N, "runs": int(launched[6]),
                          "runs_us": {"median": round(float(np.median(us)), 2), "min": round(float(us.min()), 2), "max": round(float(us.max()), 2)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=ints, default=list(range(len(ROWS))))
    ap.add_argument("--kernel", action="store_true", help="the attn_runs_kernel probe alone")
    ap.add_argument("--ab", action="store_true", help="BIOGPT_HIP_RUN_ATTN=0 against =1, each arm in a process of its own")
    ap.add_argument("--model", default=None, help="a 24-layer Q4_0 file written before (the arms of --ab)")
    a = ap.parse_args()
    import _pkg
    m = _pkg.load()
    m.lib()
    if a.kernel:
        kernel_level(m, a.reps + 2)
        return
    if a.model:
        call_level(m, a.model, a)
        return
    with tempfile.TemporaryDirectory() as td:
        f32, q40 = os.path.join(td, "f32.bin"), os.path.join(td, "q4_0.bin")
        m.write_synthetic(f32, seed=SEED, **{k: v for k, v in m.BIOGPT_BASE.items() if k != "ftype"})
        m.quantize_file(f32, q40, "q4_0")
        os.remove(f32)
        if not a.ab:
            call_level(m, q40, a)
            return
        arms = {}
        for val in ("0", "1"):      # this process never opens the device: one arm at a time holds it
            env = dict(os.environ, BIOGPT_HIP_RUN_ATTN=val)
            cmd = [sys.executable, os.path.abspath(__file__), "--model", q40, "--reps", str(a.reps), "--warmup", str(a.warmup), "--rows", ",".join(str(r) for r in a.rows)]
            res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True)
            sys.stdout.write(res.stdout)
            arms[val] = {r["row"]: r for r in (json.loads(line) for line in res.stdout.splitlines() if line.startswith("{"))}
        for row in a.rows:
            name = ROWS[row][0]
            r0, r1 = arms["0"].get(name, {}), arms["1"].get(name, {})
            if "batch" in r0 and "batch" in r1:
                print(json.dumps({"mode": "ab", "row": name, "fast_ms": r0["batch"]["median_ms"], "runs_ms": r1["batch"]["median_ms"],
                                  "runs_over_fast": round(r1["batch"]["median_ms"] / r0["batch"]["median_ms"], 4),
                                  "fast_over_loop": r0["ratio"], "runs_over_loop": r1["ratio"]}), flush=True)


if __name__ == "__main__":
    main()
